// Host check of ffmi::plan_gemm (csrc/kernels/gemm_plan.h): built with the
// address and undefined-behaviour sanitizers together with gemm_plan.cpp and
// run by tests/test_gemm_plan_host.py.  No device, no HIP.
//  1. Over T 1..1100 x the shapes of tests/test_gemm_planner.py (its SWEEP and
//     the LLaMA layers at TP 1/2/4/8) x both epilogues x the X/Y-packed and
//     W-stream flags x deferrable x fuse kind (T <= 32) x workspace {none,
//     exact, exact - 1, unlimited}: every valid plan is instantiated, its
//     grid is non-empty, 1 <= S <= min(8, K/32), the slabs are S*T*ntiles*16*4
//     bytes, a clamped plan is unsplit, 4 row tiles per wave never meet more
//     than 8 weight tiles, and gemm_workspace_bytes covers the plan's need.
//  2. The FFMI_GEMM_PLAN parser: the strings of test_gemm_planner.py and
//     hostile ones (empty, only ';', 64 KiB of digits, 10 000 entries).
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "../flexflow_amd/csrc/kernels/gemm_plan.h"

using namespace ffmi;

static long fails = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      if (fails++ < 20) {                \
        std::printf("FAIL %s: ", #cond); \
        std::printf(__VA_ARGS__);        \
        std::printf("\n");               \
      }                                  \
    }                                    \
  } while (0)

static const size_t kUnlimited = (size_t)-1;

static std::vector<std::pair<int, int>> shapes() {
  std::set<std::pair<int, int>> s = {{200, 288},   {224, 1056},   {4096, 64},
                                     {1000, 8192}, {11008, 4096}, {4096, 11008}};
  // (hidden, intermediate, heads, vocab) of LLaMA 68M / 7B / 13B / 65B
  const int llama[4][4] = {{768, 3072, 12, 32000}, {4096, 11008, 32, 32000},
                           {5120, 13824, 40, 32000}, {8192, 22016, 64, 32000}};
  for (auto &m : llama)
    for (int tp : {1, 2, 4, 8}) {
      const int H = m[0], I = m[1], heads = m[2], V = m[3];
      if (heads % tp) continue;
      const int Vl = tp > 1 && (V / tp) % 16 == 0 ? V / tp : V;
      s.insert({3 * H / tp, H}), s.insert({H, H / tp}), s.insert({I / tp, H});
      s.insert({H, I / tp}), s.insert({Vl, H});
    }
  return {s.begin(), s.end()};
}

static long plans = 0;

// ws: the workspace offered; all: gemm_workspace_bytes of the shape
static void check_plan(const GemmPlan &p, int T, int N, int K, int flags, bool deferrable,
                       size_t ws, size_t all) {
  ++plans;
  const int epi = flags & 1;
#define WHERE "T %d N %d K %d flags %#x defer %d ws %zu", T, N, K, flags, (int)deferrable, ws
  CHECK(plan_instantiated(p), WHERE);
  CHECK(p.grid[0] >= 1 && p.grid[1] >= 1 && p.grid[2] >= 1 && p.block >= 64 && p.block <= 512, WHERE);
  CHECK(p.S >= 1 && p.S <= std::min(8, K / 32), WHERE);
  CHECK(p.ntiles == (N + 15) / 16 * (epi ? 2 : 1) && p.KT == K / 32, WHERE);
  const size_t need = (size_t)p.S * T * p.ntiles * 16 * 4;
  CHECK(p.slab_bytes == (p.S > 1 ? need : 0), WHERE);
  CHECK(p.slab_bytes <= ws, WHERE);
  CHECK(!(p.MTW == 4 && p.NTW > 8), WHERE);
  CHECK(all >= p.slab_bytes, WHERE);
  CHECK(!p.defer || (p.S > 1 && deferrable && !epi), WHERE);
  CHECK(p.S == 1 || p.defer || p.MAXS >= p.S, WHERE);
  CHECK(p.form != GEMM_TILE || ((flags & FFMI_X_PACKED) && T >= 497), WHERE);
  CHECK((p.form == GEMM_MID || p.form == GEMM_TILE) == (T > 64), WHERE);
  CHECK(p.form != GEMM_MID || (p.grid[0] == (unsigned)p.nblk && p.grid[1] == (unsigned)p.S &&
                               p.grid[2] == (unsigned)p.mblocks),
        WHERE);
#undef WHERE
}

static void sweep() {
#define AT "T %d N %d K %d flags %#x defer %d", T, N, K, flags, deferrable
  for (const auto &nk : shapes())
    for (int T = 1; T <= 1100; ++T)
      for (int epi = 0; epi < 2; ++epi)
        for (int f = 0; f < 8; ++f) {
          const int N = nk.first, K = nk.second;
          const int flags = epi | (f & 1 ? FFMI_X_PACKED : 0) | (f & 2 ? FFMI_Y_PACKED : 0) |
                            (f & 4 ? FFMI_W_STREAM : 0);
          const size_t all = gemm_workspace_bytes(T, N, K, flags);
          for (int deferrable = 0; deferrable < 2; ++deferrable) {
            const GemmPlan u = plan_gemm(T, N, K, flags, deferrable, 0, kUnlimited);
            CHECK(u.valid == !((f & 2) && N % 32), AT);
            if (!u.valid) continue;
            check_plan(u, T, N, K, flags, deferrable, kUnlimited, all);
            const GemmPlan none = plan_gemm(T, N, K, flags, deferrable, 0, 0);
            CHECK(none.valid && none.S == 1 && none.slab_bytes == 0, AT);
            check_plan(none, T, N, K, flags, deferrable, 0, all);
            if (u.S > 1) {
              const GemmPlan exact = plan_gemm(T, N, K, flags, deferrable, 0, u.slab_bytes);
              CHECK(exact.valid && exact.S == u.S && exact.form == u.form, AT);
              check_plan(exact, T, N, K, flags, deferrable, u.slab_bytes, all);
              const GemmPlan less = plan_gemm(T, N, K, flags, deferrable, 0, u.slab_bytes - 1);
              CHECK(less.valid && less.S == 1 && less.slab_bytes == 0, AT);
              check_plan(less, T, N, K, flags, deferrable, u.slab_bytes - 1, all);
            }
            if (T > 32) continue;
            for (int kind = 1; kind <= 2; ++kind)
              for (size_t ws : {(size_t)0, kUnlimited}) {
                const GemmPlan z = plan_gemm(T, N, K, flags, deferrable, kind, ws);
                const bool ok = N % 16 == 0 && (kind == 1 ? !epi && !(f & 2) : !(f & 1)) &&
                                !((f & 2) && N % 32);
                CHECK(z.valid == ok, "kind %d " AT, kind);
                if (!z.valid) continue;
                check_plan(z, T, N, K, flags, deferrable, ws, all);
                CHECK(z.form == GEMM_SKINNY && z.FZ == kind && z.S == 1 && z.MT == (T + 15) / 16,
                      "kind %d " AT, kind);
              }
          }
        }
#undef AT
}

// {MTW, NTW, S} of the hook's plan (ffmi_linear: not deferrable, any workspace)
static std::tuple<int, int, int> hook(int T, int N, int K) {
  int v[6];
  gemm_debug_plan(T, N, K, 0, v);
  const GemmPlan p = plan_gemm(T, N, K, 0, false, 0, kUnlimited);
  CHECK(p.valid && plan_instantiated(p) && v[0] == GEMM_MID && p.form == GEMM_MID && v[1] == p.MTW &&
            v[2] == p.NTW && v[3] == p.S && v[4] == p.mblocks && v[5] == p.nblk,
        "hook T %d N %d K %d", T, N, K);
  return {v[1], v[2], v[3]};
}

static void parser() {
  const int T = 168, N = 4096, K = 288;  // KT = 9
  unsetenv("FFMI_GEMM_PLAN");
  const auto own = hook(T, N, K);
  for (int ntw : {2, 4, 6, 8, 12, 16})
    for (int S = 1; S <= 8; ++S) {
      setenv("FFMI_GEMM_PLAN", (std::to_string(ntw) + "," + std::to_string(S)).c_str(), 1);
      CHECK(hook(T, N, K) == std::make_tuple(3, ntw, S), "forced %d,%d", ntw, S);
    }
  std::vector<std::string> bad = {"3,2", "5,1", "10,2", "32,1", "0,1", "8,9", "8,0", "8,-1", "8",
                                  "x",   "",    ";",    ";;;;", " ",   ",",   ":", "::,", "8,", ",2"};
  bad.push_back(std::string(4096, ';'));
  bad.push_back(std::string(64 << 10, '7'));                          // one number, out of range
  bad.push_back(std::string(64 << 10, '7') + "," + std::string(64 << 10, '7'));
  bad.push_back("4096:288:" + std::string(64 << 10, '1') + ",2");
  for (const auto &b : bad) {
    setenv("FFMI_GEMM_PLAN", b.c_str(), 1);
    CHECK(hook(T, N, K) == own, "bad string '%.20s' (%zu chars)", b.c_str(), b.size());
  }
  // 10 000 listed shapes: other shapes, invalid entries for this one, then its plan last
  std::string list;
  for (int i = 0; i < 10000; ++i)
    list += i % 100 == 7 ? "4096:288:5,2;" : std::to_string(100000 + i) + ":288:12,2;";
  setenv("FFMI_GEMM_PLAN", list.c_str(), 1);
  CHECK(hook(T, N, K) == own, "long list without a plan for the shape");
  setenv("FFMI_GEMM_PLAN", (list + "4096:288:6,3").c_str(), 1);
  CHECK(hook(T, N, K) == std::make_tuple(3, 6, 3), "long list, plan in the last entry");
  // more slices than k-steps; the other paths are not touched
  setenv("FFMI_GEMM_PLAN", "8,4", 1);
  CHECK(std::get<2>(hook(T, N, 96)) <= 3, "S = 4 > KT = 3");
  setenv("FFMI_GEMM_PLAN", "8,2", 1);
  CHECK(plan_gemm(32, 4096, 4096, 0, false, 0, kUnlimited).form == GEMM_SKINNY, "skinny");
  // a forced split is still clamped by the workspace
  const GemmPlan c = plan_gemm(T, N, K, 0, false, 0, 1000);
  CHECK(c.valid && c.NTW == 8 && c.S == 1 && c.slab_bytes == 0, "forced plan, short workspace");
  unsetenv("FFMI_GEMM_PLAN");
  CHECK(hook(T, N, K) == own, "unset");
}

int main() {
  parser();
  sweep();
  std::printf("%ld plans, %ld failures\n", plans, fails);
  return fails ? 1 : 0;
}
