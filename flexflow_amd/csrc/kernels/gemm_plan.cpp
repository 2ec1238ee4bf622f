// gemm_plan.cpp -- the GEMM launch planner (gemm_plan.h): host code only.
#include "gemm_plan.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

namespace ffmi {

// ---------------------------------------------------------------------------
// Environment switches of the GEMM, all of them (A/B runs, diagnostics and
// tests; none is needed in production).  Lifetime: "once" = read at the first
// launch or query that reaches the switch and kept for the process; "load" =
// read when the library is loaded; "call" = read on every call (tests flip
// these with monkeypatch).
// ---------------------------------------------------------------------------
static int env_int(const char *name, int unset) {
  const char *e = getenv(name);
  return e ? atoi(e) : unset;
}
struct Pair { int a, b; };
static Pair env_pair(const char *name, int a, int b) {
  Pair p{a, b};
  if (const char *e = getenv(name)) (void)sscanf(e, "%d,%d", &p.a, &p.b);
  return p;
}
// FFMI_SKINNY_PIPE=0|1: skinny k-loop never / always software-pipelined (unset: by length); once
static int sw_skinny_pipe() { static const int v = env_int("FFMI_SKINNY_PIPE", -1); return v; }
// FFMI_SKINNY_SPLIT=0: every skinny launch unsplit; once
static bool sw_skinny_split() { static const bool v = env_int("FFMI_SKINNY_SPLIT", 1) != 0; return v; }
// FFMI_SKINNY="NT,KW": tiles and K-split waves of every unsplit plain skinny launch, T <= 32; once
static Pair sw_skinny() { static const Pair v = env_pair("FFMI_SKINNY", 0, 0); return v; }
// FFMI_FZ_KW8=1|2: 8 K-split waves for one-row-tile norm-consumer launches (1 qkv, 2 gate/up too); once
static int sw_fz_kw8() { static const int v = env_int("FFMI_FZ_KW8", 0); return v; }
// FFMI_FZ_NT2=1: fused forms take two tiles per workgroup at one row tile too; once
static bool sw_fz_nt2() { static const bool v = env_int("FFMI_FZ_NT2", 0) != 0; return v; }
// FFMI_WAVE_GEMM=0: no wave form (wide short-K layers keep the K-split form); once
static bool sw_wave_gemm() { static const bool v = env_int("FFMI_WAVE_GEMM", 1) != 0; return v; }
// FFMI_WAVE_FORM="NT,WPG": tiles per wave and waves per workgroup of the wave form (2,4); once
static Pair sw_wave_form() { static const Pair v = env_pair("FFMI_WAVE_FORM", 2, 4); return v; }
// FFMI_MID_MTW4=0: no 4-row-tile waves in the M-split form; load
static const int sw_mid_mtw4 = env_int("FFMI_MID_MTW4", 1) == 0 ? 3 : 4;
// FFMI_MID_NARROW=0: no 2- and 4-tile M-split workgroups; once
static int sw_mid_nopt() { static const int v = env_int("FFMI_MID_NARROW", 1) == 0 ? 4 : 6; return v; }
// FFMI_PREFILL_PLAN=0: the k-step model plans prefill blocks too; once
static bool sw_prefill_plan() { static const bool v = env_int("FFMI_PREFILL_PLAN", 1) != 0; return v; }
// FFMI_MID_ULD=0: no unconditional weight loads in the M-split kernel; once
static bool sw_mid_uld() { static const bool v = env_int("FFMI_MID_ULD", 1) != 0; return v; }
// FFMI_GEMM_STAMP (any value): plain M-split launches take the stamp variant (gemm_debug_stamps); once
static bool sw_gemm_stamp() { static const bool v = getenv("FFMI_GEMM_STAMP") != nullptr; return v; }
// FFMI_GEMM_PLAN="NTW,S" | "N:K:NTW,S;...": M-split tile width and split, of listed shapes only; call
static const char *sw_gemm_plan() { return getenv("FFMI_GEMM_PLAN"); }
// FFMI_TILE_GEMM=0|1|2: the 256 x 256 tile form never / where its grid fills (default) / wherever allowed; call
static int sw_tile_gemm() { return env_int("FFMI_TILE_GEMM", 1); }
// FFMI_MID_XCD=0|1|2: split-K slices renumbered onto XCDs never / from 4 slices (default) / from 2; call
static int sw_mid_xcd() { return env_int("FFMI_MID_XCD", 1); }

// Split-K factor of the skinny path: only narrow layers (few column groups,
// e.g. the 68M SSM's o/down with 48 tiles) and only when the consumer takes
// the partial slabs (no reduce pass); keeps >= 4 k-steps per wave.
static int skinny_split(int T, int N, int K, int epi, bool deferrable) {
  if (!sw_skinny_split() || !deferrable || epi || T > 64) return 1;
  const int ntiles = (N + 15) / 16;
  if (ntiles >= 128) return 1;
  const int KT = K / 32;
  int S = 256 / ntiles;
  S = std::min(S, std::max(1, KT / 8));  // >= 1 k-step per wave of an 8-wave slice
  return std::max(1, std::min(S, 8));
}

// Wide, short-K layers of the skinny range (T <= 64) take gemm_wave_kernel.
// (A split launch never does: skinny_split splits below 128 tiles only.)
static bool wave_form(int ntiles, int KT, int epi, int S) {
  return sw_wave_gemm() && !epi && ntiles >= 1024 && KT <= 32 && S == 1;
}

// Launch plan of the M-split kernel: weight tiles per workgroup (NTW) and
// split-K factor (S).  Each workgroup is bound by its CU's load path (per-wave
// timeline, scripts/diag_stamps.py: a k-step moves NTW KiB of weights + 4*MTW
// KiB of activations at ~50 GB/s per CU; two workgroups on one CU each run at
// half speed), so the plan keeps the grid within one wave of 256 workgroups,
// prefers wide tiles (fewer activation bytes per weight byte) and charges the
// split-K reduce pass.  Times in us; only the ranking matters.
static void mid_plan(GemmPlan &p, int T, int N, int K, int epi, bool deferred) {
  const int mtiles = p.mtiles, KT = p.KT, ntiles = p.ntiles;
  // row tiles per wave: 4 waves x MTW tiles cover one row block; 4 for 13-16
  // tiles (T 193-256: the width-4 verify step, T = 216, in ONE row block
  // instead of two that each re-read every weight tile) and for prefill
  // blocks (fewer row blocks re-reading the weights)
  p.MTW = mtiles <= 8 ? 2 : mtiles <= 12 ? 3 : mtiles <= 16 || mtiles > 24 ? sw_mid_mtw4 : 3;
  p.mblocks = (mtiles + 4 * p.MTW - 1) / (4 * p.MTW);
  double best = 1e30;
  p.NTW = 8, p.S = 1;
  // measured k-step times (us) at MTW = 3, packed activations (diag_stamps.py)
  // (2 and 4: narrow per-rank shards of tensor parallelism, e.g. LLaMA-7B
  // o_proj at TP = 8 is 256 tiles x K = 512 -- 43 workgroups at NTW = 6)
  static const int ntw_opts[6] = {2, 4, 6, 8, 12, 16};
  static const double base[6] = {0.27, 0.30, 0.36, 0.40, 0.65, 0.90};
  for (int o = 6 - sw_mid_nopt(); o < 6; ++o) {
    const int ntw = ntw_opts[o];
    if (p.MTW == 4 && ntw > 8) continue;  // (register budget, see kMidShapes)
    const int nblk = (ntiles + ntw - 1) / ntw;
    for (int S = 1; S <= 8 && S <= KT; ++S) {
      const long wgs = (long)nblk * S * p.mblocks;
      const double rounds = (double)((wgs + 255) / 256);
      const double steps = (double)((KT + S - 1) / S);
      const double tstep = base[o] * (ntw + 4.0 * p.MTW) / (ntw + 12.0);
      double t = rounds * (steps * tstep + 4.0);
      const double slab_mb = (double)S * T * ntiles * 16 * 4 / 1e6;
      // slabs cost their write here and their read in the consumer; a
      // deferred read (norm / attention prologue) is no cheaper than the
      // reduce pass's: /6 had picked 8 slabs for LLaMA-7B o_proj at T = 168,
      // 4 tiles x 4 slabs ran 0.6 % faster end to end (3 of 3 A/B pairs)
      // (the SiLU reduce pass re-reads the gate AND up slabs: at the verify
      // size, 9-12 row tiles in one block, a forced-plan sweep of the TP = 8
      // gate/up shard put 4 tiles x 4-5 slabs at 18.4-18.9 us against 21.7
      // for the 6 x 8 the /3 charge picked, profiles/r06_tp8_gateup_plans.log;
      // the TP 1 / 2 / 4 and 65B TP 8 picks are unchanged by /2)
      const double slab_rate = epi && p.MTW == 3 && p.mblocks == 1 ? 2.0 : 3.0;
      if (S > 1) t += deferred ? slab_mb / 3.0 : 3.0 + slab_mb / slab_rate;
      if (t < best - 1e-9) best = t, p.NTW = ntw, p.S = S;
    }
  }
  // prefill blocks (>= 4 row blocks: T > 576 at MTW = 3): the k-step model
  // above is calibrated at T = 168; forced-plan sweeps at T = 1024
  // (scripts/gpu_prefill_plans.sh, LLaMA-7B shapes) put 8 tiles unsplit
  // first on qkv / o / gate-up / lm_head and 8 tiles x 2 slices on the
  // K = 11008 down projection (gate/up 337 -> 270 us, qkv 149 -> 139,
  // down 148 -> 135, lm_head 428 -> 409); FFMI_PREFILL_PLAN=0 keeps the model
  if (sw_prefill_plan() && p.mblocks >= 4) {
    p.NTW = 8;
    p.S = K >= 8192 && KT >= 2 ? 2 : 1;
    // 4-row-tile waves run one workgroup per CU: only where the grid still
    // covers the CUs (T = 1024: o_proj 128 workgroups -> 3-tile waves, 56 vs
    // 70 us; gate/up, down (2 slices), qkv, lm_head keep 4: 267 vs 280 us,
    // 131 vs 142 us, equal)
    if (p.MTW == 4 && (long)((ntiles + 7) / 8) * p.S * p.mblocks < 256) {
      p.MTW = 3;
      p.mblocks = (mtiles + 11) / 12;
    }
  }
  // diagnostics: FFMI_GEMM_PLAN="NTW,S" forces the tile width and split of
  // every M-split launch; "N:K:NTW,S;..." only of the listed shapes (A/B
  // runs and tests; read per call)
  const char *q = sw_gemm_plan();
  while (q && *q) {
    int a = 0, b = 0, c = 0, d = 0, ntw = 0, S = 0;
    const int n = sscanf(q, "%d:%d:%d,%d", &a, &b, &c, &d);
    if (n == 4 && a == N && b == K) ntw = c, S = d;
    else if (n != 4 && sscanf(q, "%d,%d", &a, &b) == 2) ntw = a, S = b;
    if ((ntw == 2 || ntw == 4 || ntw == 6 || ntw == 8 || ntw == 12 || ntw == 16) && S >= 1 &&
        S <= std::min(KT, 8)) {
      p.NTW = ntw, p.S = S;
      break;
    }
    q = strchr(q, ';');
    if (q) ++q;
  }
  if (p.MTW == 4 && p.NTW > 8) p.NTW = 8;
  p.nblk = (ntiles + p.NTW - 1) / p.NTW;
}

// prefill blocks: the compute-bound 256 x 256 tile form where its grid
// covers the CUs (FFMI_TILE_GEMM: 0 never, 2 whenever the shape allows)
static bool tile_form(const GemmPlan &p, bool xp) {
  if (p.mtiles < 32 || !xp) return false;
  const int mode = sw_tile_gemm();
  const int nbn = (p.ntiles + 15) / 16, nbm = (p.mtiles + 15) / 16;
  // one 256 x 256 tile per CU and round: worth it where the rounds are
  // well filled (T = 1024: qkv 192 tiles 168 -> 140 us, lm_head 500 tiles
  // 396 -> 314, gate/up 344 tiles 274 -> 268; T = 577: gate/up's 258 tiles
  // = one round + 2, 188 -> 221, stays M-split)
  const int nwg = nbn * nbm, rounds = (nwg + 255) / 256;
  return mode == 2 || (mode == 1 && nwg >= 160 && nwg * 10 >= rounds * 256 * 6);
}

// diagnostics: FFMI_SKINNY="NT,KW" forces the tile count and K-split waves
// of every unsplit skinny launch (A/B runs, scripts/gemm_bench.py), also
// where the wave form would run
static bool forced_skinny_tiles(GemmPlan &p) {
  const Pair f = sw_skinny();
  if (f.a <= 0 || p.S != 1 || p.MT > 2 || !listed(kSkinnyForms, SkinnyForm{f.a, f.b, 0, 0}))
    return false;
  p.NT = f.a, p.KW = f.b;
  return true;
}

// Tiles per workgroup and K-split waves of an unfused skinny launch of S
// slices (plain epilogue).
static void skinny_tiles(GemmPlan &p, bool nt) {
  const int ntiles = p.ntiles, KT = p.KT, S = p.S;
  p.NT = 1, p.KW = 4;
  // wide layers (lm_head): two tiles per workgroup once there are >= 2 row
  // tiles (SSM lm_head at T = 24: 16.1 -> 12.3 us warm; at one row tile a
  // single tile stays faster: LLaMA-7B lm_head T = 8 cold 47.8 vs 55.8 us)
  if (p.MT >= 2 && ntiles >= 512) p.NT = 2;
  // 8-wave groups only where the accumulators fit 2 waves/SIMD (no spills)
  else if (ntiles >= 512 || p.MT >= 8) p.KW = 4;
  // ... and where each wave still gets a full batch of U k-steps (K = 768 of
  // the SSM: 4 waves x 6 k-steps beat 8 x 3, qkv T = 24: 5.7 -> 4.2 us).
  // Non-temporal weight loads (FFMI_W_STREAM) keep 4 waves at every row-tile
  // count (LLaMA-7B decode, cold, T = 1-16: o 7.6-8.8 -> 7.2-8.6 us, down
  // 17.0-24.8 -> 16.4-21.9 us over two runs of gemm_bench.py --wstream; T = 32
  // within noise), so a row's reduction order still depends on (N-tile, K,
  // policy) only, not on T: the threshold is a fixed 64 k-steps per slice
  // (8 waves x the largest batch U = 8), never U itself, which depends on T.
  else if ((KT + S - 1) / S >= 64 && !nt) p.KW = 8;
}

// The fused residual/norm forms (FuseArgs; S == 1, T <= 32): the unfused
// path's tile and wave choices, one instantiation set per role.
static void fused_tiles(GemmPlan &p, int ntiles, bool nt) {
  // FFMI_FZ_KW8 (A/B): 8 K-split waves instead of 4 for the one-row-tile
  // consumer launches -- 1: qkv, 2: qkv and gate/up
  const int kw8 = sw_fz_kw8();
  p.NT = 1, p.KW = 4;
  if (p.EPI) p.NT = 2, p.KW = kw8 >= 2 && p.MT == 1 ? 8 : 4;  // (consumer only)
  else if (p.FZ == 2 && kw8 >= 1 && p.MT == 1 && ntiles >= 512) p.KW = 8;
  // FFMI_FZ_NT2=1: two tiles per workgroup at one row tile too (A/B)
  else if ((p.MT >= 2 || sw_fz_nt2()) && ntiles >= 512) p.NT = 2;
  else if (ntiles < 512 && p.KT >= 64 && !nt) p.KW = 8;
}

int reduce_maxs(int S) {
  for (int ms : kReduceMaxS)
    if (S <= ms) return ms;
  return 0;
}

bool plan_instantiated(const GemmPlan &p) {
  if (p.S > 1 && !p.defer && !(listed(kReduceMaxS, p.MAXS) && reduce_instantiated(p.EPI, p.MAXS)))
    return false;
  switch (p.form) {
    case GEMM_SKINNY:
      return listed(kRowTiles, p.MT) && p.MT <= skinny_max_row_tiles(p.FZ) &&
             p.U == skinny_unroll(p.MT) && listed(kSkinnyForms, SkinnyForm{p.NT, p.KW, p.EPI, p.FZ});
    case GEMM_WAVE:
      return listed(kRowTiles, p.MT) && listed(kWaveForms, WaveForm{p.NT, p.WPG});
    case GEMM_MID:
      return listed(kMidShapes, MidShape{p.MTW, p.NTW}) && (p.EPI == 0 || p.EPI == 1);
    case GEMM_TILE:
      return p.EPI == 0 || p.EPI == 1;
  }
  return false;
}

GemmPlan plan_gemm(int T, int N, int K, int epilogue_flags, bool deferrable, int fuse_kind,
                   size_t ws_bytes) {
  GemmPlan p;
  const bool xp = (epilogue_flags & FFMI_X_PACKED) != 0, yp = (epilogue_flags & FFMI_Y_PACKED) != 0;
  const bool nt = (epilogue_flags & FFMI_W_STREAM) != 0;
  const int epi = epilogue_flags & ~(FFMI_X_PACKED | FFMI_Y_PACKED | FFMI_W_STREAM);
  if (T <= 0 || N <= 0 || K <= 0 || (epi != FFMI_EPI_NONE && epi != FFMI_EPI_SILU_MUL)) return p;
  if ((xp && K % 32) || (yp && N % 32)) return p;
  p.EPI = epi;
  p.XP = xp;
  p.KT = K / 32;
  p.mtiles = (T + 15) / 16;
  p.ntiles = (N + 15) / 16 * (epi ? 2 : 1);
  // S slices where the workspace holds their slabs, else un-split (slower)
  auto split = [&](int S) {
    const size_t need = (size_t)S * T * p.ntiles * 16 * sizeof(float);
    p.S = S > 1 && ws_bytes >= need ? S : 1;
    p.slab_bytes = p.S > 1 ? need : 0;
  };
  auto skinny_launch = [&]() {
    p.form = GEMM_SKINNY;
    p.NTL = nt;
    p.grid[0] = (p.ntiles + p.NT - 1) / p.NT, p.grid[1] = p.S;
    p.block = p.KW * 64;
    p.lds = p.KW > 1 ? (size_t)(p.KW - 1) * p.MT * p.NT * 4 * 64 * sizeof(float) : 0;
    // software-pipelined k-loop once every wave has >= 2 full batches (LLaMA-7B
    // decode at T = 8, cold: qkv 21.2 -> 19.5 us, gate/up 39.1 -> 36.8, lm_head
    // 49.5 -> 46.1); short loops (the SSM, K = 768) keep the batched form, which
    // the pipeline slowed (SSM lm_head warm 9.3 -> 12.1 us).
    // FFMI_SKINNY_PIPE=0/1 forces it off/on (A/B runs).
    const int force = sw_skinny_pipe();
    const int per_wave = ((p.KT + p.S - 1) / p.S + p.KW - 1) / p.KW;
    p.PIPE = force >= 0 ? force != 0 : per_wave >= 2 * p.U;
    p.defer = p.S > 1;  // (split only when deferrable)
  };
  if (fuse_kind) {
    // producer: row-major residual out, plain epilogue; consumer: row-major X
    // (the residual), K = the norm width; both unsplit, T <= 32
    if (p.mtiles > 2 || N % 16 || K % 32) return p;
    if (fuse_kind == 1 ? (epi || yp) : fuse_kind != 2 || xp) return p;
    p.FZ = fuse_kind;
    p.MT = p.mtiles, p.U = 8;
    fused_tiles(p, (N + 15) / 16, nt);
    skinny_launch();
  } else if (tile_form(p, xp)) {
    p.form = GEMM_TILE;
    p.nbm = (p.mtiles + 15) / 16;
    p.grid[0] = (p.ntiles + 15) / 16 * p.nbm;
    p.block = 512;
  } else if (p.mtiles > 4) {
    p.form = GEMM_MID;
    mid_plan(p, T, N, K, epi, deferrable && !epi);
    split(p.S);
    p.grid[0] = p.nblk, p.grid[1] = p.S, p.grid[2] = p.mblocks;
    p.block = 256;
    // split-K launches: the workgroups of a k-slice renumbered onto the same
    // XCDs, so that an XCD's L2 fetches only its slices' X columns
    // (mid_xcd_map).  From 4 slices on: with 2 (qkv at T = 168) every XCD still
    // needs half of X and the launch measured no faster.
    // FFMI_MID_XCD: 0 blockIdx numbering, 1 the default, 2 every split launch
    const int xmode = sw_mid_xcd();
    p.xmap = xmode != 0 && p.S >= (xmode == 2 ? 2 : 4);
    p.STAMP = sw_gemm_stamp() && !epi;
    // unconditional weight loads (ULD) whenever NTW % 4 != 0 (gate/up T = 168:
    // 55.9 -> 51.2 us, qkv 37.2 -> 34.6 us in scripts/gemm_bench.py);
    // FFMI_MID_ULD=0 turns them off (A/B runs)
    p.ULD = sw_mid_uld() && p.NTW % 4;
    // non-temporal weight loads only where each weight tile has ONE reader
    // (mblocks == 1); prefill blocks re-read every tile from L2 / the MALL
    p.NTL = nt && p.mblocks == 1;
    p.defer = p.S > 1 && deferrable && !epi;  // the consumer combines the slabs
    p.MAXS = p.S > 1 && !p.defer ? reduce_maxs(p.S) : 0;
  } else {
    p.MT = p.mtiles <= 1 ? 1 : p.mtiles <= 2 ? 2 : 4;
    p.U = skinny_unroll(p.MT);
    split(skinny_split(T, N, K, epi, deferrable));
    if (epi) {
      p.NT = 2, p.KW = 4;  // a (gate, up) tile pair per workgroup
      skinny_launch();
    } else if (forced_skinny_tiles(p)) {
      skinny_launch();
    } else if (wave_form(p.ntiles, p.KT, epi, p.S)) {
      // wide, short-K layers (the SSM lm_head): one wave per 2 tiles over the
      // whole K (gemm_wave_kernel)
      // two tiles per wave: SSM lm_head (32000 x 768) at T = 24 11.1 us (13.3
      // in the K-split form, 13.3 with one tile per wave and twice the waves),
      // T = 8 9.4 us (12.5)
      // (FFMI_WAVE_FORM=NT,WPG: tiles per wave and waves per workgroup, A/B)
      const Pair f = sw_wave_form();
      const bool ok = listed(kWaveForms, WaveForm{f.a, f.b});
      p.form = GEMM_WAVE;
      p.NT = ok ? f.a : 2, p.WPG = ok ? f.b : 4;
      p.NTL = nt;
      p.grid[0] = ((p.ntiles + p.NT - 1) / p.NT + p.WPG - 1) / p.WPG;
      p.block = p.WPG * 64;
    } else {
      skinny_tiles(p, nt);
      skinny_launch();
    }
  }
  p.valid = true;
  return p;
}

size_t gemm_workspace_bytes(int T, int N, int K, int epilogue) {
  epilogue &= ~(FFMI_X_PACKED | FFMI_Y_PACKED | FFMI_W_STREAM);
  return std::max(plan_gemm(T, N, K, epilogue, false, 0, (size_t)-1).slab_bytes,
                  plan_gemm(T, N, K, epilogue, true, 0, (size_t)-1).slab_bytes);
}

void gemm_debug_plan(int T, int N, int K, int epilogue, int *plan) {
  const GemmPlan p = plan_gemm(T, N, K, epilogue & ~(FFMI_Y_PACKED | FFMI_W_STREAM), false, 0, (size_t)-1);
  plan[0] = p.form;
  plan[1] = p.MTW, plan[2] = p.NTW, plan[3] = p.S, plan[4] = p.mblocks, plan[5] = p.nblk;
}

}  // namespace ffmi
