// gemm_plan.h -- the host-side launch plan of the fp16 GEMM (gemm.hip).
//
// plan_gemm() takes every decision of a launch -- form, kernel instantiation,
// grid, split-K factor and workspace need -- from the shape alone; launch_gemm
// issues what the plan says, gemm_workspace_bytes and gemm_debug_plan read it.
// Plain C++17, no HIP: tests/gemm_plan_check.cpp sweeps it on the CPU.
#pragma once
#include <stddef.h>

#include "../../../include/ffmi.h"

namespace ffmi {

// Launch form (what gemm_debug_plan reports as the path).
enum { GEMM_SKINNY = 0, GEMM_WAVE = 1, GEMM_MID = 2, GEMM_TILE = 3 };

// ---- instantiation lists: every kernel the library is built with ----------
// launch_gemm turns a plan's run-time values into template arguments through
// these lists only; a value outside them is an error, never another shape.

// gemm_skinny_kernel<MT, NT, KW, U, EPI, PIPE, NTL, FZ>: row tiles MT (also
// gemm_wave_kernel's) x forms, PIPE and NTL both ways; U follows MT, and the
// fused forms (FZ, T <= 32) exist at one and two row tiles only.
struct SkinnyForm {
  int NT, KW, EPI, FZ;
};
constexpr bool operator==(const SkinnyForm &a, const SkinnyForm &b) {
  return a.NT == b.NT && a.KW == b.KW && a.EPI == b.EPI && a.FZ == b.FZ;
}
constexpr int kRowTiles[] = {1, 2, 4};
constexpr int skinny_unroll(int MT) { return MT == 4 ? 4 : 8; }
constexpr int skinny_max_row_tiles(int FZ) { return FZ ? 2 : 4; }
constexpr SkinnyForm kSkinnyForms[] = {
    {1, 4, 0, 0}, {1, 8, 0, 0}, {2, 4, 0, 0}, {2, 8, 0, 0}, {4, 4, 0, 0}, {4, 2, 0, 0},
    {2, 2, 0, 0}, {2, 4, 1, 0},                              // unfused
    {2, 4, 0, 1}, {1, 8, 0, 1}, {1, 4, 0, 1},                // residual-add producer
    {2, 4, 0, 2}, {1, 8, 0, 2}, {1, 4, 0, 2}, {2, 8, 1, 2}, {2, 4, 1, 2}};  // norm consumer

// gemm_wave_kernel<MT, NT, kWaveUB, NTL, WPG>: kRowTiles x forms x NTL
struct WaveForm {
  int NT, WPG;
};
constexpr bool operator==(const WaveForm &a, const WaveForm &b) {
  return a.NT == b.NT && a.WPG == b.WPG;
}
constexpr WaveForm kWaveForms[] = {{2, 4}, {2, 2}, {3, 2}, {4, 2}, {4, 4}};
constexpr int kWaveUB = 4;

// gemm_mid_kernel<MTW, NTW, kMidPF, EPI, STAMP, XP, ULD, NTL>: shapes x EPI x
// XP x ULD x NTL, and the STAMP variant of EPI 0 (ULD = NTL = false).  No
// 4 x 12 / 4 x 16: that many accumulator tiles exceed the register budget.
struct MidShape {
  int MTW, NTW;
};
constexpr bool operator==(const MidShape &a, const MidShape &b) {
  return a.MTW == b.MTW && a.NTW == b.NTW;
}
constexpr MidShape kMidShapes[] = {{2, 2}, {2, 4}, {2, 6}, {2, 8}, {2, 12}, {2, 16},
                                   {3, 2}, {3, 4}, {3, 6}, {3, 8}, {3, 12}, {3, 16},
                                   {4, 2}, {4, 4}, {4, 6}, {4, 8}};
constexpr int kMidPF = 4;

// gemm_tile_kernel<EPI, kTileNB>: both epilogues
constexpr int kTileNB = 4;

// gemm_reduce_kernel<EPI, MAXS>: 16 with the plain epilogue only (the per-head
// o-projection slabs, launch_partials_reduce)
constexpr int kReduceMaxS[] = {2, 4, 8, 16};
constexpr bool reduce_instantiated(int EPI, int MAXS) { return !(EPI && MAXS == 16); }

template <class V, size_t N>
constexpr bool listed(const V (&list)[N], const V &v) {
  for (size_t i = 0; i < N; ++i)
    if (list[i] == v) return true;
  return false;
}

// ---- the plan ------------------------------------------------------------
struct GemmPlan {
  // false: an argument error (launch_gemm returns hipErrorInvalidValue)
  bool valid = false;
  int form = GEMM_SKINNY;
  // Template arguments of the kernel to instantiate.
  //   skinny: MT, NT, KW, U, EPI, PIPE, NTL, FZ (1 / 2: the fused residual
  //           producer / norm consumer)        wave: MT, NT, WPG, NTL
  //   mid:    MTW, NTW, EPI, STAMP, XP, ULD, NTL      tile: EPI
  // STAMP asks for the diagnostic variant, which has ULD = NTL = false; ULD
  // and NTL describe the plain one (taken when the stamp buffer cannot be had).
  int EPI = 0, MT = 0, NT = 0, KW = 0, U = 0, FZ = 0, WPG = 0, MTW = 0, NTW = 0;
  bool PIPE = false, NTL = false, STAMP = false, XP = false, ULD = false;
  // Launch geometry
  unsigned grid[3] = {1, 1, 1}, block = 0;
  size_t lds = 0;  // dynamic LDS bytes
  // Derived values the kernels take as arguments
  int KT = 0;        // 32-deep k-steps
  int mtiles = 0;    // 16-row tiles
  int ntiles = 0;    // 16-column weight tiles (gate and up tiles both count)
  int S = 1;         // split-K slices, after the workspace clamp
  size_t slab_bytes = 0;  // fp32 slabs S slices need: S * T * ntiles * 16 * 4 (0 unsplit)
  int xmap = 0;             // mid: slices renumbered onto XCDs (mid_xcd_map)
  int mblocks = 0, nblk = 0;  // mid: row blocks and tile blocks of the grid
  int nbm = 0;                // tile: 256-row blocks
  // S > 1: the slabs are left for the consumer (Partials), or summed by
  // gemm_reduce_kernel<EPI, MAXS>
  bool defer = false;
  int MAXS = 0;
};

// The launch of Y[T][N] = X[T][K] . W^T.  epilogue_flags: FFMI_EPI_* with the
// FFMI_X_PACKED / FFMI_Y_PACKED / FFMI_W_STREAM flags; deferrable: the consumer
// can combine split-K slabs; fuse_kind: FuseArgs::kind; ws_bytes: the
// workspace the caller holds (0: none) -- a split that needs more is un-split
// here, and every choice that depends on S follows from the clamped value.
GemmPlan plan_gemm(int T, int N, int K, int epilogue_flags, bool deferrable, int fuse_kind,
                   size_t ws_bytes);
// Every template argument of the plan lies in the lists above.
bool plan_instantiated(const GemmPlan &p);
// MAXS of the reduce pass over S slabs (0: more than any instantiation)
int reduce_maxs(int S);

// Workspace that serves every launch of the shape (no layout flag changes it).
size_t gemm_workspace_bytes(int T, int N, int K, int epilogue);
// diagnostics: {path, MTW, NTW, S, mblocks, nblk} of the launch launch_gemm
// makes for these arguments without a deferred consumer (ffmi_linear); the
// last five describe the M-split grid and are 0, 0, 1, 0, 0 on the other
// paths.  Host only: no launch, no device.
void gemm_debug_plan(int T, int N, int K, int epilogue, int *plan /* [6] */);

}  // namespace ffmi
