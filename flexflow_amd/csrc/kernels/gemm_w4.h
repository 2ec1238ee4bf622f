// gemm_w4.h -- what the two MXFP4-weight GEMM kernels (gemm_w4.hip: T <= 64,
// gemm_w4_mid.hip: 65 .. 256 rows) share: the launch constants, the exact
// e2m1 -> f16 widening at a block's scale and the e8m0 scale as a float.
#pragma once

#include "gemm_w8.h"  // (u4v, h2w, ld_w8)

namespace ffmi {

constexpr int kW4NT = 2;    // n-tiles per wave (even: a gate tile and its up tile)
constexpr int kW4Ring = 6;  // quad blocks in flight per tile and wave
constexpr int kW4Rows = 64;  // rows per skinny launch
constexpr int kW4MaxS = 8;
constexpr int kW4MinSteps = 2;  // quad steps a k-slice keeps at least
constexpr int kW4Groups = 256;  // workgroups the plan aims for (one per CU)
// the M-split kernel: a workgroup's 4 waves split the rows and share kW4MidNTW
// weight tiles, the column group of a skinny workgroup (same gridDim.x)
constexpr int kW4MidNTW = 4 * kW4NT;
constexpr int kW4MidRows = 256;  // rows per M-split launch (4 waves x 4 m-tiles)
// quad steps in flight per wave, both operands, at MTW m-tiles per wave: a
// slot is 10 + 16 MTW VGPRs, so the ring shortens as the accumulators grow
constexpr int w4_mid_ring(int MTW) { return MTW == 2 ? 4 : MTW == 3 ? 3 : 2; }

// eight e2m1 nibbles of one scale block -> an MFMA f16 fragment, times `scale`
__device__ __forceinline__ h8 w4_widen(uint32_t q, float scale) {
  const h2w p0 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(q, scale, 0);
  const h2w p1 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(q, scale, 1);
  const h2w p2 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(q, scale, 2);
  const h2w p3 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(q, scale, 3);
  return h8{p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], p3[0], p3[1]};
}
// 2^(byte - 127)
__device__ __forceinline__ float e8m0_f32(uint32_t byte) { return __uint_as_float(byte << 23); }

// the M-split launch of rows 65 .. kW4MidRows (gemm_w4_mid.hip); ws: [S][T][NP]
// floats when p.S > 1, summed by the caller
void launch_w4_mid_rows(const W4Plan &p, int MTW, bool silu, bool ntl, const uint16_t *X,
                        const uint8_t *W4, const uint8_t *scales, uint16_t *Y, float *ws, int T,
                        int N, int K, hipStream_t s);

}  // namespace ffmi
