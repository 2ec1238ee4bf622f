// gemm_w8.h -- what the two fp8-weight GEMM kernels (gemm_w8.hip: T <= 64,
// gemm_w8_mid.hip: 65 .. 256 rows) share: the launch constants, the 16-byte
// weight load and the exact e4m3 -> f16 widening.
#pragma once

#include "attention_util.h"

namespace ffmi {

constexpr int kW8NT = 2;    // n-tiles per wave (even: a gate tile and its up tile)
constexpr int kW8Ring = 6;  // double blocks in flight per tile and wave
constexpr int kW8Rows = 64;  // rows per skinny launch
constexpr int kW8MaxS = 8;
constexpr int kW8MinSteps = 4;  // double steps a k-slice keeps at least
constexpr int kW8Groups = 256;  // workgroups the plan aims for (one per CU)
// the M-split kernel: a workgroup's 4 waves split the rows and share kW8MidNTW
// weight tiles, the column group of a skinny workgroup (same gridDim.x)
constexpr int kW8MidNTW = 4 * kW8NT;
constexpr int kW8MidRing = 4;    // double steps in flight per wave, both operands
constexpr int kW8MidRows = 256;  // rows per M-split launch (4 waves x 4 m-tiles)

typedef uint32_t u4v __attribute__((ext_vector_type(4)));
typedef _Float16 h2w __attribute__((ext_vector_type(2)));

template <bool NTL>
__device__ __forceinline__ u4v ld_w8(const uint8_t *p) {
  if constexpr (NTL) return __builtin_nontemporal_load(reinterpret_cast<const u4v *>(p));
  else return *reinterpret_cast<const u4v *>(p);
}

// eight e4m3 bytes (a: elements 0-3, b: 4-7) -> an MFMA f16 fragment, exactly
__device__ __forceinline__ h8 w8_widen(uint32_t a, uint32_t b) {
  const h2w p0 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)a, 1.0f, false);
  const h2w p1 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)a, 1.0f, true);
  const h2w p2 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)b, 1.0f, false);
  const h2w p3 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)b, 1.0f, true);
  return h8{p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], p3[0], p3[1]};
}

// the M-split launch of rows 65 .. kW8MidRows (gemm_w8_mid.hip); ws: [S][T][NP]
// floats when p.S > 1, summed by the caller
void launch_w8_mid_rows(const W8Plan &p, int MTW, bool silu, bool ntl, const uint16_t *X,
                        const uint8_t *W8, const float *scales, uint16_t *Y, float *ws, int T,
                        int N, int K, hipStream_t s);

}  // namespace ffmi
