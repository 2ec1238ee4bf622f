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

// W8A8 (gemm_w8a8.hip; the quantising norm of norm.hip): the row quantiser's
// pieces.  X8[t] holds row t's e4m3 bytes of x / a[t], a[t] = absmax / 448 (1
// for an all-zero row); within a 64-column block the 8-column chunk c sits at
// byte 16 (c & 3) + 8 (c >> 2): the weight layout's order, so 16 contiguous
// bytes are a lane's second operands of the two MFMAs of a double step.
constexpr int kA8NTW = kW8MidNTW;  // weight tiles per workgroup: plan_w8's column group
constexpr int kA8Rows = 256;       // rows per launch (4 waves x 4 m-tiles)

// the largest |x| of eight finite fp16 values, as fp16 bits
__device__ __forceinline__ uint32_t a8_absmax8(uint4 v, uint32_t m) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int e = 0; e < 4; ++e) m = max(m, max(w[e] & 0x7fffu, (w[e] >> 16) & 0x7fffu));
  return m;
}
// the workgroup's largest m -> the row scale (scratch: one word per wave)
template <int NW>
__device__ __forceinline__ float a8_row_scale(uint32_t m, uint32_t *scratch) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o));
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = m;
  __syncthreads();
  uint32_t r = scratch[0];
#pragma unroll
  for (int q = 1; q < NW; ++q) r = max(r, scratch[q]);
  return r ? __fdiv_rn(h2f((uint16_t)r), 448.f) : 1.f;
}
// the 8-column chunk ch of row `row` (eight fp16 values) -> its 8 bytes of X8
__device__ __forceinline__ void a8_store8(uint8_t *X8, size_t row, int K, int ch, uint4 v, float a) {
  const uint2 o = make_uint2(kv8_quant_h4(v.x & 0xffff, v.x >> 16, v.y & 0xffff, v.y >> 16, a),
                             kv8_quant_h4(v.z & 0xffff, v.z >> 16, v.w & 0xffff, v.w >> 16, a));
  *reinterpret_cast<uint2 *>(X8 + row * K + (ch >> 3) * 64 + (ch & 3) * 16 + ((ch >> 2) & 1) * 8) = o;
}

// the M-split launch of rows 65 .. kW8MidRows (gemm_w8_mid.hip); ws: [S][T][NP]
// floats when p.S > 1, summed by the caller
void launch_w8_mid_rows(const W8Plan &p, int MTW, bool silu, bool ntl, const uint16_t *X,
                        const uint8_t *W8, const float *scales, uint16_t *Y, float *ws, int T,
                        int N, int K, hipStream_t s);

}  // namespace ffmi
