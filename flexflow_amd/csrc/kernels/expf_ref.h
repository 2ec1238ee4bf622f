// expf_ref.h -- the host libm's expf restated for device code, shared by the
// fp16 softmax / top-k (sampling.hip) and the fp32 one (f32.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace ffmi {

// exp(x) for the softmax / top-k terms and probabilities, bit-identical to the
// host libm expf the oracle calls (glibc's double-evaluated algorithm: x /
// ln2 * 32 rounded to k, 2^(k/32) from a 32-entry table, a cubic in the
// remainder, one rounding to float; checked against glibc 2.35 expf on every
// float in [-104, 0], scripts/diag/expf_ref_check.c: 1 difference in 1.1e9,
// at x = -63.1, whose fp16 probability is 0 either way).  The device
// library's expf differs from it by one float ulp on ~1e-4 of inputs, mostly
// near 0 -- where a flat row's terms all lie -- which moved fp16 p values
// across a rounding boundary and reordered tied top-k ids (the fresh-seed
// random-shape sweep of test_softmax_topk_random_shapes_exact), and the
// fp32 top-k's ids on flat rows (test_arg_topk_f32_flat_rows).
// (static: one copy of the table per translation unit that includes this)
static __constant__ unsigned long long kExp2Tab[32] = {
    0x3ff0000000000000ull, 0x3fefd9b0d3158574ull, 0x3fefb5586cf9890full, 0x3fef9301d0125b51ull,
    0x3fef72b83c7d517bull, 0x3fef54873168b9aaull, 0x3fef387a6e756238ull, 0x3fef1e9df51fdee1ull,
    0x3fef06fe0a31b715ull, 0x3feef1a7373aa9cbull, 0x3feedea64c123422ull, 0x3feece086061892dull,
    0x3feebfdad5362a27ull, 0x3feeb42b569d4f82ull, 0x3feeab07dd485429ull, 0x3feea47eb03a5585ull,
    0x3feea09e667f3bcdull, 0x3fee9f75e8ec5f74ull, 0x3feea11473eb0187ull, 0x3feea589994cce13ull,
    0x3feeace5422aa0dbull, 0x3feeb737b0cdc5e5ull, 0x3feec49182a3f090ull, 0x3feed503b23e255dull,
    0x3feee89f995ad3adull, 0x3feeff76f2fb5e47ull, 0x3fef199bdd85529cull, 0x3fef3720dcef9069ull,
    0x3fef5818dcfba487ull, 0x3fef7c97337b9b5full, 0x3fefa4afa2a490daull, 0x3fefd0765b6e4540ull};
__device__ __forceinline__ float expf_ref_core(float x) {
  const double N = 32.0;
  const double InvLn2N = 0x1.71547652b82fep+0 * N, SHIFT = 0x1.8p+52;
  const double C0 = 0x1.c6af84b912394p-5 / N / N / N, C1 = 0x1.ebfce50fac4f3p-3 / N / N,
               C2 = 0x1.62e42ff0c52d6p-1 / N;
  const double z = __dmul_rn(InvLn2N, (double)x);
  double kd = __dadd_rn(z, SHIFT);
  const unsigned long long ki = (unsigned long long)__double_as_longlong(kd);
  kd = __dsub_rn(kd, SHIFT);
  const double r = __dsub_rn(z, kd);
  const double s = __longlong_as_double((long long)(kExp2Tab[ki & 31] + (ki << 47)));
  const double p = __fma_rn(C0, r, C1);
  const double r2 = __dmul_rn(r, r);
  double y = __fma_rn(C2, r, 1.0);
  y = __fma_rn(p, r2, y);
  return (float)__dmul_rn(y, s);
}
// Branch-free (every caller passes x = logit - row max <= 0): the formula runs
// on max(x, -104) and the result is selected, so an unrolled loop of terms
// issues all its table loads ahead of the arithmetic instead of one
// load-and-wait per term behind per-element branches.
__device__ __forceinline__ float expf_ref(float x) {
  const bool in = x > -104.0f;
  const float xr = in ? x : -104.0f;  // (NaN and -inf too: selected away below)
  const float y = expf_ref_core(xr);
  return in ? y : (x == x ? 0.0f : x);  // (underflow to 0; NaN stays NaN)
}

}  // namespace ffmi
