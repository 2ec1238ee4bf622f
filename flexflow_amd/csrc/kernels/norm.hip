// norm.hip -- RMSNorm / ResidualRMSNorm, embedding, SiLU-mul, softmax+argmax/topk.
//
// HBM-bound row kernels: one 256-thread workgroup per row, 16-B vector
// loads/stores (8 halves per lane), the row kept in registers between the
// reduction and the scale pass (one read + one write per element).  Unlike
// the reference (which launches every buffer row, rms_norm_kernels.cu:133-134)
// only the T active rows are processed.
#include <algorithm>

#include "../ffmi_internal.h"
#include "expf_ref.h"

namespace ffmi {

__device__ __forceinline__ float h2f_(uint16_t v) { return __half2float(__ushort_as_half(v)); }
__device__ __forceinline__ uint16_t f2h_(float v) { return __half_as_ushort(__float2half_rn(v)); }

template <int NW, typename T>
__device__ __forceinline__ T block_sum(T v, T *scratch) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) scratch[wave] = v;
  __syncthreads();
  T r = scratch[0];
#pragma unroll
  for (int q = 1; q < NW; ++q) r += scratch[q];
  return r;
}

// rms_norm_kernels.cu:97-124 / residual_rms_norm_kernels.cu:98-131:
//   r = x1 (+ x2, rounded to half); rms = half(rsqrt(mean(r^2) + eps));
//   y = half(r * rms); out = half(y * w)
// One workgroup of NT threads per row, MAXC 8-element chunks per thread; every
// load of the row (x1, x2 or its split-K slabs, and w) is issued before the
// reduction, so a row costs one memory round trip.
// SRC (compile time, so that the loads are straight-line code: behind
// runtime branches the compiler reused a loaded register as the slab address
// and waited for the x1 load before issuing the slabs -- two round trips):
//   0: x1 only   1: x1 + x2 (fp16)   2: x1 + split-K slabs   3: gather (x1 =
//   embedding table, rows picked by the step's token ids)
//   4 / 5: 1 / 2 with the FFMI_FAULT_RESID_ROUND negative control (tests
//   only): the sum of squares takes the UNROUNDED fp32 residual sum, where
//   residual_rms_norm_kernels.cu:112-114 squares the half-rounded one
template <int NT, int MAXC, int MAXS, int SRC>
__global__ __launch_bounds__(NT) void rmsnorm_kernel(
    const uint16_t *__restrict__ x1, const uint16_t *__restrict__ x2,
    const uint16_t *__restrict__ w, uint16_t *__restrict__ res_out,
    uint16_t *__restrict__ out, int H, float eps, int out_packed,
    const float *__restrict__ x2p, int pS, int pNP, const char *__restrict__ gather,
    uint4 *__restrict__ blob_dst, int blob_n16, const int32_t *__restrict__ gprev) {
  __shared__ double scratch[NT / 64];
  const int row = blockIdx.x;
  const int T = gridDim.x;
  const int nchunk = H >> 3;
  // gather: x1 is the embedding table and row t reads its token's row (the
  // embedding lookup fused into the first layer's norm; res_out gets the copy)
  constexpr bool FAULT = SRC >= 4;
  constexpr int S = FAULT ? SRC - 3 : SRC;  // the data source of the variant
  // (a chained SSM beam step: token id -1 - i is entry i of the previous
  // step's top-k ids, gprev, which the host could not know when it staged
  // this step; ffmi_model beam_launch_chained)
  int gid = 0;
  if (S == 3) {
    gid = batch_view(gather).tokens[row].token_id;
    if (gid < 0) gid = gprev[-1 - gid];
  }
  const uint16_t *a = S == 3 ? x1 + (size_t)gid * H : x1 + (size_t)row * H;
  // blob fetch: gather is the step's staging blob in mapped host memory; the
  // grid copies it into device memory for the step's later kernels (replaces
  // the H2D copy node and the system-scope boundary after it), its loads in
  // flight together with the token-id read
  if (S == 3 && blob_dst) {
    const uint4 *src = reinterpret_cast<const uint4 *>(gather);
    for (int i = row * NT + threadIdx.x; i < blob_n16; i += T * NT) blob_dst[i] = src[i];
  }
  uint4 v[MAXC], wv[MAXC];
  // every load of the row first (slabs, x2, x1, w), then the arithmetic;
  // x2 = the deferred split-K slabs of the producing GEMM summed in order,
  // folded per chunk when a thread holds several chunks (register budget)
  uint4 xb[MAXC];
  f4 slo[MAXS], shi[MAXS];
  auto fold = [&]() {
    f4 lo = slo[0], hi = shi[0];
#pragma unroll
    for (int sl = 1; sl < MAXS; ++sl)
      if (sl < pS) lo += slo[sl], hi += shi[sl];
    uint16_t hb[8];
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
      hb[q4] = f2h_(lo[q4]);
      hb[q4 + 4] = f2h_(hi[q4]);
    }
    return *reinterpret_cast<uint4 *>(hb);
  };
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    const int ch = min((int)threadIdx.x + c * NT, nchunk - 1);  // clamped: no branch
    if (S == 2) {
      const float *q = x2p + (size_t)row * pNP + ch * 8;
#pragma unroll
      for (int sl = 0; sl < MAXS; ++sl) {
        const float *qs = q + (size_t)min(sl, pS - 1) * T * pNP;
        slo[sl] = *reinterpret_cast<const f4 *>(qs);
        shi[sl] = *reinterpret_cast<const f4 *>(qs + 4);
      }
    }
    if (S == 1) xb[c] = *reinterpret_cast<const uint4 *>(x2 + (size_t)row * H + ch * 8);
    v[c] = *reinterpret_cast<const uint4 *>(a + ch * 8);
    wv[c] = *reinterpret_cast<const uint4 *>(w + ch * 8);
    if (S == 2 && MAXC > 1) xb[c] = fold();
  }
  if (S == 2 && MAXC == 1) xb[0] = fold();
  // the sum of squares in fp64, as the oracle's (exact products, then one
  // rounding to float): an fp32 sum in another order than the oracle's moved
  // rms across a half rounding boundary in ~1 row in 10^3 at H = 16160
  // (test_rmsnorm_random_shapes sweep), where every output of the row shifts
  double ss = 0.0;
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    const int ch = threadIdx.x + c * NT;
    if (ch < nchunk) {
      uint4 xa = v[c];
      if (S == 1 || S == 2) {
        const uint4 xbb = xb[c];
        const __half2 *pa = reinterpret_cast<const __half2 *>(&xa);
        const __half2 *pb = reinterpret_cast<const __half2 *>(&xbb);
        if (FAULT) {  // negative control: square the unrounded sum
          const uint16_t *ea = reinterpret_cast<const uint16_t *>(&xa);
          const uint16_t *eb = reinterpret_cast<const uint16_t *>(&xbb);
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            const float f = h2f_(ea[q]) + h2f_(eb[q]);
            ss += (double)f * (double)f;
          }
        }
        __half2 r[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) r[q] = __hadd2(pa[q], pb[q]);  // correctly rounded
        xa = *reinterpret_cast<uint4 *>(r);
        *reinterpret_cast<uint4 *>(res_out + (size_t)row * H + ch * 8) = xa;
      } else if (S == 3) {
        *reinterpret_cast<uint4 *>(res_out + (size_t)row * H + ch * 8) = xa;
      }
      v[c] = xa;
      const uint16_t *e = reinterpret_cast<const uint16_t *>(&xa);
      if (!FAULT) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const float f = h2f_(e[q]);
          ss += (double)f * (double)f;
        }
      }
    }
  }
  const float sum = (float)block_sum<NT / 64>(ss, scratch);
  // sqrtf: the correctly rounded square root (HIP's __fsqrt_rn is the native
  // v_sqrt_f32, ~1 ulp, unless OCML_BASIC_ROUNDED_OPERATIONS is defined)
  const float rms_f = __fdiv_rn(1.0f, sqrtf(__fadd_rn(__fdiv_rn(sum, (float)H), eps)));
  const float rms = h2f_(f2h_(rms_f));
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    const int ch = threadIdx.x + c * NT;
    if (ch < nchunk) {
      const uint16_t *e = reinterpret_cast<const uint16_t *>(&v[c]);
      const uint16_t *we = reinterpret_cast<const uint16_t *>(&wv[c]);
      uint16_t o8[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        float y = h2f_(f2h_(__fmul_rn(h2f_(e[q]), rms)));
        o8[q] = f2h_(__fmul_rn(y, h2f_(we[q])));
      }
      uint16_t *dst = out_packed ? out + act_packed_off(row, ch * 8, H) : out + (size_t)row * H + ch * 8;
      *reinterpret_cast<uint4 *>(dst) = *reinterpret_cast<uint4 *>(o8);
    }
  }
}

// FFMI_FAULT_RESID_ROUND (tests only, process-wide): residual norms take the
// faulted variants (SRC 4 / 5)
static bool g_norm_fault = false;
void set_norm_fault(bool on) { g_norm_fault = on; }

hipError_t launch_rmsnorm(const uint16_t *x1, const uint16_t *x2, const uint16_t *w,
                          uint16_t *res_out, uint16_t *out, int T, int H, float eps,
                          hipStream_t s, bool out_packed, Partials x2p, const char *gather,
                          char *blob_dst, size_t blob_bytes, const int32_t *gather_prev) {
  if (gather && (x2 || x2p.S > 0 || !res_out)) return hipErrorInvalidValue;
  if (blob_dst && (!gather || blob_bytes > (size_t)1 << 30 || (uintptr_t)gather % 16 ||
                   (uintptr_t)blob_dst % 16))
    return hipErrorInvalidValue;
  // whole 16-byte chunks: the staging and device blobs are 16-aligned and
  // padded (ffmi_batch_create), so the rounded-up tail stays inside both
  const int blob_n16 = blob_dst ? (int)((blob_bytes + 15) / 16) : 0;
  if (T <= 0) return hipSuccess;
  if (out_packed && H % 32) return hipErrorInvalidValue;
  const int op = out_packed ? 1 : 0;
  const int nchunk = H / 8;
  if (nchunk > 4096) return hipErrorInvalidValue;
  const float *pp = x2p.S > 0 ? x2p.p : nullptr;
  // > 8 slabs: the per-head o-projection slabs of a small model (OprojArgs,
  // <= 16 heads, H <= 1024)
  if (pp && (x2p.S > 16 || (x2p.S > 8 && nchunk > 128))) return hipErrorInvalidValue;
  if ((x2 || pp) && !res_out) return hipErrorInvalidValue;
  // split-K slabs: one 8-column chunk per thread (H <= 8192); the model does
  // not defer its o/down partials beyond that
  if (pp && nchunk > 1024) return hipErrorInvalidValue;
  const int src = gather ? 3 : pp ? 2 : x2 ? 1 : 0;
  const int ms = !pp || x2p.S <= 1 ? 1 : x2p.S <= 2 ? 2 : x2p.S <= 4 ? 4 : x2p.S <= 8 ? 8
               : x2p.S <= 12 ? 12 : 16;
#define FFMI_RMS3(NT, MC, MS, SR)                                                              \
  hipLaunchKernelGGL((rmsnorm_kernel<NT, MC, MS, SR>), dim3(T), dim3(NT), 0, s, x1, x2, w,    \
                     res_out, out, H, eps, op, pp, x2p.S, x2p.NP, gather,               \
                     reinterpret_cast<uint4 *>(blob_dst), blob_n16, gather_prev)
#define FFMI_RMS(NT, MC)                                   \
  do {                                                     \
    if (src == 0) FFMI_RMS3(NT, MC, 1, 0);                 \
    else if (src == 1) FFMI_RMS3(NT, MC, 1, 1);            \
    else if (src == 3) FFMI_RMS3(NT, MC, 1, 3);            \
    else if (ms == 1) FFMI_RMS3(NT, MC, 1, 2);             \
    else if (ms == 2) FFMI_RMS3(NT, MC, 2, 2);             \
    else if (ms == 4) FFMI_RMS3(NT, MC, 4, 2);             \
    else FFMI_RMS3(NT, MC, 8, 2);                          \
  } while (0)
#define FFMI_RMS_NOSLAB(NT, MC)                            \
  do {                                                     \
    if (src == 0) FFMI_RMS3(NT, MC, 1, 0);                 \
    else if (src == 1) FFMI_RMS3(NT, MC, 1, 1);            \
    else FFMI_RMS3(NT, MC, 1, 3);                          \
  } while (0)
  if (g_norm_fault && (src == 1 || src == 2)) {  // negative control (tests only)
#define FFMI_RMSF(NT)                                      \
  do {                                                     \
    if (src == 1) FFMI_RMS3(NT, 1, 1, 4);                  \
    else if (ms == 1) FFMI_RMS3(NT, 1, 1, 5);              \
    else if (ms == 2) FFMI_RMS3(NT, 1, 2, 5);              \
    else if (ms == 4) FFMI_RMS3(NT, 1, 4, 5);              \
    else if (ms == 8) FFMI_RMS3(NT, 1, 8, 5);              \
    else return hipErrorInvalidValue;                      \
  } while (0)
    if (nchunk <= 128) FFMI_RMSF(128);
    else if (nchunk <= 256) FFMI_RMSF(256);
    else if (nchunk <= 512) FFMI_RMSF(512);
    else if (nchunk <= 1024) FFMI_RMSF(1024);
    else return hipErrorInvalidValue;
#undef FFMI_RMSF
    return hipGetLastError();
  }
  if (nchunk <= 128 && ms == 12) FFMI_RMS3(128, 1, 12, 2);
  else if (nchunk <= 128 && ms == 16) FFMI_RMS3(128, 1, 16, 2);
  else if (nchunk <= 128) FFMI_RMS(128, 1);
  else if (nchunk <= 256) FFMI_RMS(256, 1);
  else if (nchunk <= 512) FFMI_RMS(512, 1);
  else if (nchunk <= 1024) FFMI_RMS(1024, 1);
  else if (nchunk <= 2048) FFMI_RMS_NOSLAB(1024, 2);
  else FFMI_RMS_NOSLAB(1024, 4);
#undef FFMI_RMS_NOSLAB
#undef FFMI_RMS
#undef FFMI_RMS3
  return hipGetLastError();
}

// embed_forward_no_aggr (embedding_kernels.cu:233-244)
__global__ void embedding_kernel(const char *__restrict__ blob,
                                 const uint16_t *__restrict__ table,
                                 uint16_t *__restrict__ out, int H) {
  const BatchView bv = batch_view(blob);
  const int t = blockIdx.x;
  const int tok = bv.tokens[t].token_id;
  const uint4 *src = reinterpret_cast<const uint4 *>(table + (size_t)tok * H);
  uint4 *dst = reinterpret_cast<uint4 *>(out + (size_t)t * H);
  for (int c = threadIdx.x; c < H / 8; c += blockDim.x) dst[c] = src[c];
}

hipError_t launch_embedding(const char *blob, int T, const uint16_t *table, uint16_t *out,
                            int H, hipStream_t s) {
  if (T <= 0) return hipSuccess;
  if (H % 8 != 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(embedding_kernel, dim3(T), dim3(256), 0, s, blob, table, out, H);
  return hipGetLastError();
}

// SigmoidSiluMultiKernel (sigmoid_silu_multi.cu:37-47)
__global__ void silu_mul_kernel(const uint16_t *__restrict__ a, const uint16_t *__restrict__ b,
                                uint16_t *__restrict__ out, size_t n) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n;
       i += (size_t)gridDim.x * blockDim.x) {
    const float g = h2f_(a[i]);
    const float sg = __fdiv_rn(1.0f, __fadd_rn(1.0f, expf(-g)));
    const float t = h2f_(f2h_(__fmul_rn(g, h2f_(f2h_(sg)))));
    out[i] = f2h_(__fmul_rn(t, h2f_(b[i])));
  }
}

hipError_t launch_silu_mul(const uint16_t *a, const uint16_t *b, uint16_t *out, size_t n,
                           hipStream_t s) {
  if (n == 0) return hipSuccess;
  size_t blocks = (n + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  hipLaunchKernelGGL(silu_mul_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a, b, out, n);
  return hipGetLastError();
}

// Wave-wide reductions on DPP / permlane (device library), not LDS
// bpermute shuffles: the result is uniform across the wave.
extern "C" __device__ float __ockl_wfred_max_f32(float);
extern "C" __device__ double __ockl_wfred_add_f64(double);
extern "C" __device__ unsigned long long __ockl_wfred_max_u64(unsigned long long);

// softmax (fp16 output, softmax.cu:262-288) + ArgMax (argmax.cu:62-100) /
// ArgTopK (arg_topk.cu:339-448), register-resident: one TPB-thread workgroup
// per row reads the row ONCE as 16-B vectors (NV per thread) and keeps it in
// registers.  p_i = half(exp(x_i - max) / S); the pick is the lowest index of
// the largest p_i (ties created by the fp16 rounding resolve exactly as cub
// ArgMax / the top-k heap do).
//  * S = float(sum of exp(x_i - M) accumulated in double): the oracle's
//    float(double sum), whatever the summation order.
//  * p_i is computed only for CANDIDATES: p is non-decreasing in x, and the
//    k-th largest of the per-wave maxima, L, is <= the row's k-th largest
//    logit, so every member of the top-k (ties included) has fp16 p >= p(L),
//    i.e. an unrounded p_i above the lower rounding boundary of p(L): x_i >=
//    M + log(boundary * S).  That threshold (lowered by a margin that covers
//    the float error of exp/div/log) excludes all but a handful of logits, and
//    the 32000 exp + correctly rounded divisions of a full p pass go away.
//  * The candidates' (p desc, idx asc) keys go to an LDS list; one wave picks
//    the k best (k wave reductions, no workgroup barrier).  More than kCand
//    candidates (flat rows, planted ties) fall back to k rounds of a
//    workgroup-wide selection over the registers.
//  * G > 1 (few rows: the SSM's beam steps, decode): G workgroups per row
//    (grid G x T), each loading the whole row (max and wave maxima identical
//    in all of them) but summing the exp terms of only 1/G of every thread's
//    elements: the double-precision expf_ref terms are the kernel's cost, and
//    T = 24 rows kept them on 24 CUs.  Each workgroup publishes its partial
//    sum (one lane: agent-scope store, drained, then an agent-scope add on
//    the row's counter); the workgroup whose add comes last reads the G
//    partials by atomic reads, sums them in chunk order, resets the counter
//    and finishes the row from its registers.  No workgroup waits for
//    another.  The double sum is split differently than at G = 1 (and than
//    the oracle's serial loop): S = float(double sum) in any order, as above.
//    `part` = [T][G] doubles, `cnt` = [T] counters, zero before the first
//    launch and left zero.
template <int TPB, int NV, int G>
__global__ __launch_bounds__(TPB) void softmax_topk_reg_kernel(
    const uint16_t *__restrict__ logits, int V, int k, int32_t *__restrict__ ids,
    float *__restrict__ probs, double *__restrict__ part, unsigned *__restrict__ cnt,
    int32_t *__restrict__ ids2) {
  constexpr int NW = TPB / 64;
  constexpr int kCand = 128;
  static_assert(G == 1 || ((NV * 8) % G == 0 && NV * 8 / G >= 2),
                "split: whole dwords of a thread's elements per workgroup");
  constexpr int E = NV * 8 / G;  // elements of each thread's row part this workgroup sums
  // wave maxima / sums / selection keys, and the candidate list
  __shared__ double sh[NW + 2];
  __shared__ unsigned long long cand[kCand];
  __shared__ unsigned ncand;
  __shared__ int last_arrival;
  float *fsh = reinterpret_cast<float *>(sh);
  unsigned long long *ksh = reinterpret_cast<unsigned long long *>(sh);
  const int row = G == 1 ? blockIdx.x : blockIdx.y, chunk = G == 1 ? 0 : blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int nvec = V >> 3;
  const uint4 *x = reinterpret_cast<const uint4 *>(logits + (size_t)row * V);
  // split form: workgroup `chunk` loads the row's vectors rotated so that the
  // elements it sums are always its first E (compile-time register indices):
  // local vector v holds row vector gv(v); E < 8: a runtime half / quarter of
  // local vector 0, at element eo
  constexpr int EPV = E < 8 ? 8 / E : 1;  // workgroups sharing one vector
  const int vrot = G == 1 ? 0 : (E >= 8 ? chunk * (E / 8) : chunk / EPV);
  const int eo = E >= 8 ? 0 : (chunk % EPV) * E;
  auto gv = [&](int v) -> int { return (G == 1 ? v : (v + vrot) % NV) * TPB + tid; };
  uint4 r[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int i = gv(v);
    r[v] = i < nvec ? x[i] : make_uint4(0xfc00fc00u, 0xfc00fc00u, 0xfc00fc00u, 0xfc00fc00u);
  }
  if (tid == 0) ncand = 0;
  auto elem = [&](int v, int e) -> float {
    const uint32_t w = (&r[v].x)[e >> 1];
    return h2f_((uint16_t)((e & 1) ? (w >> 16) : (w & 0xffffu)));
  };
  float mx = -INFINITY;
#pragma unroll
  for (int v = 0; v < NV; ++v)
#pragma unroll
    for (int e = 0; e < 8; ++e) mx = fmaxf(mx, elem(v, e));
  mx = __ockl_wfred_max_f32(mx);
  if (lane == 0) fsh[wv] = mx;
  __syncthreads();
  float wmax[NW];
#pragma unroll
  for (int q = 0; q < NW; ++q) wmax[q] = fsh[q];
  __syncthreads();
  float M = wmax[0];
#pragma unroll
  for (int q = 1; q < NW; ++q) M = fmaxf(M, wmax[q]);
  // L = k-th largest wave maximum (k <= 4 <= NW): a lower bound of the k-th
  // largest logit
  float L = -INFINITY;
  {
    float top[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int q = 0; q < NW; ++q) {
      float v = wmax[q];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float hi = fmaxf(top[j], v), lo = fminf(top[j], v);
        top[j] = hi, v = lo;
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j == k - 1) L = top[j];
  }
  // the sum's terms use the oracle's expf (expf_ref), as the p values do:
  // with the hardware exp2 (__expf, a few ulp) a peaked row, whose S a few
  // terms dominate, took their errors straight into S's float rounding, and
  // 1 p in ~10^4 came out one fp16 ulp off (the random-shape sweep of
  // test_softmax_topk_random_shapes_exact)
  double se = 0.0;
  if constexpr (E >= 8) {
#pragma unroll
    for (int v = 0; v < E / 8; ++v)
      if (gv(v) < nvec)
#pragma unroll
        for (int e = 0; e < 8; ++e) se += (double)expf_ref(elem(v, e) - M);
  } else {
    // dwords eo/2 .. eo/2 + E/2 - 1 of local vector 0 (selects, no indexing)
    const int d0 = eo >> 1;
    auto dw = [&](int d) -> uint32_t {  // selects (a runtime array index would go to scratch)
      const uint32_t lo = (d & 1) ? r[0].y : r[0].x, hi = (d & 1) ? r[0].w : r[0].z;
      return (d & 2) ? hi : lo;
    };
    if (gv(0) < nvec)
#pragma unroll
      for (int q = 0; q < E / 2; ++q) {
        const uint32_t w = dw(d0 + q);
        se += (double)expf_ref(h2f_((uint16_t)(w & 0xffffu)) - M);
        se += (double)expf_ref(h2f_((uint16_t)(w >> 16)) - M);
      }
  }
  se = __ockl_wfred_add_f64(se);
  if (lane == 0) sh[wv] = se;
  __syncthreads();
  double sd = 0.0;
#pragma unroll
  for (int q = 0; q < NW; ++q) sd += sh[q];
  if constexpr (G > 1) {
    // (the guide's single-counter hand-off: agent-scope store of the bytes,
    // drained, then the add; the last adder reads them with agent-scope
    // loads after its add returned -- one load per lane, all in flight)
    if (wv == 0) {
      unsigned before = 0;
      if (lane == 0) {
        __hip_atomic_store(&part[(size_t)row * G + chunk], sd, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        before = __hip_atomic_fetch_add(&cnt[row], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      const int last = __shfl(before, 0) == (unsigned)(G - 1);
      if (last) {
        double pq = 0.0;
        if (lane < G)
          pq = __hip_atomic_load(&part[(size_t)row * G + lane], __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_AGENT);
        double tot = 0.0;
#pragma unroll
        for (int q = 0; q < G; ++q) tot += __shfl(pq, q);  // chunk order
        if (lane == 0) {
          __hip_atomic_store(&cnt[row], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          sh[NW] = tot;
        }
      }
      if (lane == 0) last_arrival = last;
    }
    __syncthreads();
    if (!last_arrival) return;
    sd = sh[NW];
  }
  const float S = (float)sd;
  // candidate threshold from p(L): its lower fp16 rounding boundary, minus a
  // margin of 2^-10 in x (>> the float error of exp, the division and log)
  // (finite: logits set to -inf -- taken ones -- are never candidates)
  float thr = -3.402823466e38f;
  {
    const uint16_t pL = f2h_(__fdiv_rn(expf_ref(L - M), S));
    if (pL > 1) {
      const float lo = 0.5f * (h2f_(pL) + h2f_((uint16_t)(pL - 1)));
      thr = M + logf(lo * S) - 0.0009765625f * fmaxf(1.0f, fabsf(M));
    }
  }
  // keys: (p + 1) << 32 | ~idx, 0 = not a candidate / taken
  auto key_of = [&](float xv, unsigned i) -> unsigned long long {
    const uint16_t p = f2h_(__fdiv_rn(expf_ref(xv - M), S));
    return ((unsigned long long)(p + 1u) << 32) | (unsigned long long)(0xffffffffu - i);
  };
  auto emit = [&](int rd, unsigned long long b) {
    ids[(size_t)row * k + rd] = (int)(0xffffffffu - (unsigned)(b & 0xffffffffu));
    if (ids2) ids2[(size_t)row * k + rd] = (int)(0xffffffffu - (unsigned)(b & 0xffffffffu));
    if (probs) probs[(size_t)row * k + rd] = h2f_((uint16_t)((b >> 32) - 1u));
  };
#pragma unroll
  for (int v = 0; v < NV; ++v)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float xv = elem(v, e);
      const unsigned i = (unsigned)(gv(v) * 8 + e);
      if (xv >= thr && (int)i < V) {
        const unsigned slot = atomicAdd(&ncand, 1u);
        if (slot < (unsigned)kCand) cand[slot] = key_of(xv, i);
      }
    }
  __syncthreads();
  const unsigned n = ncand;
  if (n <= (unsigned)kCand) {
    if (wv == 0) {  // keys are distinct (they hold the index)
      unsigned long long a = (unsigned)lane < n ? cand[lane] : 0ull;
      unsigned long long b = (unsigned)(lane + 64) < n ? cand[lane + 64] : 0ull;
      for (int rd = 0; rd < k; ++rd) {
        const unsigned long long best = __ockl_wfred_max_u64(a > b ? a : b);
        if (lane == 0) emit(rd, best);
        if (a == best) a = 0ull;
        if (b == best) b = 0ull;
      }
    }
    return;
  }
  // many candidates: k rounds of a workgroup-wide selection
  for (int rd = 0; rd < k; ++rd) {
    unsigned long long best = 0;
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float xv = elem(v, e);
        const unsigned i = (unsigned)(gv(v) * 8 + e);
        if (xv >= thr && (int)i < V) {
          const unsigned long long key = key_of(xv, i);
          best = key > best ? key : best;
        }
      }
    best = __ockl_wfred_max_u64(best);
    if (lane == 0) ksh[wv] = best;
    __syncthreads();
    unsigned long long b = ksh[0];
#pragma unroll
    for (int q = 1; q < NW; ++q) b = ksh[q] > b ? ksh[q] : b;
    __syncthreads();
    const unsigned idx = 0xffffffffu - (unsigned)(b & 0xffffffffu);
    if (tid == 0) emit(rd, b);
    if (rd + 1 < k && (idx >> 3) % TPB == (unsigned)tid) {  // owner marks it taken (-inf)
#pragma unroll
      for (int v = 0; v < NV; ++v)
        if ((unsigned)gv(v) == (idx >> 3)) {
          // (compile-time register indices only: a runtime-indexed store
          // into the row's registers would put it in scratch)
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            uint32_t &w = (&r[v].x)[e >> 1];
            const uint32_t m = (e & 1) ? 0xffff0000u : 0x0000ffffu;
            if ((unsigned)e == (idx & 7)) w = (w & ~m) | (0xfc00fc00u & m);
          }
        }
    }
  }
}

// softmax (fp16 output, softmax.cu:262-288) + ArgMax (argmax.cu:62-100) /
// ArgTopK (arg_topk.cu:339-448) for rows the register kernel does not take
// (a vocabulary not a multiple of 8, unaligned rows, V > 32768 such as
// LLaMA-3's 128256): the same rule -- p_i = half(exp(x_i - max) / S), S =
// float(double sum), (p desc, index asc) -- in three strided passes over the
// row (max and wave maxima, sum, candidates; the second and third hit L2),
// the candidate threshold and LDS list of softmax_topk_reg_kernel below, and
// k workgroup-wide rounds over the row only when more than kCand logits are
// candidates.
template <int TPB>
__global__ __launch_bounds__(TPB) void softmax_topk_kernel(
    const uint16_t *__restrict__ logits, int V, int k, int32_t *__restrict__ ids,
    float *__restrict__ probs, int32_t *__restrict__ ids2) {
  constexpr int NW = TPB / 64;
  constexpr int kCand = 128;
  __shared__ double sh[NW + 2];
  __shared__ unsigned long long cand[kCand];
  __shared__ unsigned ncand;
  float *fsh = reinterpret_cast<float *>(sh);
  unsigned long long *ksh = reinterpret_cast<unsigned long long *>(sh);
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint16_t *x = logits + (size_t)row * V;
  if (tid == 0) ncand = 0;
  float mx = -INFINITY;
  for (int i = tid; i < V; i += TPB) mx = fmaxf(mx, h2f_(x[i]));
  mx = __ockl_wfred_max_f32(mx);
  if (lane == 0) fsh[wv] = mx;
  __syncthreads();
  float wmax[NW];
#pragma unroll
  for (int q = 0; q < NW; ++q) wmax[q] = fsh[q];
  __syncthreads();
  float M = wmax[0];
#pragma unroll
  for (int q = 1; q < NW; ++q) M = fmaxf(M, wmax[q]);
  // L = k-th largest wave maximum: the waves' index sets are disjoint, so it
  // is a lower bound of the row's k-th largest logit
  float L = -INFINITY;
  {
    float top[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int q = 0; q < NW; ++q) {
      float v = wmax[q];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float hi = fmaxf(top[j], v), lo = fminf(top[j], v);
        top[j] = hi, v = lo;
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j == k - 1) L = top[j];
  }
  double se = 0.0;
  for (int i = tid; i < V; i += TPB) se += (double)expf_ref(h2f_(x[i]) - M);
  se = __ockl_wfred_add_f64(se);
  if (lane == 0) sh[wv] = se;
  __syncthreads();
  double sd = 0.0;
#pragma unroll
  for (int q = 0; q < NW; ++q) sd += sh[q];
  const float S = (float)sd;
  float thr = -3.402823466e38f;
  {
    const uint16_t pL = f2h_(__fdiv_rn(expf_ref(L - M), S));
    if (pL > 1) {
      const float lo = 0.5f * (h2f_(pL) + h2f_((uint16_t)(pL - 1)));
      thr = M + logf(lo * S) - 0.0009765625f * fmaxf(1.0f, fabsf(M));
    }
  }
  auto key_of = [&](float xv, unsigned i) -> unsigned long long {
    const uint16_t p = f2h_(__fdiv_rn(expf_ref(xv - M), S));
    return ((unsigned long long)(p + 1u) << 32) | (unsigned long long)(0xffffffffu - i);
  };
  auto emit = [&](int rd, unsigned long long b) {
    ids[(size_t)row * k + rd] = (int)(0xffffffffu - (unsigned)(b & 0xffffffffu));
    if (ids2) ids2[(size_t)row * k + rd] = (int)(0xffffffffu - (unsigned)(b & 0xffffffffu));
    if (probs) probs[(size_t)row * k + rd] = h2f_((uint16_t)((b >> 32) - 1u));
  };
  for (int i = tid; i < V; i += TPB) {
    const float xv = h2f_(x[i]);
    if (xv >= thr) {
      const unsigned slot = atomicAdd(&ncand, 1u);
      if (slot < (unsigned)kCand) cand[slot] = key_of(xv, (unsigned)i);
    }
  }
  __syncthreads();
  const unsigned n = ncand;
  if (n <= (unsigned)kCand) {
    if (wv == 0) {
      unsigned long long a = (unsigned)lane < n ? cand[lane] : 0ull;
      unsigned long long b = (unsigned)(lane + 64) < n ? cand[lane + 64] : 0ull;
      for (int rd = 0; rd < k; ++rd) {
        const unsigned long long best = __ockl_wfred_max_u64(a > b ? a : b);
        if (lane == 0) emit(rd, best);
        if (a == best) a = 0ull;
        if (b == best) b = 0ull;
      }
    }
    return;
  }
  int chosen[4] = {-1, -1, -1, -1};
  for (int rd = 0; rd < k; ++rd) {
    unsigned long long best = 0;
    for (int i = tid; i < V; i += TPB) {
      const float xv = h2f_(x[i]);
      if (xv < thr) continue;
      bool taken = false;
#pragma unroll
      for (int q = 0; q < 4; ++q) taken |= (q < rd && chosen[q] == i);
      if (taken) continue;
      const unsigned long long key = key_of(xv, (unsigned)i);
      best = key > best ? key : best;
    }
    best = __ockl_wfred_max_u64(best);
    if (lane == 0) ksh[wv] = best;
    __syncthreads();
    unsigned long long b = ksh[0];
#pragma unroll
    for (int q = 1; q < NW; ++q) b = ksh[q] > b ? ksh[q] : b;
    __syncthreads();
    chosen[rd] = (int)(0xffffffffu - (unsigned)(b & 0xffffffffu));
    if (tid == 0) emit(rd, b);
  }
}

// split-row workspace: [kSplitRows] row counters at a FIXED offset (one
// workspace serves steps of every T: a counter must never share bytes with
// another T's partials), then [T][G <= 16] partial sums
constexpr int kSplitRows = 256;
constexpr size_t kSplitPartOff = kSplitRows * 4;
size_t argmax_workspace_bytes(int T) {
  return T <= 0 ? 0 : kSplitPartOff + (size_t)std::min(T, kSplitRows) * 16 * 8;
}

hipError_t launch_argmax(const uint16_t *logits, int T, int V, int k, int32_t *ids,
                         float *probs, hipStream_t s, void *ws, size_t ws_bytes, int32_t *ids2) {
  if (T <= 0) return hipSuccess;
  if (k < 1 || k > 4) return hipErrorInvalidValue;
  // workgroups per row (the split form needs the caller's zeroed workspace):
  // T x G <= 256, one workgroup per CU; FFMI_TOPK_SPLIT = 0 (off) / G (forced)
  static const int split_env = getenv("FFMI_TOPK_SPLIT") ? atoi(getenv("FFMI_TOPK_SPLIT")) : -1;
  // (T 129-256, the verify step's argmax, two workgroups per row with
  // FFMI_TOPK_SPLIT2=1: measured slower, 20.0 vs 13.1 us at T = 168 after the
  // lm_head GEMM -- 336 workgroups put two on many CUs -- and the verify step
  // 5.30 vs 5.28 ms; off)
  static const bool split2 = getenv("FFMI_TOPK_SPLIT2") && atoi(getenv("FFMI_TOPK_SPLIT2"));
  // (T <= 16 took 16 before: 8 measured 0.5 us faster at T = 8, k 1 and 3,
  // profiles/r06_topk_g.log)
  int G = T <= 32 ? 8 : T <= 64 ? 4 : T <= 128 ? 2 : (T <= kSplitRows && split2) ? 2 : 1;
  if (split_env >= 0) G = split_env;
  if (!ws || ws_bytes < argmax_workspace_bytes(T) || T > kSplitRows) G = 1;
  unsigned *cnt = reinterpret_cast<unsigned *>(ws);
  double *part = ws ? reinterpret_cast<double *>(static_cast<char *>(ws) + kSplitPartOff) : nullptr;
  // workgroup width (A/B: FFMI_TOPK_TPB = 256 / 512 / 1024)
  static const int tpb = [] {
    const char *e = getenv("FFMI_TOPK_TPB");
    const int v = e ? atoi(e) : 1024;
    return v == 256 || v == 512 ? v : 1024;
  }();
  const int nv = (V / 8 + tpb - 1) / tpb;
  // (NV = 8 at 1024 threads would spill: larger vocabularies take the loop kernel)
  if (V % 8 == 0 && ((uintptr_t)logits & 15) == 0 && nv * tpb <= 4096) {
#define FFMI_SMR(TPB, NV)                                                                  \
  hipLaunchKernelGGL((softmax_topk_reg_kernel<TPB, NV, 1>), dim3(T), dim3(TPB), 0, s, logits, V, \
                     k, ids, probs, nullptr, nullptr, ids2)
#define FFMI_SMG(NV, GG)                                                                     \
  hipLaunchKernelGGL((softmax_topk_reg_kernel<1024, NV, GG>), dim3(GG, T), dim3(1024), 0, s, \
                     logits, V, k, ids, probs, part, cnt, ids2)
    const int gmax = 4 * std::max(1, nv);  // >= 2 of a thread's 8 NV elements per workgroup
    while (G > 1 && (G > gmax || (G & (G - 1)))) G >>= 1;
    if (tpb == 1024 && G > 1) {
      if (nv <= 1) {
        if (G >= 4) FFMI_SMG(1, 4);
        else FFMI_SMG(1, 2);
      } else if (nv <= 2) {
        if (G >= 8) FFMI_SMG(2, 8);
        else if (G == 4) FFMI_SMG(2, 4);
        else FFMI_SMG(2, 2);
      } else {
        if (G >= 16) FFMI_SMG(4, 16);
        else if (G == 8) FFMI_SMG(4, 8);
        else if (G == 4) FFMI_SMG(4, 4);
        else FFMI_SMG(4, 2);
      }
    } else if (tpb == 256) {
      if (nv <= 4) FFMI_SMR(256, 4);
      else if (nv <= 8) FFMI_SMR(256, 8);
      else FFMI_SMR(256, 16);
    } else if (tpb == 512) {
      if (nv <= 2) FFMI_SMR(512, 2);
      else if (nv <= 4) FFMI_SMR(512, 4);
      else FFMI_SMR(512, 8);
    } else {
      if (nv <= 1) FFMI_SMR(1024, 1);
      else if (nv <= 2) FFMI_SMR(1024, 2);
      else FFMI_SMR(1024, 4);
    }
#undef FFMI_SMR
#undef FFMI_SMG
  } else {
    hipLaunchKernelGGL(softmax_topk_kernel<1024>, dim3(T), dim3(1024), 0, s, logits, V, k, ids, probs,
                       ids2);
  }
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Top-p sampling (llama.cc:286-289: scalar_truediv by the temperature ->
// softmax -> sampling.cu), one workgroup per row, no sort:
//   z_i = half(x_i / half(temperature))          (element_unary.cu:80-81,136)
//   p_i = half(expf(z_i - M) / S), the top-k kernels' probability on z
//   order (p desc, index asc) (the stable radix sort of sampling.cu:122-135),
//   pick the first token whose cumulative p reaches t = (u * topp) * topp
//   (sampling.cu:81,99-100 compares prefix / topp >= u * topp), else the last
//   token of the order (sampling.cu:94).
// For p >= 0 the fp16 bit pattern is a monotone key and p <= 1 leaves 15361 of
// them, every p a multiple of 2^-24 and a row's sum below 2: the cumulative
// sums are exact in 32-bit integers of that unit, in any summation order.
//  1. z (kept as fp16 in the row's workspace), the row maximum;
//  2. S = float(double sum of expf_ref terms), as the top-k kernels';
//  3. every p_i: its key replaces z in the workspace and its integer mass goes
//     to an LDS histogram over the keys (LDS atomics: a softmax row spreads
//     over thousands of keys, so few of them collide);
//  4. a workgroup scan from the top key down finds the key K at which the
//     cumulative mass reaches ceil(t * 2^24), and from the mass above K the
//     rank r, in index order, of the pick among the tokens holding K;
//  5. the tokens holding K are counted per 64 consecutive indices (one wave
//     ballot each, the counts in the histogram's LDS), a second scan finds the
//     group of rank r, and the wave that owns the group emits its lane.
// The workspace element i is only ever touched by thread i % TPB.
// ---------------------------------------------------------------------------
constexpr int kSampleKeys = 0x3c00 + 1;  // keys of p in [0, 1]
constexpr int kSampleTPB = 1024;

__device__ __forceinline__ unsigned p_mass(unsigned key) {  // p / 2^-24, key <= 0x3c00
  const unsigned e = key >> 10, m = key & 1023u;
  return e ? (1024u + m) << (e - 1) : m;
}

// First position q (scan order: ascending, or descending when DESC) at which
// the running sum of arr[0 .. N) reaches target (>= 1): res = {q, sum before
// q}, or {-1, .} when the whole array sums to less.  Each thread sums a
// contiguous run, a wave scan and the waves' totals order the runs, and the
// one thread whose run crosses the target walks it.  Ends with a barrier.
template <int TPB, bool DESC>
__device__ __forceinline__ void block_find(const unsigned *arr, int N, unsigned target,
                                           unsigned *wsum, int *res) {
  constexpr int NW = TPB / 64;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int L = (N + TPB - 1) / TPB;
  const int q0 = min(tid * L, N), q1 = min(q0 + L, N);
  auto at = [&](int q) -> unsigned { return arr[DESC ? N - 1 - q : q]; };
  unsigned s = 0;
  for (int q = q0; q < q1; ++q) s += at(q);
  unsigned inc = s;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned t = __shfl_up(inc, o);
    if (lane >= o) inc += t;
  }
  if (lane == 63) wsum[wv] = inc;
  if (tid == 0) res[0] = -1;
  __syncthreads();
  unsigned c = inc - s;
#pragma unroll
  for (int q = 0; q < NW; ++q)
    if (q < wv) c += wsum[q];
  if (c < target && target - c <= s)
    for (int q = q0; q < q1; ++q) {
      const unsigned v = at(q);
      if (target - c <= v) {
        res[0] = q;
        res[1] = (int)c;
        break;
      }
      c += v;
    }
  __syncthreads();
}

// HWEXP (FFMI_SAMPLE_HWEXP=1, A/B runs only: not the rule's p): the hardware
// exp2 in place of expf_ref, to measure what the exact terms cost
template <int TPB, bool HWEXP>
__global__ __launch_bounds__(TPB) void sample_topp_kernel(
    const uint16_t *__restrict__ logits, int V, float temperature, float topp,
    const float *__restrict__ u, int32_t *__restrict__ ids, float *__restrict__ probs,
    uint16_t *__restrict__ pws) {
  constexpr int NW = TPB / 64;
  __shared__ unsigned hist[kSampleKeys];
  __shared__ double sh[NW];
  __shared__ unsigned wsum[NW];
  __shared__ int res[2];
  float *fsh = reinterpret_cast<float *>(sh);
  unsigned long long *ksh = reinterpret_cast<unsigned long long *>(sh);
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint16_t *x = logits + (size_t)row * V;
  uint16_t *w = pws + (size_t)row * V;
  auto ex = [](float d) -> float { return HWEXP ? __expf(d) : expf_ref(d); };
  for (int i = tid; i < kSampleKeys; i += TPB) hist[i] = 0;
  const float th = h2f_(f2h_(temperature));
  float mx = -INFINITY;
  for (int i = tid; i < V; i += TPB) {
    const uint16_t z = f2h_(__fdiv_rn(h2f_(x[i]), th));
    w[i] = z;
    mx = fmaxf(mx, h2f_(z));
  }
  mx = __ockl_wfred_max_f32(mx);
  if (lane == 0) fsh[wv] = mx;
  __syncthreads();
  float M = fsh[0];
#pragma unroll
  for (int q = 1; q < NW; ++q) M = fmaxf(M, fsh[q]);
  __syncthreads();
  double se = 0.0;
  for (int i = tid; i < V; i += TPB) se += (double)ex(h2f_(w[i]) - M);
  se = __ockl_wfred_add_f64(se);
  if (lane == 0) sh[wv] = se;
  __syncthreads();
  double sd = 0.0;
#pragma unroll
  for (int q = 0; q < NW; ++q) sd += sh[q];
  const float S = (float)sd;
  __syncthreads();
  // the last token of the order (lowest p, then highest index), for a row
  // whose whole mass stays below t: the largest (~key, index)
  unsigned long long lastk = 0;
  for (int i = tid; i < V; i += TPB) {
    const unsigned key = f2h_(__fdiv_rn(ex(h2f_(w[i]) - M), S));
    w[i] = (uint16_t)key;
    // (a NaN row -- an infinite logit -- has keys outside the histogram: no mass)
    if (key < (unsigned)kSampleKeys && key) atomicAdd(&hist[key], p_mass(key));
    const unsigned long long lk = ((unsigned long long)(0xffffu - key) << 32) | (unsigned)i;
    lastk = lk > lastk ? lk : lastk;
  }
  lastk = __ockl_wfred_max_u64(lastk);
  if (lane == 0) ksh[wv] = lastk;
  // t * 2^24 rounded up: the smallest integer mass that reaches t
  unsigned target;
  {
    const double t = __dmul_rn(__dmul_rn((double)u[row], (double)topp), (double)topp);
    const double tm = ceil(__dmul_rn(t, 16777216.0));
    target = tm >= 1.0 ? (tm < 4.0e9 ? (unsigned)tm : 4000000000u) : 1u;
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < NW; ++q) lastk = ksh[q] > lastk ? ksh[q] : lastk;
  block_find<TPB, true>(hist, kSampleKeys, target, wsum, res);
  const int kq = res[0];
  if (kq < 0) {  // (uniform: the whole workgroup leaves)
    if (tid == 0) {
      const int i = (int)(lastk & 0xffffffffu);
      ids[row] = i;
      if (probs) probs[row] = h2f_((uint16_t)(0xffffu - (unsigned)(lastk >> 32)));
    }
    return;
  }
  const unsigned K = (unsigned)(kSampleKeys - 1 - kq);
  const unsigned pm = p_mass(K);
  const unsigned rank = (target - (unsigned)res[1] + pm - 1) / pm - 1;  // 0-based, among K's tokens
  __syncthreads();  // (every thread has read res; hist becomes the group counts)
  const int nchunk = (V + TPB - 1) / TPB;
  for (int j = 0; j < nchunk; ++j) {
    const int i = j * TPB + tid;
    const unsigned long long b = __ballot(i < V && w[i] == (uint16_t)K);
    if (lane == 0) hist[j * NW + wv] = (unsigned)__popcll(b);
  }
  __syncthreads();
  block_find<TPB, false>(hist, nchunk * NW, rank + 1, wsum, res);
  const int g = res[0];
  if (g < 0 || g % NW != wv) return;
  const int i = (g / NW) * TPB + tid;
  const bool hit = i < V && w[i] == (uint16_t)K;
  const unsigned long long b = __ballot(hit);
  const unsigned below = (unsigned)__popcll(b & ((1ull << lane) - 1ull));
  if (hit && below == rank - (unsigned)res[1]) {
    ids[row] = i;
    if (probs) probs[row] = h2f_((uint16_t)K);
  }
}

// one 16-bit word per logit; the histogram's LDS, reused for the counts of
// whole chunks of 64-index groups, bounds the row length
constexpr int kSampleMaxV = kSampleKeys / (kSampleTPB / 64) * kSampleTPB;
size_t sample_topp_workspace_bytes(int T, int V) {
  return T <= 0 || V <= 0 ? 0 : (size_t)T * (size_t)V * sizeof(uint16_t);
}

hipError_t launch_sample_topp(const uint16_t *logits, int T, int V, float temperature, float topp,
                              const float *u, int32_t *ids, float *probs, void *ws,
                              size_t ws_bytes, hipStream_t s) {
  if (T <= 0) return hipSuccess;
  if (V < 1 || V > kSampleMaxV || !ws || ws_bytes < sample_topp_workspace_bytes(T, V))
    return hipErrorInvalidValue;
  static const bool hwexp = getenv("FFMI_SAMPLE_HWEXP") && atoi(getenv("FFMI_SAMPLE_HWEXP"));
  if (hwexp)
    hipLaunchKernelGGL((sample_topp_kernel<kSampleTPB, true>), dim3(T), dim3(kSampleTPB), 0, s, logits,
                       V, temperature, topp, u, ids, probs, reinterpret_cast<uint16_t *>(ws));
  else
    hipLaunchKernelGGL((sample_topp_kernel<kSampleTPB, false>), dim3(T), dim3(kSampleTPB), 0, s, logits,
                       V, temperature, topp, u, ids, probs, reinterpret_cast<uint16_t *>(ws));
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Vocab-sharded greedy / speculative tail (model.cc:3392-3419 shards lm_head
// over the vocabulary and Combines; here every rank keeps its [T][V/P] logit
// shard and three small exchanges of per-row records make the pick global):
//   phase 0: local max m_r                     -> exchange -> M = max_r m_r
//   phase 1: local sum of exp(x - M) (double)  -> exchange -> S = float(sum)
//   phase 2: local top-k of p = half(exp(x-M)/S) (p desc, lowest global id)
//            -> exchange -> merge: the k best of the P*k candidates.
// M and S are the unsharded kernel's values (a max is exact; S is the float
// rounding of the same double sum, accumulated per shard then over ranks in
// rank order), and p is computed with the same expressions, so the pick and
// its tie rule (lowest index of the largest fp16 p, cub ArgMax / the top-k
// heap) are those of the one-GPU kernel.  Exchange records are [P][T][W]
// floats: a rank writes its own slot and zeroes the others, and the sum
// all-reduce then acts as an all-gather (x + 0 = x).
// ---------------------------------------------------------------------------
template <int TPB>
__global__ __launch_bounds__(TPB) void vshard_kernel(const uint16_t *__restrict__ logits, int T,
                                                      int Vl, int P, int rank, int k, int phase,
                                                      float *__restrict__ xch, int W,
                                                      int32_t *__restrict__ ids,
                                                      float *__restrict__ probs) {
  constexpr int NW = TPB / 64;
  constexpr int kCand = 128;
  __shared__ double dsh[NW];
  __shared__ float fsh[NW];
  __shared__ unsigned long long ksh[NW];
  __shared__ unsigned long long cand[kCand];
  __shared__ unsigned ncand;
  const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint16_t *x = logits + (size_t)t * Vl;
  auto slot = [&](int r) { return xch + ((size_t)r * T + t) * W; };
  if (phase == 3) {  // merge the P*k candidates of the last exchange
    if (tid == 0) {
      int taken[4] = {-1, -1, -1, -1};
      for (int rd = 0; rd < k; ++rd) {
        unsigned long long best = 0;
        int bq = -1;
        for (int r = 0; r < P; ++r)
          for (int j = 0; j < k; ++j) {
            const float pv = slot(r)[2 * j], iv = slot(r)[2 * j + 1];
            if (iv < 0.f) continue;  // (empty candidate)
            const int q = r * k + j;
            bool used = false;
            for (int z = 0; z < rd; ++z) used |= taken[z] == q;
            if (used) continue;
            const unsigned long long key =
                ((unsigned long long)(f2h_(pv) + 1u) << 32) |
                (unsigned long long)(0xffffffffu - (unsigned)iv);
            if (key > best) best = key, bq = q;
          }
        taken[rd] = bq;
        ids[(size_t)t * k + rd] = (int)(0xffffffffu - (unsigned)(best & 0xffffffffu));
        if (probs) probs[(size_t)t * k + rd] = h2f_((uint16_t)((best >> 32) - 1u));
      }
    }
    return;
  }
  float *own = slot(rank);
  if (phase == 0) {
    float m = -INFINITY;
    for (int i = tid; i < Vl; i += TPB) m = fmaxf(m, h2f_(x[i]));
    m = __ockl_wfred_max_f32(m);
    if (lane == 0) fsh[wv] = m;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NW; ++q) m = fmaxf(m, fsh[q]);
    if (tid < P * W) {
      const int r = tid / W, w = tid % W;
      slot(r)[w] = (r == rank && w == 0) ? m : 0.f;
    }
    return;
  }
  float M = -INFINITY;
  for (int r = 0; r < P; ++r) M = fmaxf(M, xch[((size_t)r * T + t) * W]);  // phase-0 records
  if (phase == 1) {
    // (exchange buffer: [P][T][W] of phase 0 is read above and rewritten
    //  below only after the whole block has read it)
    double se = 0.0;
    for (int i = tid; i < Vl; i += TPB) se += (double)expf_ref(h2f_(x[i]) - M);
    se = __ockl_wfred_add_f64(se);
    if (lane == 0) dsh[wv] = se;
    __syncthreads();
    se = 0.0;
#pragma unroll
    for (int q = 0; q < NW; ++q) se += dsh[q];
    if (tid < P * W) {
      const int r = tid / W, w = tid % W;
      const float hi = (float)se, lo = (float)(se - (double)hi);
      slot(r)[w] = r != rank ? 0.f : (w == 0 ? M : w == 1 ? hi : w == 2 ? lo : 0.f);
    }
    return;
  }
  // phase 2: global S from the phase-1 records, local top-k candidates --
  // only logits whose fp16 p can reach the k-th largest local wave maximum's
  // p are evaluated (the threshold of softmax_topk_reg_kernel), through an
  // LDS list picked by one wave; k workgroup-wide rounds if it overflows
  double sd = 0.0;
  for (int r = 0; r < P; ++r) {
    const float *q = xch + ((size_t)r * T + t) * W;
    sd += (double)q[1] + (double)q[2];
  }
  const float S = (float)sd;
  if (tid == 0) ncand = 0;
  float wm = -INFINITY;
  for (int i = tid; i < Vl; i += TPB) wm = fmaxf(wm, h2f_(x[i]));
  wm = __ockl_wfred_max_f32(wm);
  if (lane == 0) fsh[wv] = wm;
  __syncthreads();  // (also: every thread has read the phase-1 records)
  float L = -INFINITY;
  {
    float top[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int q = 0; q < NW; ++q) {
      float v = fsh[q];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float hi = fmaxf(top[j], v), lo = fminf(top[j], v);
        top[j] = hi, v = lo;
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j == k - 1) L = top[j];
  }
  float thr = -3.402823466e38f;
  {
    const uint16_t pL = f2h_(__fdiv_rn(expf_ref(L - M), S));
    if (pL > 1) {
      const float lo = 0.5f * (h2f_(pL) + h2f_((uint16_t)(pL - 1)));
      thr = M + logf(lo * S) - 0.0009765625f * fmaxf(1.0f, fabsf(M));
    }
  }
  auto key_of = [&](float xv, int i) -> unsigned long long {
    const uint16_t p = f2h_(__fdiv_rn(expf_ref(xv - M), S));
    const unsigned gi = (unsigned)(rank * Vl + i);
    return ((unsigned long long)(p + 1u) << 32) | (unsigned long long)(0xffffffffu - gi);
  };
  auto emit = [&](int rd, unsigned long long b) {
    own[2 * rd] = b ? h2f_((uint16_t)((b >> 32) - 1u)) : 0.f;
    own[2 * rd + 1] = b ? (float)(0xffffffffu - (unsigned)(b & 0xffffffffu)) : -1.f;
  };
  for (int i = tid; i < Vl; i += TPB) {
    const float xv = h2f_(x[i]);
    if (xv >= thr) {
      const unsigned sl = atomicAdd(&ncand, 1u);
      if (sl < (unsigned)kCand) cand[sl] = key_of(xv, i);
    }
  }
  __syncthreads();
  const unsigned n = ncand;
  if (n <= (unsigned)kCand) {
    if (wv == 0) {  // keys are distinct (they hold the index)
      unsigned long long a = (unsigned)lane < n ? cand[lane] : 0ull;
      unsigned long long b = (unsigned)(lane + 64) < n ? cand[lane + 64] : 0ull;
      for (int rd = 0; rd < k; ++rd) {
        const unsigned long long best = __ockl_wfred_max_u64(a > b ? a : b);
        if (lane == 0) emit(rd, best);
        if (best) {
          if (a == best) a = 0ull;
          if (b == best) b = 0ull;
        }
      }
    }
  } else {
    int chosen[4] = {-1, -1, -1, -1};
    for (int rd = 0; rd < k; ++rd) {
      unsigned long long best = 0;
      for (int i = tid; i < Vl; i += TPB) {
        const float xv = h2f_(x[i]);
        if (xv < thr) continue;
        bool used = false;
#pragma unroll
        for (int z = 0; z < 4; ++z) used |= (z < rd && chosen[z] == i);
        if (used) continue;
        const unsigned long long key = key_of(xv, i);
        best = key > best ? key : best;
      }
      best = __ockl_wfred_max_u64(best);
      if (lane == 0) ksh[wv] = best;
      __syncthreads();
      unsigned long long b = ksh[0];
#pragma unroll
      for (int q = 1; q < NW; ++q) b = ksh[q] > b ? ksh[q] : b;
      __syncthreads();
      chosen[rd] = b ? (int)(0xffffffffu - (unsigned)(b & 0xffffffffu)) - rank * Vl : -1;
      if (tid == 0) emit(rd, b);
    }
  }
  if (tid < P * W) {  // zero the other ranks' slots and this slot's unused tail
    const int r = tid / W, w = tid % W;
    if (r != rank) slot(r)[w] = 0.f;
    else if (w >= 2 * k) own[w] = 0.f;
  }
}

hipError_t launch_vshard(const uint16_t *logits, int T, int Vl, int P, int rank, int k,
                         int phase, float *xch, int W, int32_t *ids, float *probs,
                         hipStream_t s) {
  if (T <= 0) return hipSuccess;
  if (k < 1 || k > 4 || P * W > 256 || W < 2 * k || W < 4) return hipErrorInvalidValue;
  hipLaunchKernelGGL((vshard_kernel<1024>), dim3(T), dim3(1024), 0, s, logits, T, Vl, P, rank, k,
                     phase, xch, W, ids, probs);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Vocab-sharded top-p sampling: sample_topp_kernel's rule on logits that stay
// sharded ([T][Vl] per rank, ids [rank*Vl, (rank+1)*Vl)).  The masses are
// integers (multiples of 2^-24), so their sums do not depend on how the
// vocabulary is split, and every rank derives the same pick from small
// per-row records -- five exchanges, never the logits:
//   phase 0: z = half(x / half(temperature)) into the row's key workspace,
//            local max                       -> exchange -> M = max over ranks
//   phase 1: local double sum of exp(z - M)  -> exchange -> S = float(sum)
//   phase 2: key = half(exp(z - M) / S) replaces z; the 15361-key LDS mass
//            histogram, summed into the 121 buckets key >> 7; the rank's last
//            token of the order (lowest key, highest index)
//                                            -> exchange -> the bucket B at
//            which the cumulative mass from the top reaches the target (none:
//            the row falls back to the last token over the ranks)
//   phase 3: tokens per key for the 128 keys of B -> exchange -> the key K,
//            the rank r of the pick among K's tokens in global index order,
//            the owner (first rank whose prefix of counts exceeds r)
//   phase 4: the owner finds its (r - prefix)-th token holding K (the ballot
//            counts of sample_topp_kernel)   -> exchange -> the global id
//   phase 5: ids / probs on every rank.
// Exchange records are [P][rows][W] floats, W per phase (kVsW): a rank writes
// its own slot and zeroes the others, the sum all-reduce is an all-gather.
// Every value sent is an integer below 2^24 or a float sent as is (masses and
// ids go as v >> 12 and v & 4095), so x + 0 = x holds exactly.  What a row
// needs from one launch to the next and every rank derives alike (M, target,
// B, the mass above B, the fallback token, K) is kept in `state`, local memory
// that is not exchanged.  The workspace element i is only touched by thread
// i % TPB.  A phase's record width differs from the one before it, so a
// workgroup's slots would overlap another row's unread ones in one buffer: the
// records alternate between two buffers (a launch reads xin, the all-reduced
// records of the phase before, and writes xout).
// ---------------------------------------------------------------------------
constexpr int kVsBuckets = (kSampleKeys + 127) / 128;  // 121
// (multiples of 4 floats: the transport moves 16-byte vectors)
constexpr int kVsUsed[5] = {1, 2, 2 * kVsBuckets + 3, 128, 2};
constexpr int kVsW[5] = {4, 4, (kVsUsed[2] + 3) & ~3, 128, 4};
constexpr int kVsMaxW = 256;
enum { VS_M, VS_TARGET, VS_FALLBACK, VS_B, VS_C, VS_FB_ID, VS_FB_KEY, VS_K, kVsState };
static_assert(kVsW[2] <= kVsMaxW && kVsW[3] <= kVsMaxW, "exchange record width");

__device__ __forceinline__ void vs_put(float *p, unsigned v) {
  p[0] = (float)(v >> 12), p[1] = (float)(v & 4095u);
}
__device__ __forceinline__ unsigned vs_get(const float *p) {
  return (unsigned)p[0] * 4096u + (unsigned)p[1];
}

template <int TPB, int PHASE>
__global__ __launch_bounds__(TPB) void vshard_sample_kernel(
    const uint16_t *__restrict__ logits, int Vl, int P, int rank, int row0, float temperature,
    float topp, const float *__restrict__ u, uint16_t *__restrict__ kws,
    unsigned *__restrict__ state, const float *__restrict__ xin, float *__restrict__ xout,
    int32_t *__restrict__ ids, float *__restrict__ probs) {
  constexpr int NW = TPB / 64;
  constexpr int WR = kVsW[PHASE > 0 ? PHASE - 1 : 0];  // records read
  constexpr int WW = kVsW[PHASE < 5 ? PHASE : 4];      // records written
  const int b = blockIdx.x, n = gridDim.x, t = row0 + b;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint16_t *x = logits + (size_t)t * Vl;
  uint16_t *w = kws + (size_t)t * Vl;
  unsigned *st = state + (size_t)t * kVsState;
  auto rd = [&](int r) -> const float * { return xin + ((size_t)r * n + b) * WR; };
  auto wr = [&](int r) -> float * { return xout + ((size_t)r * n + b) * WW; };
  float *own = wr(rank);
  // the other ranks' slots and this slot from `used` on (a loop: the records
  // are wider than the workgroup at P * WW > TPB)
  auto zero_slots = [&](int used) {
    for (int q = tid; q < P * WW; q += TPB) {
      const int r = q / WW;
      if (r != rank || q - r * WW >= used) wr(r)[q - r * WW] = 0.f;
    }
  };
  (void)lane, (void)wv, (void)x, (void)w, (void)rd, (void)own, (void)zero_slots;

  if constexpr (PHASE == 0) {
    __shared__ float fsh[NW];
    const float th = h2f_(f2h_(temperature));
    float mx = -INFINITY;
    for (int i = tid; i < Vl; i += TPB) {
      const uint16_t z = f2h_(__fdiv_rn(h2f_(x[i]), th));
      w[i] = z;
      mx = fmaxf(mx, h2f_(z));
    }
    mx = __ockl_wfred_max_f32(mx);
    if (lane == 0) fsh[wv] = mx;
    __syncthreads();
    float M = fsh[0];
#pragma unroll
    for (int q = 1; q < NW; ++q) M = fmaxf(M, fsh[q]);
    zero_slots(kVsUsed[0]);
    if (tid == 0) own[0] = M;
  } else if constexpr (PHASE == 1) {
    __shared__ double dsh[NW];
    float M = -INFINITY;
    for (int r = 0; r < P; ++r) M = fmaxf(M, rd(r)[0]);
    double se = 0.0;
    for (int i = tid; i < Vl; i += TPB) se += (double)expf_ref(h2f_(w[i]) - M);
    se = __ockl_wfred_add_f64(se);
    if (lane == 0) dsh[wv] = se;
    __syncthreads();  // (also: every thread has read the phase-0 records)
    se = 0.0;
#pragma unroll
    for (int q = 0; q < NW; ++q) se += dsh[q];
    zero_slots(kVsUsed[1]);
    if (tid == 0) {
      const float hi = (float)se;
      own[0] = hi, own[1] = (float)(se - (double)hi);
      st[VS_M] = __float_as_uint(M);
    }
  } else if constexpr (PHASE == 2) {
    __shared__ unsigned hist[kSampleKeys];
    __shared__ unsigned long long ksh[NW];
    for (int i = tid; i < kSampleKeys; i += TPB) hist[i] = 0;
    double sd = 0.0;
    for (int r = 0; r < P; ++r) sd += (double)rd(r)[0] + (double)rd(r)[1];
    const float S = (float)sd, M = __uint_as_float(st[VS_M]);
    __syncthreads();  // (also: every thread has read the phase-1 records)
    // this rank's last token of the order: the largest (~key, local index)
    unsigned long long lastk = 0;
    for (int i = tid; i < Vl; i += TPB) {
      const unsigned key = f2h_(__fdiv_rn(expf_ref(h2f_(w[i]) - M), S));
      w[i] = (uint16_t)key;
      // (a NaN row -- an infinite logit -- has keys outside the histogram: no mass)
      if (key < (unsigned)kSampleKeys && key) atomicAdd(&hist[key], p_mass(key));
      const unsigned long long lk = ((unsigned long long)(0xffffu - key) << 32) | (unsigned)i;
      lastk = lk > lastk ? lk : lastk;
    }
    lastk = __ockl_wfred_max_u64(lastk);
    if (lane == 0) ksh[wv] = lastk;
    __syncthreads();
    // the mass of each bucket key >> 7, a wave per bucket
    for (int bk = wv; bk < kVsBuckets; bk += NW) {
      const int k0 = bk * 128 + lane, k1 = k0 + 64;
      unsigned m = (k0 < kSampleKeys ? hist[k0] : 0u) + (k1 < kSampleKeys ? hist[k1] : 0u);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) m += __shfl_xor(m, o);
      if (lane == 0) vs_put(own + 2 * bk, m);
    }
    zero_slots(kVsUsed[2]);
    if (tid == 0) {
#pragma unroll
      for (int q = 0; q < NW; ++q) lastk = ksh[q] > lastk ? ksh[q] : lastk;
      own[2 * kVsBuckets] = (float)(0xffffu - (unsigned)(lastk >> 32));
      vs_put(own + 2 * kVsBuckets + 1, (unsigned)rank * (unsigned)Vl + (unsigned)(lastk & 0xffffffffu));
    }
  } else if constexpr (PHASE == 3) {
    __shared__ unsigned coarse[128], cnt[128], wsum[NW];
    __shared__ int res[2];
    if (tid < 128) {
      unsigned m = 0;
      if (tid < kVsBuckets)
        for (int r = 0; r < P; ++r) m += vs_get(rd(r) + 2 * tid);
      coarse[tid] = m, cnt[tid] = 0;
    }
    // the last token of the order over the ranks: lowest key, highest id
    unsigned fb_key = 0xffffffffu, fb_id = 0;
    if (tid == 0)
      for (int r = 0; r < P; ++r) {
        const unsigned key = (unsigned)rd(r)[2 * kVsBuckets];
        if (key <= fb_key) fb_key = key, fb_id = vs_get(rd(r) + 2 * kVsBuckets + 1);
      }
    // t * 2^24 rounded up: the smallest integer mass that reaches t
    unsigned target;
    {
      const double tt = __dmul_rn(__dmul_rn((double)u[t], (double)topp), (double)topp);
      const double tm = ceil(__dmul_rn(tt, 16777216.0));
      target = tm >= 1.0 ? (tm < 4.0e9 ? (unsigned)tm : 4000000000u) : 1u;
    }
    __syncthreads();  // (also: the phase-2 records are read)
    block_find<TPB, true>(coarse, kVsBuckets, target, wsum, res);
    const int kq = res[0];
    const unsigned B = (unsigned)(kVsBuckets - 1 - kq);
    if (kq >= 0) {  // (uniform) this rank's tokens per key of bucket B, one add per wave and key
      const int nchunk = (Vl + TPB - 1) / TPB;
      for (int j = 0; j < nchunk; ++j) {
        const int i = j * TPB + tid;
        const unsigned key = i < Vl ? w[i] : 0xffffu;
        const bool in = key < (unsigned)kSampleKeys && (key >> 7) == B;
        unsigned long long m = __ballot(in);
        while (m) {
          const int l = __ffsll((long long)m) - 1;
          const unsigned k0 = __shfl(key, l);
          const unsigned long long same = __ballot(in && key == k0);
          if (lane == l) atomicAdd(&cnt[k0 & 127u], (unsigned)__popcll(same));
          m &= ~same;
        }
      }
    }
    __syncthreads();
    zero_slots(kVsUsed[3]);
    if (tid < 128) own[tid] = (float)cnt[tid];  // (<= Vl < 2^24)
    if (tid == 0) {
      st[VS_TARGET] = target, st[VS_FALLBACK] = kq < 0, st[VS_B] = B, st[VS_C] = (unsigned)res[1];
      st[VS_FB_ID] = fb_id, st[VS_FB_KEY] = fb_key;
    }
  } else if constexpr (PHASE == 4) {
    __shared__ unsigned hist[kSampleKeys];  // the counts per 64 consecutive indices
    __shared__ unsigned fm[128], wsum[NW];
    __shared__ int res[2];
    const bool fallback = st[VS_FALLBACK] != 0;
    const unsigned B = st[VS_B], target = st[VS_TARGET], c = st[VS_C];
    if (tid < 128) {  // the mass of each key of bucket B over the ranks
      unsigned tot = 0;
      for (int r = 0; r < P; ++r) tot += (unsigned)rd(r)[tid];
      const unsigned key = B * 128u + (unsigned)tid;
      fm[tid] = !fallback && key < (unsigned)kSampleKeys ? tot * p_mass(key) : 0u;
    }
    __syncthreads();
    int owner = -1;
    unsigned K = 0, rloc = 0;
    if (!fallback) {  // (uniform)
      block_find<TPB, true>(fm, 128, target - c, wsum, res);
      const int kq = res[0];
      if (kq >= 0) {
        K = B * 128u + 127u - (unsigned)kq;
        const unsigned pm = p_mass(K);
        // 0-based, among K's tokens in global index order
        const unsigned rk = (target - c - (unsigned)res[1] + pm - 1) / pm - 1;
        unsigned pre = 0;
        for (int r = 0; r < P; ++r) {
          const unsigned ck = (unsigned)rd(r)[K & 127u];
          if (owner < 0 && rk - pre < ck) owner = r, rloc = rk - pre;
          pre += ck;
        }
      }
    }
    __syncthreads();  // (every thread has read res and the phase-3 records)
    zero_slots(0);
    if (tid == 0) {
      st[VS_K] = K;
      if (owner < 0) st[VS_FALLBACK] = 1;  // (only a row outside the contract gets here)
    }
    if (owner == rank) {  // (uniform)
      const int nchunk = (Vl + TPB - 1) / TPB;
      for (int j = 0; j < nchunk; ++j) {
        const int i = j * TPB + tid;
        const unsigned long long bl = __ballot(i < Vl && w[i] == (uint16_t)K);
        if (lane == 0) hist[j * NW + wv] = (unsigned)__popcll(bl);
      }
      __syncthreads();
      block_find<TPB, false>(hist, nchunk * NW, rloc + 1, wsum, res);  // (barriers: after the zeroing)
      const int g = res[0];
      if (g >= 0 && g % NW == wv) {
        const int i = (g / NW) * TPB + tid;
        const bool hit = i < Vl && w[i] == (uint16_t)K;
        const unsigned long long bl = __ballot(hit);
        const unsigned below = (unsigned)__popcll(bl & ((1ull << lane) - 1ull));
        if (hit && below == rloc - (unsigned)res[1])
          vs_put(own, (unsigned)rank * (unsigned)Vl + (unsigned)i);
      }
    }
  } else {
    if (tid == 0) {
      unsigned id = 0, key = st[VS_K];
      if (st[VS_FALLBACK]) {
        id = st[VS_FB_ID], key = st[VS_FB_KEY];
      } else {
        for (int r = 0; r < P; ++r) id += vs_get(rd(r));
      }
      ids[t] = (int32_t)id;
      if (probs) probs[t] = h2f_((uint16_t)key);
    }
  }
}

int vshard_sample_record_floats(int phase) { return phase >= 0 && phase < 5 ? kVsW[phase] : 0; }
int vshard_sample_max_record_floats() { return kVsMaxW; }
size_t vshard_sample_state_bytes(int T) {
  return T <= 0 ? 0 : (size_t)T * kVsState * sizeof(unsigned);
}

hipError_t launch_vshard_sample(const uint16_t *logits, int Vl, int P, int rank, int row0,
                                int rows, int phase, float temperature, float topp,
                                const float *u, uint16_t *keys, unsigned *state, const float *xin,
                                float *xout, int32_t *ids, float *probs, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  if (Vl < 1 || Vl > kSampleMaxV || P < 1 || rank < 0 || rank >= P || !keys || !state || !xin ||
      !xout || xin == xout)
    return hipErrorInvalidValue;
#define FFMI_VS(PH)                                                                             \
  case PH:                                                                                      \
    hipLaunchKernelGGL((vshard_sample_kernel<kSampleTPB, PH>), dim3(rows), dim3(kSampleTPB), 0, \
                       s, logits, Vl, P, rank, row0, temperature, topp, u, keys, state, xin,    \
                       xout, ids, probs);                                                       \
    break
  switch (phase) {
    FFMI_VS(0);
    FFMI_VS(1);
    FFMI_VS(2);
    FFMI_VS(3);
    FFMI_VS(4);
    FFMI_VS(5);
    default: return hipErrorInvalidValue;
  }
#undef FFMI_VS
  return hipGetLastError();
}

// Sum of the ranks' buffers of an in-process shard group (ffmi_comm_create_
// local): out = sum over r in rank order, fp16 accumulated in fp32 then
// rounded once (RCCL's ring sums in fp16 in ring order; both are within an
// fp16 ulp of the exact sum).
struct GroupBufs {
  const void *p[8];
};
__global__ void group_sum_kernel(GroupBufs b, int n, void *__restrict__ out, size_t count,
                                 int dtype) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < count;
       i += (size_t)gridDim.x * blockDim.x) {
    if (dtype == FFMI_F16) {
      float a = 0.f;
      for (int r = 0; r < n; ++r) a += h2f_(reinterpret_cast<const uint16_t *>(b.p[r])[i]);
      reinterpret_cast<uint16_t *>(out)[i] = f2h_(a);
    } else if (dtype == FFMI_F32) {
      float a = 0.f;
      for (int r = 0; r < n; ++r) a += reinterpret_cast<const float *>(b.p[r])[i];
      reinterpret_cast<float *>(out)[i] = a;
    } else {
      int a = 0;
      for (int r = 0; r < n; ++r) a += reinterpret_cast<const int *>(b.p[r])[i];
      reinterpret_cast<int *>(out)[i] = a;
    }
  }
}

hipError_t launch_group_sum(const void *const *bufs, int n, void *out, size_t count, int dtype,
                            hipStream_t s) {
  if (n < 1 || n > 8) return hipErrorInvalidValue;
  if (count == 0) return hipSuccess;
  GroupBufs b;
  for (int r = 0; r < 8; ++r) b.p[r] = bufs[r < n ? r : 0];
  size_t blocks = (count + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(group_sum_kernel, dim3((unsigned)blocks), dim3(256), 0, s, b, n, out, count,
                     dtype);
  return hipGetLastError();
}

}  // namespace ffmi
