// norm.hip -- RMSNorm / ResidualRMSNorm, embedding, SiLU-mul, shard-group sum.
//
// HBM-bound row kernels: one 256-thread workgroup per row, 16-B vector
// loads/stores (8 halves per lane), the row kept in registers between the
// reduction and the scale pass (one read + one write per element).  Unlike
// the reference (which launches every buffer row, rms_norm_kernels.cu:133-134)
// only the T active rows are processed.
#include <algorithm>

#include "../ffmi_internal.h"
#include "half_bits.h"

namespace ffmi {

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
