// sampling.hip -- the fp16 token pick: softmax + argmax / arg-top-k, top-p
// sampling, and both under a vocab-sharded lm_head; and, at the end, the
// log-probability of a row's scored id (its own rule: the full softmax in fp32).
//
// Five kernels implement one rule -- p_i = half(expf(x_i - M) / S) with S =
// float(double sum), ordered by (p desc, index asc) -- and every decision of
// that rule that must be bit-exact is written once, in the helpers below:
//   exp_term / prob16 / block_sum_f64       the probability
//   kth_largest / cand_threshold            which logits can be in the top k
//   pick_key / pick_from_list / pick_by_rounds   the order and the selection
//   temper_row / key_mass_pass / topp_target / find_holder   top-p sampling
// One workgroup per row (HBM / L2-bound row kernels, as norm.hip's).
#include <algorithm>

#include "../ffmi_internal.h"
#include "expf_ref.h"
#include "half_bits.h"

namespace ffmi {

// Wave-wide reductions on DPP / permlane (device library), not LDS
// bpermute shuffles: the result is uniform across the wave.
extern "C" __device__ float __ockl_wfred_max_f32(float);
extern "C" __device__ double __ockl_wfred_add_f64(double);
extern "C" __device__ unsigned long long __ockl_wfred_max_u64(unsigned long long);

// ---------------------------------------------------------------------------
// Workgroup reductions over NW waves through an LDS array of NW entries.  Each
// has exactly ONE barrier, between the waves' stores and the reads: a caller
// that reuses the array afterwards places its own barrier.  lane, wv: the
// thread's lane and wave (threadIdx.x & 63, >> 6), which the kernel takes at
// its top and passes to these and to the pick helpers that call them: with
// the two derived here, at the lane-0 store, the streaming kernel's passes
// measured 1% slower.  (block_find and find_holder below work on tid and keep
// deriving all three themselves, as block_find always did: their kernels
// compile to the same registers and occupancy either way.)
// ---------------------------------------------------------------------------
// The waves' maxima (the row maximum M is max_of them, L is kth_largest).
template <int NW>
__device__ __forceinline__ void block_max_f32(float v, int lane, int wv, float *sh,
                                              float (&wmax)[NW]) {
  v = __ockl_wfred_max_f32(v);
  if (lane == 0) sh[wv] = v;
  __syncthreads();
#pragma unroll
  for (int q = 0; q < NW; ++q) wmax[q] = sh[q];
}
template <int NW>
__device__ __forceinline__ float max_of(const float (&wmax)[NW]) {
  float m = wmax[0];
#pragma unroll
  for (int q = 1; q < NW; ++q) m = fmaxf(m, wmax[q]);
  return m;
}
template <int NW>
__device__ __forceinline__ float block_max_f32(float v, int lane, int wv, float *sh) {
  float wmax[NW];
  block_max_f32<NW>(v, lane, wv, sh, wmax);
  return max_of(wmax);
}

// The double sum, the waves' sums added in wave order 0 .. NW-1.  S = float(
// this sum) is the oracle's float(double sum), whatever the summation order.
template <int NW>
__device__ __forceinline__ double block_sum_f64(double v, int lane, int wv, double *sh) {
  v = __ockl_wfred_add_f64(v);
  if (lane == 0) sh[wv] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int q = 0; q < NW; ++q) s += sh[q];
  return s;
}

// The u64 maximum: block_max_u64, or its two halves for a caller that has
// other work before the barrier, or in which one thread alone needs the
// result: put returns the wave's maximum, get (after the caller's barrier)
// folds the waves' into it.  (block_max_u64 folds from sh[0], get from the wave's
// own maximum: one value either way, but each caller keeps the form it was
// compiled with before -- folding from the wave's own in the register
// kernel's fallback moved the SGPR counts and spills of most of its variants,
// and folding from sh[0] in sample_topp_kernel took it from 65 to 64 VGPRs,
// two workgroups per CU, and 0.3 us slower.)
__device__ __forceinline__ unsigned long long wave_max_u64_put(unsigned long long v, int lane,
                                                               int wv, unsigned long long *sh) {
  v = __ockl_wfred_max_u64(v);
  if (lane == 0) sh[wv] = v;
  return v;
}
template <int NW>
__device__ __forceinline__ unsigned long long wave_max_u64_get(const unsigned long long *sh,
                                                               unsigned long long v) {
#pragma unroll
  for (int q = 0; q < NW; ++q) v = sh[q] > v ? sh[q] : v;
  return v;
}
template <int NW>
__device__ __forceinline__ unsigned long long block_max_u64(unsigned long long v, int lane,
                                                            int wv, unsigned long long *sh) {
  wave_max_u64_put(v, lane, wv, sh);
  __syncthreads();
  unsigned long long b = sh[0];
#pragma unroll
  for (int q = 1; q < NW; ++q) b = sh[q] > b ? sh[q] : b;
  return b;
}

// ---------------------------------------------------------------------------
// The probability.
// ---------------------------------------------------------------------------
// The terms of S and the p values use the oracle's expf (expf_ref): with the
// hardware exp2 (__expf, a few ulp) a peaked row, whose S a few terms
// dominate, took their errors straight into S's float rounding, and 1 p in
// ~10^4 came out one fp16 ulp off (the random-shape sweep of
// test_softmax_topk_random_shapes_exact).
// HWEXP (sample_topp_kernel's FFMI_SAMPLE_HWEXP=1, A/B runs only: not the
// rule's p): the hardware exp2, to measure what the exact terms cost.
template <bool HWEXP = false>
__device__ __forceinline__ float exp_term(float d) {
  return HWEXP ? __expf(d) : expf_ref(d);
}
// p = half(exp(x - M) / S), the division correctly rounded
template <bool HWEXP = false>
__device__ __forceinline__ uint16_t prob16(float x, float M, float S) {
  return f2h_(__fdiv_rn(exp_term<HWEXP>(x - M), S));
}

// ---------------------------------------------------------------------------
// The top-k rule: the k largest p, ties (created by the fp16 rounding) to the
// lowest index, exactly as cub ArgMax / the top-k heap resolve them.
//  * p_i is computed only for CANDIDATES: p is non-decreasing in x, and the
//    k-th largest of the per-wave maxima, L, is <= the row's k-th largest
//    logit (the waves' index sets are disjoint), so every member of the top-k
//    (ties included) has fp16 p >= p(L), i.e. an unrounded p_i above the lower
//    rounding boundary of p(L): x_i >= M + log(boundary * S).  That threshold
//    (lowered by a margin that covers the float error of exp/div/log) excludes
//    all but a handful of logits, and the 32000 exp + correctly rounded
//    divisions of a full p pass go away.
//  * The candidates' keys go to an LDS list of kCand entries; one wave picks
//    the k best (pick_from_list: k wave reductions, no workgroup barrier).
//    More than kCand candidates (flat rows, planted ties) fall back to k
//    rounds of a workgroup-wide selection over the row.
// ---------------------------------------------------------------------------
constexpr int kCand = 128;

// L = k-th largest wave maximum (k <= 4)
template <int NW>
__device__ __forceinline__ float kth_largest(const float (&wmax)[NW], int k) {
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
  float L = -INFINITY;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (j == k - 1) L = top[j];
  return L;
}

// candidate threshold from p(L): its lower fp16 rounding boundary, minus a
// margin of 2^-10 in x (>> the float error of exp, the division and log)
// (finite: logits set to -inf -- taken ones -- are never candidates; p(L) of
// 0 or the smallest subnormal -- L = -inf included -- admits every logit)
__device__ __forceinline__ float cand_threshold(float L, float M, float S) {
  float thr = -3.402823466e38f;
  const uint16_t pL = prob16(L, M, S);
  if (pL > 1) {
    const float lo = 0.5f * (h2f_(pL) + h2f_((uint16_t)(pL - 1)));
    thr = M + logf(lo * S) - 0.0009765625f * fmaxf(1.0f, fabsf(M));
  }
  return thr;
}

// keys: (p + 1) in the high word, ~idx in the low one: a larger key is a
// larger p, then a lower index; distinct (they hold the index); 0 = not a
// candidate / taken / empty
__device__ __forceinline__ unsigned long long pick_key(uint16_t p, unsigned idx) {
  return ((unsigned long long)(p + 1u) << 32) | (unsigned long long)(0xffffffffu - idx);
}
__device__ __forceinline__ unsigned key_id(unsigned long long key) {
  return 0xffffffffu - (unsigned)(key & 0xffffffffu);
}
__device__ __forceinline__ uint16_t key_p16(unsigned long long key) {
  return (uint16_t)((key >> 32) - 1u);
}

// The k best of the n <= kCand keys of the candidate list, by the first wave:
// emit(round, key) in lane 0, key 0 once the list is exhausted (a shard that
// holds fewer than k candidates; then nothing is cleared -- an empty lane's 0
// is not "taken").
template <typename Emit>
__device__ __forceinline__ void pick_from_list(const unsigned long long *cand, unsigned n, int k,
                                               int lane, int wv, Emit &&emit) {
  if (wv == 0) {
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
}

// Many candidates: k rounds of a workgroup-wide selection over the row x[0 ..
// V) in memory (global index = base + i); emit(round, key) in thread 0, key 0
// when the row holds fewer than k candidates.
template <int TPB, typename Emit>
__device__ __forceinline__ void pick_by_rounds(const uint16_t *x, int V, unsigned base, float M,
                                               float S, float thr, int k, int lane, int wv,
                                               unsigned long long *ksh, Emit &&emit) {
  const int tid = threadIdx.x;
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
      const unsigned long long key = pick_key(prob16(xv, M, S), base + (unsigned)i);
      best = key > best ? key : best;
    }
    const unsigned long long b = block_max_u64<TPB / 64>(best, lane, wv, ksh);
    __syncthreads();  // (ksh is rewritten in the next round)
    chosen[rd] = b ? (int)(key_id(b) - base) : -1;
    if (tid == 0) emit(rd, b);
  }
}

// The pick over a row in memory: candidates (x >= thr) to the LDS list, then
// one of the two selections.  *ncand is zero on entry (set before an earlier
// barrier).
template <int TPB, typename Emit>
__device__ __forceinline__ void pick_streamed(const uint16_t *x, int V, unsigned base, float M,
                                              float S, float thr, int k, int lane, int wv,
                                              unsigned long long *cand, unsigned *ncand,
                                              unsigned long long *ksh, Emit &&emit) {
  for (int i = threadIdx.x; i < V; i += TPB) {
    const float xv = h2f_(x[i]);
    if (xv >= thr) {
      const unsigned slot = atomicAdd(ncand, 1u);
      if (slot < (unsigned)kCand) cand[slot] = pick_key(prob16(xv, M, S), base + (unsigned)i);
    }
  }
  __syncthreads();
  const unsigned n = *ncand;
  if (n <= (unsigned)kCand) pick_from_list(cand, n, k, lane, wv, emit);
  else pick_by_rounds<TPB>(x, V, base, M, S, thr, k, lane, wv, ksh, emit);
}

// entry `at` of a top-k result
__device__ __forceinline__ void emit_topk(int32_t *ids, int32_t *ids2, float *probs, size_t at,
                                          unsigned long long key) {
  ids[at] = (int)key_id(key);
  if (ids2) ids2[at] = (int)key_id(key);
  if (probs) probs[at] = h2f_(key_p16(key));
}

// softmax (fp16 output, softmax.cu:262-288) + ArgMax (argmax.cu:62-100) /
// ArgTopK (arg_topk.cu:339-448), register-resident: one TPB-thread workgroup
// per row reads the row ONCE as 16-B vectors (NV per thread) and keeps it in
// registers; the rule above, the fallback rounds over the registers.
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
//    the oracle's serial loop): S = float(double sum) in any order.
//    `part` = [T][G] doubles, `cnt` = [T] counters, zero before the first
//    launch and left zero.
template <int TPB, int NV, int G>
__global__ __launch_bounds__(TPB) void softmax_topk_reg_kernel(
    const uint16_t *__restrict__ logits, int V, int k, int32_t *__restrict__ ids,
    float *__restrict__ probs, double *__restrict__ part, unsigned *__restrict__ cnt,
    int32_t *__restrict__ ids2) {
  constexpr int NW = TPB / 64;
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
  float wmax[NW];
  block_max_f32<NW>(mx, lane, wv, fsh, wmax);
  __syncthreads();  // (sh next holds the sums)
  const float M = max_of(wmax), L = kth_largest<NW>(wmax, k);  // (k <= 4 <= NW)
  double se = 0.0;
  if constexpr (E >= 8) {
#pragma unroll
    for (int v = 0; v < E / 8; ++v)
      if (gv(v) < nvec)
#pragma unroll
        for (int e = 0; e < 8; ++e) se += (double)exp_term(elem(v, e) - M);
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
        se += (double)exp_term(h2f_((uint16_t)(w & 0xffffu)) - M);
        se += (double)exp_term(h2f_((uint16_t)(w >> 16)) - M);
      }
  }
  // (block_sum_f64, written out: only wave 0 of a split workgroup uses the
  // sum, the compiler moves the waves' sums' LDS reads into that branch, and
  // behind any helper -- every shape tried -- it waited for them one by one
  // there: 4 more s_waitcnt and 0.02-0.03 us per launch at T <= 32)
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
  const float thr = cand_threshold(L, M, S);
  auto emit = [&](int rd, unsigned long long b) {
    emit_topk(ids, ids2, probs, (size_t)row * k + rd, b);
  };
#pragma unroll
  for (int v = 0; v < NV; ++v)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float xv = elem(v, e);
      const unsigned i = (unsigned)(gv(v) * 8 + e);
      if (xv >= thr && (int)i < V) {
        const unsigned slot = atomicAdd(&ncand, 1u);
        if (slot < (unsigned)kCand) cand[slot] = pick_key(prob16(xv, M, S), i);
      }
    }
  __syncthreads();
  const unsigned n = ncand;
  if (n <= (unsigned)kCand) {
    pick_from_list(cand, n, k, lane, wv, emit);
    return;
  }
  // many candidates: the k rounds over the registers, the owner of a round's
  // pick marking it taken
  for (int rd = 0; rd < k; ++rd) {
    unsigned long long best = 0;
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float xv = elem(v, e);
        const unsigned i = (unsigned)(gv(v) * 8 + e);
        if (xv >= thr && (int)i < V) {
          const unsigned long long key = pick_key(prob16(xv, M, S), i);
          best = key > best ? key : best;
        }
      }
    const unsigned long long b = block_max_u64<NW>(best, lane, wv, ksh);
    __syncthreads();  // (ksh is rewritten in the next round)
    const unsigned idx = key_id(b);
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

// The same for rows the register kernel does not take (a vocabulary not a
// multiple of 8, unaligned rows, V > 32768 such as LLaMA-3's 128256): three
// strided passes over the row (max and wave maxima, sum, candidates; the
// second and third hit L2), and the k rounds over the row only when more than
// kCand logits are candidates.
template <int TPB>
__global__ __launch_bounds__(TPB) void softmax_topk_kernel(
    const uint16_t *__restrict__ logits, int V, int k, int32_t *__restrict__ ids,
    float *__restrict__ probs, int32_t *__restrict__ ids2) {
  constexpr int NW = TPB / 64;
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
  float wmax[NW];
  block_max_f32<NW>(mx, lane, wv, fsh, wmax);
  __syncthreads();  // (sh next holds the sums)
  const float M = max_of(wmax), L = kth_largest<NW>(wmax, k);
  double se = 0.0;
  for (int i = tid; i < V; i += TPB) se += (double)exp_term(h2f_(x[i]) - M);
  const float S = (float)block_sum_f64<NW>(se, lane, wv, sh);
  const float thr = cand_threshold(L, M, S);
  auto emit = [&](int rd, unsigned long long b) {
    emit_topk(ids, ids2, probs, (size_t)row * k + rd, b);
  };
  pick_streamed<TPB>(x, V, 0u, M, S, thr, k, lane, wv, cand, &ncand, ksh, emit);
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
//  1. z (kept as fp16 in the row's workspace), the row maximum (temper_row);
//  2. S = float(double sum of expf_ref terms), as the top-k kernels';
//  3. every p_i: its key replaces z in the workspace and its integer mass goes
//     to an LDS histogram over the keys (key_mass_pass);
//  4. a workgroup scan from the top key down finds the key K at which the
//     cumulative mass reaches the target (topp_target), and from the mass
//     above K the rank r, in index order, of the pick among the tokens
//     holding K (rank_in_key);
//  5. the r-th token holding K (find_holder).
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

// t * 2^24 rounded up, t = (u * topp) * topp: the smallest integer mass that
// reaches t
__device__ __forceinline__ unsigned topp_target(float u, float topp) {
  const double t = __dmul_rn(__dmul_rn((double)u, (double)topp), (double)topp);
  const double tm = ceil(__dmul_rn(t, 16777216.0));
  return tm >= 1.0 ? (tm < 4.0e9 ? (unsigned)tm : 4000000000u) : 1u;
}

// z = half(x / half(temperature)) into the row's workspace w; the thread's
// maximum of z
template <int TPB>
__device__ __forceinline__ float temper_row(const uint16_t *x, uint16_t *w, int V,
                                            float temperature) {
  const float th = h2f_(f2h_(temperature));
  float mx = -INFINITY;
  for (int i = threadIdx.x; i < V; i += TPB) {
    const uint16_t z = f2h_(__fdiv_rn(h2f_(x[i]), th));
    w[i] = z;
    mx = fmaxf(mx, h2f_(z));
  }
  return mx;
}

// Every p_i: its key replaces z in w and its integer mass goes to the LDS
// histogram (LDS atomics: a softmax row spreads over thousands of keys, so few
// of them collide).  Returns the thread's last token of the order (lowest p,
// then highest index), for a row whose whole mass stays below the target: the
// largest (~key, index).
template <int TPB, bool HWEXP>
__device__ __forceinline__ unsigned long long key_mass_pass(uint16_t *w, int V, float M, float S,
                                                            unsigned *hist) {
  unsigned long long lastk = 0;
  for (int i = threadIdx.x; i < V; i += TPB) {
    const unsigned key = prob16<HWEXP>(h2f_(w[i]), M, S);
    w[i] = (uint16_t)key;
    // (a NaN row -- an infinite logit -- has keys outside the histogram: no mass)
    if (key < (unsigned)kSampleKeys && key) atomicAdd(&hist[key], p_mass(key));
    const unsigned long long lk = ((unsigned long long)(0xffffu - key) << 32) | (unsigned)i;
    lastk = lk > lastk ? lk : lastk;
  }
  return lastk;
}

// The 0-based rank, in index order among the tokens holding key K, of the
// token at which the cumulative mass reaches `need` more than the mass above K
__device__ __forceinline__ unsigned rank_in_key(unsigned need, unsigned K) {
  const unsigned pm = p_mass(K);
  return (need + pm - 1) / pm - 1;
}

// The rank-th token (0-based, index order) of w[0 .. V) holding key K: the
// tokens holding K are counted per 64 consecutive indices (one wave ballot
// each, the counts in `cnt` -- the histogram's LDS, (V / TPB + 1) * NW
// entries), a scan finds the group of that rank, and the wave that owns the
// group finds its lane.  Returns the index in the one thread that holds the
// token, -1 in every other.
template <int TPB>
__device__ __forceinline__ int find_holder(const uint16_t *w, int V, unsigned K, unsigned rank,
                                           unsigned *cnt, unsigned *wsum, int *res) {
  constexpr int NW = TPB / 64;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int nchunk = (V + TPB - 1) / TPB;
  for (int j = 0; j < nchunk; ++j) {
    const int i = j * TPB + tid;
    const unsigned long long b = __ballot(i < V && w[i] == (uint16_t)K);
    if (lane == 0) cnt[j * NW + wv] = (unsigned)__popcll(b);
  }
  __syncthreads();
  block_find<TPB, false>(cnt, nchunk * NW, rank + 1, wsum, res);
  const int g = res[0];
  if (g < 0 || g % NW != wv) return -1;
  const int i = (g / NW) * TPB + tid;
  const bool hit = i < V && w[i] == (uint16_t)K;
  const unsigned long long b = __ballot(hit);
  const unsigned below = (unsigned)__popcll(b & ((1ull << lane) - 1ull));
  return hit && below == rank - (unsigned)res[1] ? i : -1;
}

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
  for (int i = tid; i < kSampleKeys; i += TPB) hist[i] = 0;
  const float M = block_max_f32<NW>(temper_row<TPB>(x, w, V, temperature), lane, wv, fsh);
  __syncthreads();  // (sh next holds the sums)
  double se = 0.0;
  for (int i = tid; i < V; i += TPB) se += (double)exp_term<HWEXP>(h2f_(w[i]) - M);
  const float S = (float)block_sum_f64<NW>(se, lane, wv, sh);
  __syncthreads();  // (sh next holds the last-token keys)
  unsigned long long lastk =
      wave_max_u64_put(key_mass_pass<TPB, HWEXP>(w, V, M, S, hist), lane, wv, ksh);
  const unsigned target = topp_target(u[row], topp);
  __syncthreads();  // (the histogram and the waves' last-token keys are complete)
  lastk = wave_max_u64_get<NW>(ksh, lastk);
  block_find<TPB, true>(hist, kSampleKeys, target, wsum, res);
  const int kq = res[0];
  if (kq < 0) {  // (uniform: the whole workgroup leaves)
    if (tid == 0) {
      ids[row] = (int)(lastk & 0xffffffffu);
      if (probs) probs[row] = h2f_((uint16_t)(0xffffu - (unsigned)(lastk >> 32)));
    }
    return;
  }
  const unsigned K = (unsigned)(kSampleKeys - 1 - kq);
  const unsigned rank = rank_in_key(target - (unsigned)res[1], K);
  __syncthreads();  // (every thread has read res; hist becomes the group counts)
  const int i = find_holder<TPB>(w, V, K, rank, hist, wsum, res);
  if (i >= 0) {
    ids[row] = i;
    if (probs) probs[row] = h2f_((uint16_t)K);
  }
}

// one 16-bit word per logit; the histogram's LDS, reused for the counts of
// whole chunks of 64-index groups, bounds the row length
constexpr int kSampleMaxV = kSampleKeys / (kSampleTPB / 64) * kSampleTPB;
int sample_topp_max_v() { return kSampleMaxV; }
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
            const unsigned long long key = pick_key(f2h_(pv), (unsigned)iv);
            if (key > best) best = key, bq = q;
          }
        taken[rd] = bq;
        emit_topk(ids, nullptr, probs, (size_t)t * k + rd, best);
      }
    }
    return;
  }
  float *own = slot(rank);
  if (phase == 0) {
    float m = -INFINITY;
    for (int i = tid; i < Vl; i += TPB) m = fmaxf(m, h2f_(x[i]));
    m = block_max_f32<NW>(m, lane, wv, fsh);
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
    for (int i = tid; i < Vl; i += TPB) se += (double)exp_term(h2f_(x[i]) - M);
    se = block_sum_f64<NW>(se, lane, wv, dsh);
    if (tid < P * W) {
      const int r = tid / W, w = tid % W;
      const float hi = (float)se, lo = (float)(se - (double)hi);
      slot(r)[w] = r != rank ? 0.f : (w == 0 ? M : w == 1 ? hi : w == 2 ? lo : 0.f);
    }
    return;
  }
  // phase 2: global S from the phase-1 records, local top-k candidates (L
  // from the local wave maxima); a shard with fewer than k candidates sends
  // empty ones (p 0, id -1)
  double sd = 0.0;
  for (int r = 0; r < P; ++r) {
    const float *q = xch + ((size_t)r * T + t) * W;
    sd += (double)q[1] + (double)q[2];
  }
  const float S = (float)sd;
  if (tid == 0) ncand = 0;
  float wm = -INFINITY;
  for (int i = tid; i < Vl; i += TPB) wm = fmaxf(wm, h2f_(x[i]));
  float wmax[NW];
  block_max_f32<NW>(wm, lane, wv, fsh, wmax);  // (its barrier also: every thread has read the phase-1 records)
  const float thr = cand_threshold(kth_largest<NW>(wmax, k), M, S);
  auto emit = [&](int rd, unsigned long long b) {
    own[2 * rd] = b ? h2f_(key_p16(b)) : 0.f;
    own[2 * rd + 1] = b ? (float)key_id(b) : -1.f;
  };
  pick_streamed<TPB>(x, Vl, (unsigned)(rank * Vl), M, S, thr, k, lane, wv, cand, &ncand, ksh,
                     emit);
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
//   phase 4: the owner finds its (r - prefix)-th token holding K
//                                            -> exchange -> the global id
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
    const float M = block_max_f32<NW>(temper_row<TPB>(x, w, Vl, temperature), lane, wv, fsh);
    zero_slots(kVsUsed[0]);
    if (tid == 0) own[0] = M;
  } else if constexpr (PHASE == 1) {
    __shared__ double dsh[NW];
    float M = -INFINITY;
    for (int r = 0; r < P; ++r) M = fmaxf(M, rd(r)[0]);
    double se = 0.0;
    for (int i = tid; i < Vl; i += TPB) se += (double)exp_term(h2f_(w[i]) - M);
    se = block_sum_f64<NW>(se, lane, wv, dsh);  // (its barrier also: every thread has read the phase-0 records)
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
    unsigned long long lastk =
        wave_max_u64_put(key_mass_pass<TPB, false>(w, Vl, M, S, hist), lane, wv, ksh);
    __syncthreads();  // (the histogram and the waves' last-token keys are complete)
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
      lastk = wave_max_u64_get<NW>(ksh, lastk);
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
    const unsigned target = topp_target(u[t], topp);
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
        // among K's tokens in global index order
        const unsigned rk = rank_in_key(target - c - (unsigned)res[1], K);
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
    if (owner == rank) {  // (uniform; find_holder's barriers: after the zeroing)
      const int i = find_holder<TPB>(w, Vl, K, rloc, hist, wsum, res);
      if (i >= 0) vs_put(own, (unsigned)rank * (unsigned)Vl + (unsigned)i);
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

// ---------------------------------------------------------------------------
// Per-token log-probabilities (include/ffmi.h ffmi_token_logprobs): the log of
// the full softmax of z (the logits, or the row the top-p pick sees: z =
// half(x / half(temperature)), temper_row's expression) at one scored id,
//   lp = (z_s - M) - log(S),  M = max z,  S = sum exp(z - M)  in fp32.
// Nothing here is ranked or tied, so the hardware exp2 serves for the terms
// (the bar is 2^-16 + 2^-21 |lp|, ten times the fp32 rule's own error).
// A row's bits depend on the row alone: it is cut into chunks of kLogprobChunk
// logits whatever T is; one workgroup reduces one chunk to (m, s = sum exp(z -
// m)), every thread taking the same 16 elements in the same order and the
// waves' sums added in wave order; the second launch, one thread per row,
// takes M = max m_c and adds the s_c exp(m_c - M) in chunk order.  No atomics.
// T x ceil(V / 4096) workgroups of 256 threads: 64 at T = 8, V = 32000 (a
// decode step), 256 at V = 128256.
// ---------------------------------------------------------------------------
extern "C" __device__ float __ockl_wfred_add_f32(float);
constexpr int kLpTPB = 256;
constexpr int kLpVec = 8;                                    // logits per 16-byte load
constexpr int kLpLoads = kLogprobChunk / (kLpTPB * kLpVec);  // per thread
static_assert(kLpLoads * kLpTPB * kLpVec == kLogprobChunk, "a chunk is whole loads");

template <bool TEMPER>
__device__ __forceinline__ float lp_z(uint16_t x, float th) {
  return TEMPER ? h2f_(f2h_(__fdiv_rn(h2f_(x), th))) : h2f_(x);
}

// VEC: 16-byte loads (V % 8 == 0 and an aligned base: every group of 8 lies
// whole inside or outside the row); the element -> thread map and the order of
// the sums are the same in both forms, so their bits are
template <bool TEMPER, bool VEC>
__global__ __launch_bounds__(kLpTPB) void logprob_chunk_kernel(
    const uint16_t *__restrict__ logits, int V, int nchunk, float temperature,
    float2 *__restrict__ part) {
  constexpr int NW = kLpTPB / 64;
  __shared__ float shm[NW], shs[NW];
  const int row = blockIdx.x / nchunk, c = blockIdx.x % nchunk;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint16_t *x = logits + (size_t)row * V;
  const float th = TEMPER ? h2f_(f2h_(temperature)) : 0.f;
  float z[kLpLoads * kLpVec];
#pragma unroll
  for (int j = 0; j < kLpLoads; ++j) {
    // (c * kLogprobChunk < V <= 983040: no overflow)
    const int i0 = c * kLogprobChunk + (j * kLpTPB + tid) * kLpVec;
    if (VEC) {
      uint4 r = make_uint4(0xfc00fc00u, 0xfc00fc00u, 0xfc00fc00u, 0xfc00fc00u);  // -inf
      if (i0 < V) r = *reinterpret_cast<const uint4 *>(x + i0);
#pragma unroll
      for (int e = 0; e < kLpVec; ++e) {
        const uint32_t w = (&r.x)[e >> 1];
        const uint16_t hv = (uint16_t)((e & 1) ? w >> 16 : w & 0xffffu);
        z[j * kLpVec + e] = i0 < V ? lp_z<TEMPER>(hv, th) : -INFINITY;
      }
    } else {
#pragma unroll
      for (int e = 0; e < kLpVec; ++e)
        z[j * kLpVec + e] = i0 + e < V ? lp_z<TEMPER>(x[i0 + e], th) : -INFINITY;
    }
  }
  float m = z[0];
#pragma unroll
  for (int e = 1; e < kLpLoads * kLpVec; ++e) m = fmaxf(m, z[e]);
  m = __ockl_wfred_max_f32(m);
  if (lane == 0) shm[wv] = m;
  __syncthreads();
  m = shm[0];
#pragma unroll
  for (int q = 1; q < NW; ++q) m = fmaxf(m, shm[q]);
  // (a chunk of -inf logits only: s = 0, and the combine gives it no weight)
  const float mm = m == -INFINITY ? 0.f : m;
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < kLpLoads * kLpVec; ++e) s += __expf(z[e] - mm);
  s = __ockl_wfred_add_f32(s);
  if (lane == 0) shs[wv] = s;
  __syncthreads();
  if (tid == 0) {
    float t = shs[0];
#pragma unroll
    for (int q = 1; q < NW; ++q) t += shs[q];
    part[blockIdx.x] = make_float2(m, t);
  }
}

template <bool TEMPER>
__global__ __launch_bounds__(64) void logprob_combine_kernel(
    const uint16_t *__restrict__ logits, int T, int V, int nchunk, float temperature,
    const int32_t *__restrict__ targets, const int32_t *__restrict__ picks,
    const float2 *__restrict__ part, float *__restrict__ logprobs) {
  const int row = blockIdx.x * 64 + threadIdx.x;
  if (row >= T) return;
  int id = targets ? targets[row] : -1;
  if (id < 0 && picks) id = picks[row];
  if (id < 0 || id >= V) {  // (outside the contract: no logit is read)
    logprobs[row] = __uint_as_float(0x7fc00000u);
    return;
  }
  const float2 *p = part + (size_t)row * nchunk;
  float M = p[0].x;
  for (int c = 1; c < nchunk; ++c) M = fmaxf(M, p[c].x);
  float S = 0.f;
  for (int c = 0; c < nchunk; ++c) S += p[c].y * expf(p[c].x - M);
  const float th = TEMPER ? h2f_(f2h_(temperature)) : 0.f;
  const float zs = lp_z<TEMPER>(logits[(size_t)row * V + id], th);
  logprobs[row] = (zs - M) - logf(S);
}

static int logprob_chunks(int V) { return (V + kLogprobChunk - 1) / kLogprobChunk; }
size_t token_logprobs_workspace_bytes(int T, int V) {
  return T <= 0 || V <= 0 ? 0 : (size_t)T * logprob_chunks(V) * sizeof(float2);
}

hipError_t launch_token_logprobs(const uint16_t *logits, int T, int V, float temperature,
                                 const int32_t *targets, const int32_t *picks, float *logprobs,
                                 void *ws, hipStream_t s) {
  if (T <= 0) return hipSuccess;
  const int nchunk = logprob_chunks(V);
  if (V < 1 || V > kSampleMaxV || !ws || !(temperature >= 0.f) ||
      (size_t)T * nchunk > (size_t)INT32_MAX)
    return hipErrorInvalidValue;
  float2 *part = reinterpret_cast<float2 *>(ws);
  const bool vec = V % kLpVec == 0 && ((uintptr_t)logits & 15) == 0;
  const dim3 g1((unsigned)(T * nchunk)), g2((unsigned)((T + 63) / 64));
#define FFMI_LP(TEMPER)                                                                          \
  do {                                                                                           \
    if (vec)                                                                                     \
      hipLaunchKernelGGL((logprob_chunk_kernel<TEMPER, true>), g1, dim3(kLpTPB), 0, s, logits,  \
                         V, nchunk, temperature, part);                                          \
    else                                                                                         \
      hipLaunchKernelGGL((logprob_chunk_kernel<TEMPER, false>), g1, dim3(kLpTPB), 0, s, logits, \
                         V, nchunk, temperature, part);                                          \
    hipLaunchKernelGGL((logprob_combine_kernel<TEMPER>), g2, dim3(64), 0, s, logits, T, V,      \
                       nchunk, temperature, targets, picks, part, logprobs);                     \
  } while (0)
  if (temperature > 0.f) FFMI_LP(true);
  else FFMI_LP(false);
#undef FFMI_LP
  return hipGetLastError();
}

}  // namespace ffmi
