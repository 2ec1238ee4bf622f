// attention_fp8.hip -- the attention of an FFMI_ATTN_KV_FP8 handle: the
// two-launch scheme of attention.hip (kv_update_fp8_kernel there stores the
// step's K/V; this kernel attends) over byte caches
//   K8[req][kv head][slot][d]   and   V8T[req][kv head][d][slot],
// one OCP e4m3fn byte per element, value = scale * e4m3(byte) with one static
// scale per cache (attention_util.h has the quantiser).
//
// Work decomposition, softmax, P as an fp16 hi/lo pair and the LDS merge are
// attention_kernel<.., FUSED = false>'s: one workgroup per (item of <= 16 QT
// queries, query head), 8 waves striding over 32-key chunks, the f16
// v_mfma_f32_16x16x32_f16 for both products.  New is the operand path:
//  * e4m3 -> f16 is exact, so the bytes are widened in registers
//    (v_cvt_scalef32_pk_f16_fp8 at scale 1) and k_scale / v_scale never touch
//    an operand: k_scale is folded into the qk scale on the host, v_scale
//    into the final 1 / (sum + 1e-6) of each query.
//  * S^T = K . Q^T does not care how d is dealt to the k-steps as long as K
//    and Q agree.  Lane (row, g) takes the CONTIGUOUS bytes [g D/4, (g+1) D/4)
//    of its K row -- 16-B loads, each feeding two k-steps (8 bytes = one
//    8-half fragment each) -- and k-step ks of the Q fragment is read at
//    d = g D/4 + 8 ks instead of 32 ks + 8 g.  A chunk's K loads are half the
//    fp16 kernel's in count and bytes.
//  * the V8T side is fixed by the S^T accumulator's key permutation (slots
//    base + 4 g + r and base + 16 + 4 g + r): two dword loads per d-tile.
//  * QT == 1 (decode, beam steps): the raw bytes of a wave's next chunk -- half
//    the registers the fp16 fragments would take -- are loaded before the
//    current chunk's products, so a wave overlaps its own loads too.
// Past kv_len the V8T bytes of the last chunk enter as zeros (byte masks);
// e4m3fn has no infinity, and the quantiser never writes its NaN byte, so a
// masked key below kv_len multiplies a finite V by an exact zero.
#include "attention_util.h"

// (FFMI_NO_PK_F32 for every function of this file, the kernel's lambdas
// included: a lambda without the kernel's target features is not inlined)
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(FFMI_NO_PK_F32, apply_to = function)
#endif

namespace ffmi {

typedef _Float16 h2v __attribute__((ext_vector_type(2)));

// eight e4m3 bytes (a: elements 0-3, b: 4-7) -> an MFMA f16 fragment
__device__ __forceinline__ h8 widen8(uint32_t a, uint32_t b) {
  const h2v p0 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)a, 1.0f, false);
  const h2v p1 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)a, 1.0f, true);
  const h2v p2 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)b, 1.0f, false);
  const h2v p3 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)b, 1.0f, true);
  return h8{p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], p3[0], p3[1]};
}

// GQ: query head h reads K/V head h / (heads / kvh_) (the kv-indexed form)
template <int D, int QT, int NW, bool GQ>
__global__ __launch_bounds__(64 * NW, 1) void attention_fp8_kernel(
    const char *__restrict__ blob, const uint16_t *__restrict__ qbuf,
    const uint8_t *__restrict__ kc, const uint8_t *__restrict__ vc, uint16_t *__restrict__ out,
    int heads, int kvh_, int slots, float qk_scale, float v_scale, int out_packed) {
  constexpr int KS = D / 32;  // k-steps of the QK^T product
  constexpr int KL = D / 64;  // 16-B loads of a lane's quarter of a K row
  constexpr int DT = D / 16;  // d-tiles of the PV product
  constexpr int NQ = 16 * QT;
  constexpr bool PF = QT == 1;  // prefetch the wave's next chunk
  __shared__ float sm_m[NW][NQ];
  __shared__ float sm_l[NW][NQ];
  __shared__ __attribute__((aligned(16))) float sm_o[NW][QT][DT][4][64];

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int qi = lane & 15;
  const int g = lane >> 4;
  const int kvh = GQ ? kvh_ : heads;
  const int h = blockIdx.y, hk = GQ ? h / (heads / kvh_) : h;
  const BatchView bv = batch_view(blob);
  const ffmi_attn_work w = bv.work[blockIdx.x].w;
  const int Hl = heads * D;
  const uint8_t *kbase = kc + ((size_t)w.req * kvh + hk) * slots * D;
  const uint8_t *vbase = vc + ((size_t)w.req * kvh + hk) * D * slots;

  struct Raw {  // a lane's bytes of one 32-key chunk
    uint4 k[2][KL];
    uint32_t v[DT][2];
  };
  // (chunk indices stay below ceil(kv_len / 32): the cache is allocated to a
  // multiple of 32 slots)
  auto load_raw = [&](int c, Raw &r) {
    const int base = c * 32;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      const uint8_t *krow = kbase + (size_t)(base + sub * 16 + qi) * D + g * (D / 4);
#pragma unroll
      for (int l = 0; l < KL; ++l) r.k[sub][l] = *reinterpret_cast<const uint4 *>(krow + 16 * l);
    }
#pragma unroll
    for (int t = 0; t < DT; ++t) {
      const uint8_t *vrow = vbase + (size_t)(t * 16 + qi) * slots + base + 4 * g;
      r.v[t][0] = *reinterpret_cast<const uint32_t *>(vrow);
      r.v[t][1] = *reinterpret_cast<const uint32_t *>(vrow + 16);
    }
  };
  // bytes -> fragments; the V8T bytes of slots >= kv_len as zeros first (a
  // lane holds slots base + 4 g + r and base + 16 + 4 g + r of every d-tile)
  auto widen = [&](int base, const Raw &r, h8 (&kf)[2][KS], h8 (&va)[DT]) {
    auto below = [](int n) {  // mask of a dword's n lowest bytes
      return n >= 4 ? 0xffffffffu : n <= 0 ? 0u : (1u << (8 * n)) - 1u;
    };
    const int n0 = w.kv_len - (base + 4 * g);
    const uint32_t m0 = below(n0), m1 = below(n0 - 16);
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
      for (int l = 0; l < KL; ++l) {
        kf[sub][2 * l] = widen8(r.k[sub][l].x, r.k[sub][l].y);
        kf[sub][2 * l + 1] = widen8(r.k[sub][l].z, r.k[sub][l].w);
      }
#pragma unroll
    for (int t = 0; t < DT; ++t) va[t] = widen8(r.v[t][0] & m0, r.v[t][1] & m1);
  };

  bool qvalid[QT];
  int pre[QT], tb[QT], tlen[QT];
  uint64_t tv[QT];
  h8 qf[QT][KS];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const int q = qt * 16 + qi;
    qvalid[qt] = q < w.q_count;
    const ffmi_token_info ti = bv.tokens[w.q_start + (qvalid[qt] ? q : 0)];
    pre[qt] = ti.prefix_len, tb[qt] = ti.tree_base, tlen[qt] = ti.tree_len, tv[qt] = ti.tree_vis;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)  // (K's permutation of d: see the head of the file)
      qf[qt][ks] = !qvalid[qt] ? h8{0, 0, 0, 0, 0, 0, 0, 0}
                               : *reinterpret_cast<const h8 *>(
                                     qbuf + (size_t)(w.q_start + q) * Hl + h * D + g * (D / 4) + 8 * ks);
  }

  const float NEG = -INFINITY;
  float m_run[QT], l_run[QT];
  f4 o[QT][DT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    m_run[qt] = NEG, l_run[qt] = 0.f;
#pragma unroll
    for (int t = 0; t < DT; ++t) o[qt][t] = f4{0.f, 0.f, 0.f, 0.f};
  }

  auto compute_chunk = [&](int base, const h8 (&kf)[2][KS], const h8 (&va)[DT]) {
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
      // S^T = K . Q^T: this lane holds query qt*16+qi, keys base + 16 sub + 4 g + r
      f4 s[2];
#pragma unroll
      for (int sub = 0; sub < 2; ++sub) {
        s[sub] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
          s[sub] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[sub][ks], qf[qt][ks], s[sub], 0, 0, 0);
      }
      float sc[8];
      bool vis[8];
      float cmax = NEG;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int slot = base + (j >> 2) * 16 + 4 * g + (j & 3);
        vis[j] = qvalid[qt] && slot < w.kv_len &&
                 key_visible(slot, pre[qt], tb[qt], tlen[qt], tv[qt]);
        sc[j] = __fmul_rn(qk_scale, s[j >> 2][j & 3]);
        cmax = vis[j] ? fmaxf(cmax, sc[j]) : cmax;
      }
      cmax = fmaxf(cmax, __shfl_xor(cmax, 16));
      cmax = fmaxf(cmax, __shfl_xor(cmax, 32));
      const float m_new = fmaxf(m_run[qt], cmax);
      const float m_use = (m_new == NEG) ? 0.f : m_new;
      const float alpha = (m_run[qt] == NEG) ? 0.f : __expf(m_run[qt] - m_use);
      h8 phi, plo;
      float psum = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float e = vis[j] ? __expf(sc[j] - m_use) : 0.f;
        psum += e;
        const _Float16 hi = (_Float16)e;
        phi[j] = hi;
        plo[j] = (_Float16)(e - (float)hi);
      }
      l_run[qt] = l_run[qt] * alpha + psum;
      m_run[qt] = m_new;
#pragma unroll
      for (int t = 0; t < DT; ++t) {
        o[qt][t] *= alpha;
        o[qt][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(va[t], phi, o[qt][t], 0, 0, 0);
        o[qt][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(va[t], plo, o[qt][t], 0, 0, 0);
      }
    }
  };

  // wave w takes chunks w, w + NW, ...
  const int nchunks = (w.kv_len + 31) >> 5;
  Raw cur;
  if (PF && wave < nchunks) load_raw(wave, cur);
  for (int c = wave; c < nchunks; c += NW) {
    h8 kf[2][KS], va[DT];
    if (PF) {
      Raw nxt;
      const bool more = c + NW < nchunks;  // (wave-uniform)
      if (more) load_raw(c + NW, nxt);
      widen(c * 32, cur, kf, va);
      compute_chunk(c * 32, kf, va);
      if (more) cur = nxt;
    } else {
      load_raw(c, cur);
      widen(c * 32, cur, kf, va);
      compute_chunk(c * 32, kf, va);
    }
  }

  // per-query partial sum over the 4 lane groups (same m_run in all four)
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    float l = l_run[qt];
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
    if (g == 0) {
      sm_m[wave][qt * 16 + qi] = m_run[qt];
      sm_l[wave][qt * 16 + qi] = l;
    }
#pragma unroll
    for (int t = 0; t < DT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) sm_o[wave][qt][t][r][lane] = o[qt][t][r];
  }
  __syncthreads();

  // merge: wave w finalizes d-tiles t = w, w + NW, ... of every query tile
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const int ql = qt * 16 + qi;
    float M = NEG;
#pragma unroll
    for (int ww = 0; ww < NW; ++ww) M = fmaxf(M, sm_m[ww][ql]);
    float f[NW], L = 0.f;
#pragma unroll
    for (int ww = 0; ww < NW; ++ww) {
      const float mw = sm_m[ww][ql];
      f[ww] = (mw == NEG) ? 0.f : __expf(mw - M);
      L += f[ww] * sm_l[ww][ql];
    }
    const float inv = 1.0f / (L + 1e-6f);
    if (!qvalid[qt]) continue;
    const int orow_m = w.q_start + ql;
    uint16_t *orow = out + (size_t)orow_m * Hl + h * D;
    for (int t = wave; t < DT; t += NW) {
      uint16_t r4[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float acc = 0.f;
#pragma unroll
        for (int ww = 0; ww < NW; ++ww) acc += f[ww] * sm_o[ww][qt][t][r][lane];
        r4[r] = f2h(acc * inv * v_scale);
      }
      uint2 pk;
      pk.x = r4[0] | ((uint32_t)r4[1] << 16);
      pk.y = r4[2] | ((uint32_t)r4[3] << 16);
      uint16_t *dst = out_packed ? out + act_packed_off(orow_m, h * D + t * 16 + 4 * g, Hl)
                                 : orow + t * 16 + 4 * g;
      *reinterpret_cast<uint2 *>(dst) = pk;
    }
  }
}

// The step's K/V must already be in the byte caches (launch_kv_update_fp8).
hipError_t launch_attention_fp8(const char *blob, int W, int max_q, const uint16_t *qbuf,
                                const uint8_t *kc, const uint8_t *vc, uint16_t *out, int heads,
                                int d, int slots, float scale, float k_scale, float v_scale,
                                bool out_packed, int kv_heads, hipStream_t s) {
  if (W <= 0) return hipSuccess;
  if (out_packed && (heads * d) % 32) return hipErrorInvalidValue;
  if (max_q > FFMI_ATTN_QTILE || (d != 128 && d != 64)) return hipErrorInvalidValue;
  const bool gqa = kv_heads > 0 && kv_heads != heads;
  if (gqa && heads % kv_heads) return hipErrorInvalidValue;
  const dim3 grid(W, heads);
  const float qk = scale * k_scale;  // k_scale folded in once per launch
  const int op = out_packed ? 1 : 0, kvh = gqa ? kv_heads : heads;
#define FFMI_ATT8(D, QT, GQ)                                                                  \
  hipLaunchKernelGGL((attention_fp8_kernel<D, QT, 8, GQ>), grid, dim3(512), 0, s, blob, qbuf, \
                     kc, vc, out, heads, kvh, slots, qk, v_scale, op)
#define FFMI_ATT8_D(D)                    \
  do {                                    \
    if (max_q <= 16 && gqa) FFMI_ATT8(D, 1, true);   \
    else if (max_q <= 16) FFMI_ATT8(D, 1, false);    \
    else if (gqa) FFMI_ATT8(D, 2, true);             \
    else FFMI_ATT8(D, 2, false);                     \
  } while (0)
  if (d == 128) FFMI_ATT8_D(128);
  else FFMI_ATT8_D(64);
#undef FFMI_ATT8_D
#undef FFMI_ATT8
  return hipGetLastError();
}

}  // namespace ffmi

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
