// gemm_w8a8.hip -- W8A8 linear layers: fp8 (e4m3) weights against fp8
// activations with one dynamic scale per token, on the native fp8 matrix
// instruction (v_mfma_f32_16x16x32_fp8_fp8, fp32 accumulate).
//
//   Y[t][n] = a[t] * s[n] * sum_k x8[t][k] * q[n][k]
// q / s: the packed weights of gemm_w8.hip, unchanged.  x8 / a: the row
// quantiser below (or the quantising RMSNorm of norm.hip, bit for bit the
// same): a[t] = absmax of row t / 448 (fp32 division; 1 for an all-zero row),
// x8 the e4m3 byte of x / a[t] by kv8_quant4's rule.  Inf / NaN in the fp16
// input is outside the contract.  X8 keeps, within every 64-column block of a
// row, the weight layout's order (gemm_w8.h: chunk c at byte 16 (c & 3) + 8
// (c >> 2)), so both operands of a double step are one 16-byte piece per lane
// and neither is ever converted: the lane's low 8 bytes feed the first MFMA,
// the high 8 the second.  Products of two e4m3 values are exact in fp32.
//
// The GEMM, one kernel family for 1 .. 256 rows per weight pass:
//  * a workgroup is 4 waves that split the ROWS: wave w owns m-tiles w * MTW ..
//    w * MTW + MTW - 1 (MTW = 1 .. 4) and all four share the kA8NTW = 8 weight
//    tiles of column group blockIdx.x; gridDim.y = S splits K by plan_w8, a
//    function of (N, K, epilogue) only;
//  * weights go HBM -> registers -> LDS as BYTES: wave w loads the 1 KiB double
//    blocks of tiles w and w + 4 (16 bytes per lane, non-temporal under
//    FFMI_W_STREAM) through a register ring PF double steps deep and stores
//    them as they are into a double-buffered LDS tile [2][8][64] of 16-byte
//    pieces (16 KiB; the widened f16 tile of gemm_w8_mid.hip is 32 KiB and
//    costs four conversions per 8 bytes).  Every wave reads all 8 pieces of a
//    step with 16-byte LDS reads: a weight byte crosses the CU's L1 once, not
//    once per wave;
//  * activations never touch LDS: lane l loads the 16-byte piece 16 (l >> 4)
//    of row (l & 15) of each of its m-tiles straight from X8 into the same
//    ring (loads retire in order: X is issued as early as the weights it
//    meets).  Rows >= T are never read: a whole m-tile past T is zeros by a
//    wave-uniform predicate, a wave that owns no row at all skips its MFMAs
//    (at T <= 16 three waves only move weights), a row past T inside a live
//    tile re-reads row T - 1, and none of them is stored (D = W . X^T: an X
//    row reaches only its own outputs);
//  * one barrier per double step: step k's MFMAs read LDS buffer k & 1 while
//    step k + 1's pieces are written to the other.
// Per output element: the double steps of the slice in sequence, two MFMAs
// each (low half, then high), then (acc * s[n]) * a[t], then the direct
// epilogue or the [S][T][NP] slabs for launch_partials_reduce (slices 0 .. S-1
// in order).  None of it depends on T, on MTW, on the ring or on the
// neighbours, so a row's bits are a function of the row, N, K and the epilogue.
#include <algorithm>

#include "gemm_w8.h"

namespace ffmi {

// ---------------------------------------------------------------------------
// Row quantiser: one 256-thread workgroup per row, the row in registers
// between the absmax reduction and the conversion (norm.hip's row kernels).
// ---------------------------------------------------------------------------
template <int MAXC>
__global__ __launch_bounds__(256) void quantize_rows_kernel(const uint16_t *__restrict__ X,
                                                            uint8_t *__restrict__ X8,
                                                            float *__restrict__ row_scales, int K) {
  __shared__ uint32_t scratch[4];
  const size_t row = blockIdx.x;
  const int nchunk = K >> 3;
  uint4 v[MAXC];
#pragma unroll
  for (int c = 0; c < MAXC; ++c)  // (clamped: no branch ahead of the loads)
    v[c] = *reinterpret_cast<const uint4 *>(X + row * K + min((int)threadIdx.x + c * 256, nchunk - 1) * 8);
  uint32_t m = 0;
#pragma unroll
  for (int c = 0; c < MAXC; ++c)
    if ((int)threadIdx.x + c * 256 < nchunk) m = a8_absmax8(v[c], m);
  const float a = a8_row_scale<4>(m, scratch);
  if (threadIdx.x == 0) row_scales[row] = a;
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    const int ch = threadIdx.x + c * 256;
    if (ch < nchunk) a8_store8(X8, row, K, ch, v[c], a);
  }
}

hipError_t launch_quantize_rows_fp8(const uint16_t *X, int T, int K, uint8_t *X8, float *row_scales,
                                    hipStream_t s) {
  if (T <= 0) return hipSuccess;
  if (K <= 0 || K % 64 || K > 256 * 8 * 16) return hipErrorInvalidValue;
  const int per = (K / 8 + 255) / 256;
#define FFMI_QR(MC) \
  hipLaunchKernelGGL((quantize_rows_kernel<MC>), dim3(T), dim3(256), 0, s, X, X8, row_scales, K)
  if (per <= 1) FFMI_QR(1);
  else if (per <= 2) FFMI_QR(2);
  else if (per <= 4) FFMI_QR(4);
  else if (per <= 8) FFMI_QR(8);
  else FFMI_QR(16);
#undef FFMI_QR
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// The GEMM.  T <= 4 * MTW * 16 rows; X8 [T][K] bytes in block order, a [T];
// W8 / scales / pitch and the EPI 1 tile pairing as gemm_w8_kernel's.
// ---------------------------------------------------------------------------
typedef long a8frag;  // eight e4m3 bytes: one operand of the fp8 MFMA

template <int MTW, int PF, int EPI, bool NTL>
__global__ __launch_bounds__(256) void gemm_w8a8_kernel(
    const uint8_t *__restrict__ X8, const float *__restrict__ row_scales,
    const uint8_t *__restrict__ W8, const float *__restrict__ scales, uint16_t *__restrict__ Y,
    float *__restrict__ Ypart, int T, int N, int K, int KT2, int NTILES, int pitch) {
  constexpr int NTW = kA8NTW, WL = NTW / 4;  // WL: tiles a wave loads
  __shared__ __attribute__((aligned(16))) u4v sW[2][NTW][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ks = blockIdx.y, S = gridDim.y;
  const int tile0 = blockIdx.x * NTW, row0 = wave * (MTW * 16);
  const int per = (KT2 + S - 1) / S;
  const int kb = min(KT2, ks * per), ke = min(KT2, kb + per);  // (workgroup-uniform)

  const uint8_t *wsrc[WL];
#pragma unroll
  for (int q = 0; q < WL; ++q)  // (a tile past the last re-reads it and is not stored)
    wsrc[q] = W8 + (size_t)min(tile0 + wave + 4 * q, NTILES - 1) * 1024 + lane * 16;
  const size_t wks = (size_t)pitch * 1024;
  const uint8_t *xsrc[MTW];
  bool xok[MTW];  // (wave-uniform)
#pragma unroll
  for (int i = 0; i < MTW; ++i) {
    xok[i] = row0 + i * 16 < T;
    xsrc[i] = X8 + (size_t)min(row0 + i * 16 + (lane & 15), T - 1) * K + 16 * (lane >> 4);
  }

  f4 acc[MTW][NTW];
#pragma unroll
  for (int i = 0; i < MTW; ++i)
#pragma unroll
    for (int j = 0; j < NTW; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};

  if (kb < ke) {
    // A PF-deep register ring holds both operands of double steps k..k+PF-1
    u4v wq[PF][WL], xq[PF][MTW];
    const u4v zero = {0, 0, 0, 0};
    auto load = [&](int Q, int kq) {
#pragma unroll
      for (int q = 0; q < WL; ++q) wq[Q][q] = ld_w8<NTL>(wsrc[q] + (size_t)kq * wks);
#pragma unroll
      for (int i = 0; i < MTW; ++i)
        xq[Q][i] = xok[i] ? *reinterpret_cast<const u4v *>(xsrc[i] + (size_t)kq * 64) : zero;
    };
    auto stage = [&](int Q, int buf) {  // this wave's tiles of one step, as they are
#pragma unroll
      for (int q = 0; q < WL; ++q) sW[buf][wave + 4 * q][lane] = wq[Q][q];
    };
#pragma unroll
    for (int Q = 0; Q < PF; ++Q) load(Q, min(kb + Q, ke - 1));
    stage(0, 0);
    __syncthreads();
    int cur = 0;
    // one double step on ring slot Q: the MFMAs read the slot's X in place and
    // the step's pieces from LDS, then the slot is refilled PF steps ahead and
    // the NEXT step's pieces go to the other LDS tile
    auto step = [&](int Q, int kt) {
      if (xok[0]) {  // (a wave without rows only moves weights)
#pragma unroll
        for (int j = 0; j < NTW; ++j) {
          const u4v b = sW[cur][j][lane];
          const a8frag b0 = (a8frag)(b.x | ((uint64_t)b.y << 32));
          const a8frag b1 = (a8frag)(b.z | ((uint64_t)b.w << 32));
#pragma unroll
          for (int i = 0; i < MTW; ++i) {  // D = W . X^T
            const a8frag x0 = (a8frag)(xq[Q][i].x | ((uint64_t)xq[Q][i].y << 32));
            const a8frag x1 = (a8frag)(xq[Q][i].z | ((uint64_t)xq[Q][i].w << 32));
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(b0, x0, acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(b1, x1, acc[i][j], 0, 0, 0);
          }
        }
      }
      load(Q, min(kt + PF, ke - 1));
      stage((Q + 1) % PF, cur ^ 1);
      __syncthreads();
      cur ^= 1;
    };
    int kt0 = kb;
    for (; kt0 + PF <= ke; kt0 += PF) {  // steady state: whole ring turns
#pragma unroll
      for (int Q = 0; Q < PF; ++Q) step(Q, kt0 + Q);
    }
#pragma unroll
    for (int Q = 0; Q < PF - 1; ++Q)  // tail: < PF steps, slots 0..
      if (kt0 + Q < ke) step(Q, kt0 + Q);
  }

  // Epilogue.  D layout: row m = row0 + i*16 + (lane & 15), columns n = tile*16
  // + (lane >> 4)*4 + r.  (acc * s[n]) * a[t], in that order.
  const int mr = row0 + (lane & 15), nq = (lane >> 4) * 4;
  const int NP = NTILES * 16;
  float am[MTW];
#pragma unroll
  for (int i = 0; i < MTW; ++i) am[i] = row_scales[min(i * 16 + mr, T - 1)];
#pragma unroll
  for (int j = 0; j < NTW; ++j) {
    if (tile0 + j >= NTILES) continue;
    const f4 sc = *reinterpret_cast<const f4 *>(scales + (size_t)(tile0 + j) * 16 + nq);
#pragma unroll
    for (int i = 0; i < MTW; ++i) {
      acc[i][j] *= sc;
      acc[i][j] *= am[i];
    }
  }
  if (S > 1) {  // EPI == 0 only
#pragma unroll
    for (int j = 0; j < NTW; ++j) {
      const int tile = tile0 + j;
      if (tile >= NTILES) continue;
#pragma unroll
      for (int i = 0; i < MTW; ++i) {
        const int m = i * 16 + mr;
        if (m < T)
          *reinterpret_cast<f4 *>(Ypart + ((size_t)ks * T + m) * NP + tile * 16 + nq) = acc[i][j];
      }
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < NTW; j += (EPI ? 2 : 1)) {
    const int tile = tile0 + j;
    if (tile >= NTILES) continue;
    const int n = (EPI ? (tile >> 1) : tile) * 16 + nq;
    if (n >= N) continue;
#pragma unroll
    for (int i = 0; i < MTW; ++i) {
      const int m = i * 16 + mr;
      if (m >= T) continue;
      uint16_t o[4];
#pragma unroll
      for (int r = 0; r < 4; ++r)
        o[r] = EPI ? silu_mul_h(acc[i][j][r], acc[i][j + (EPI ? 1 : 0)][r]) : f2h(acc[i][j][r]);
      uint16_t *dst = Y + (size_t)m * N + n;
      if (n + 4 <= N && (((uintptr_t)dst & 7) == 0)) {
        *reinterpret_cast<uint2 *>(dst) =
            make_uint2(o[0] | ((uint32_t)o[1] << 16), o[2] | ((uint32_t)o[3] << 16));
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (n + r < N) dst[r] = o[r];
      }
    }
  }
}

// the one-pass size is the requirement: there is no multi-pass route to keep
size_t gemm_w8a8_workspace_bytes(int T, int N, int K, int epilogue) {
  if (T <= 0 || N <= 0 || K <= 0 || K % 64) return 0;
  const W8Plan p = plan_w8(N, K, epilogue);
  return p.S > 1 ? (size_t)p.S * std::min(T, kA8Rows) * p.ntiles * 16 * sizeof(float) : 0;
}

// ring depth: the narrow forms keep as many weight bytes in flight per wave as
// the skinny W8A16 kernel (2 tiles x 6 KiB); the wide ones have the registers
// for 4 steps of both operands
template <int MTW>
static void launch_a8_mtw(const W8Plan &p, bool silu, bool ntl, const uint8_t *X8, const float *a,
                          const uint8_t *W8, const float *scales, uint16_t *Y, float *ws, int T,
                          int N, int K, hipStream_t s) {
  constexpr int PF = MTW <= 2 ? 6 : 4;
  const dim3 grid(p.nblk, p.S), block(256);
#define FFMI_A8(EPI, NTL)                                                                         \
  hipLaunchKernelGGL((gemm_w8a8_kernel<MTW, PF, EPI, NTL>), grid, block, 0, s, X8, a, W8, scales, \
                     Y, ws, T, N, K, p.KT2, p.ntiles, p.ntiles)
  if (silu && ntl) FFMI_A8(1, true);
  else if (silu) FFMI_A8(1, false);
  else if (ntl) FFMI_A8(0, true);
  else FFMI_A8(0, false);
#undef FFMI_A8
}

// One launch per kA8Rows rows, MTW = m-tiles of the pass over the 4 waves
hipError_t launch_gemm_w8a8(const uint8_t *X8, const float *row_scales, const uint8_t *W8,
                            const float *scales, uint16_t *Y, float *ws, size_t ws_bytes, int T,
                            int N, int K, int epilogue, hipStream_t s) {
  if (T <= 0) return hipSuccess;
  if (N <= 0 || K <= 0 || K % 64 || (epilogue & (FFMI_X_PACKED | FFMI_Y_PACKED)))
    return hipErrorInvalidValue;
  const int base = epilogue & ~FFMI_W_STREAM;
  if (base != FFMI_EPI_NONE && base != FFMI_EPI_SILU_MUL) return hipErrorInvalidValue;
  static_assert(kA8NTW == 4 * kW8NT, "plan_w8's column group is the workgroup's");
  const W8Plan p = plan_w8(N, K, epilogue);
  if (p.S > 1 && (!ws || ws_bytes < gemm_w8a8_workspace_bytes(T, N, K, epilogue)))
    return hipErrorInvalidValue;
  const bool silu = base == FFMI_EPI_SILU_MUL, ntl = (epilogue & FFMI_W_STREAM) != 0;
  for (int t0 = 0; t0 < T; t0 += kA8Rows) {
    const int Tp = std::min(kA8Rows, T - t0);
    const uint8_t *Xp = X8 + (size_t)t0 * K;
    const float *ap = row_scales + t0;
    uint16_t *Yp = Y + (size_t)t0 * N;
    switch (((Tp + 15) / 16 + 3) / 4) {
      case 1: launch_a8_mtw<1>(p, silu, ntl, Xp, ap, W8, scales, Yp, ws, Tp, N, K, s); break;
      case 2: launch_a8_mtw<2>(p, silu, ntl, Xp, ap, W8, scales, Yp, ws, Tp, N, K, s); break;
      case 3: launch_a8_mtw<3>(p, silu, ntl, Xp, ap, W8, scales, Yp, ws, Tp, N, K, s); break;
      default: launch_a8_mtw<4>(p, silu, ntl, Xp, ap, W8, scales, Yp, ws, Tp, N, K, s); break;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (p.S > 1) {
      Partials part;
      part.p = ws, part.S = p.S, part.NP = p.ntiles * 16;
      if ((e = launch_partials_reduce(part, Yp, Tp, N, s)) != hipSuccess) return e;
    }
  }
  return hipSuccess;
}

}  // namespace ffmi
