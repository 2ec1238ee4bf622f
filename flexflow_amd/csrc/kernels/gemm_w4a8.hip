// gemm_w4a8.hip -- W4A8 linear layers: MXFP4 weights against fp8 (e4m3)
// activations with one dynamic scale per token, on CDNA4's block-scaled matrix
// instruction (v_mfma_scale_f32_16x16x128_f8f6f4, fp32 accumulate).
//
//   Y[t][n] = a[t] * sum_k x8[t][k] * e2m1(nib[n][k]) * 2^e(n, k / 32)
// nib / e: the packed nibbles and e8m0 scale bytes of gemm_w4.hip, unchanged
// (a resident W4 model serves the A16 and the A8 route); x8 / a: the rows
// launch_quantize_rows_fp8 or the quantising RMSNorm writes (gemm_w8a8.hip),
// unchanged.  The instruction multiplies 128 k of an fp4 operand by 128 k of
// an fp8 operand and applies one e8m0 scale per lane to each operand in
// hardware: its block is the MXFP4 block, so a quad step of a (m-tile, n-tile)
// pair is ONE MFMA and no nibble is ever converted (gemm_w4_mid.hip: four
// v_cvt_scalef32_pk and four f16 MFMAs for the same 128 k).
//
// The instruction's lane mapping, as measured on gfx950 with one-hot
// activations against weights of a different scale per block (lane l = (r, g)
// = (l & 15, l >> 4)):
//  * the fp4 operand (first, cbsz 4, four VGPRs): row r, k = 32 g .. 32 g + 31
//    of the step, element i of a dword in bits 4i .. 4i + 3 -- one whole scale
//    block per lane;
//  * the fp8 operand (second, blgp 0, eight VGPRs): row r; bytes 0 .. 15 are
//    k = 16 g .. 16 g + 15, bytes 16 .. 31 are k = 64 + 16 g .. 64 + 16 g + 15
//    -- NOT 32 consecutive k: the 8-bit formats keep the two-halves layout of a
//    64-k instruction pair, only the 4-bit one is contiguous;
//  * the scale of the fp4 operand: byte 0 (op_sel 0) of the lane's scale VGPR
//    scales the lane's own 32 elements, the bytes above are ignored; the fp8
//    operand's scale is the constant 127 (2^0);
//  * D as every 16x16 MFMA here: lane (r, g) holds columns 4 g .. 4 g + 3 of
//    the first operand's rows against row r of the second.
//
// Data movement.  The packed quad block gives lane (r, g') dword j = block j,
// columns 8 g' .. 8 g' + 7: a 4 x 4 dword transpose away from the fp4 operand.
// The transpose is free on the way through LDS: wave w loads the quad blocks of
// tiles w and w + 4 (16 bytes per lane, non-temporal under FFMI_W_STREAM)
// through a register ring and stores each as four dword writes, dword j of lane
// (r, g') to 16-byte piece r + 16 j at dword g' -- one write instruction covers
// 64 consecutive dwords, no bank conflict -- and every wave reads its operand
// of a tile and step as the one 16-byte piece `lane`.  The nibble tile is
// [2][8] KiB (gemm_w4_mid.hip's widened f16 tile: 64 KiB).  A tile's 64 scale
// bytes per step travel with it (16 dwords, row r's four bytes in dword r);
// lane (r, g) shifts dword r down by 8 g.  Activations never touch LDS: lane
// (t, g) gathers its 32 bytes of quad step q straight from X8 as four 8-byte
// pieces at byte 128 q + 64 h + 32 (g & 1) + 8 (g >> 1) + 16 i, (h, i) = (0, 0),
// (0, 1), (1, 0), (1, 1): by X8's chunk order (gemm_w8.h) columns 64 h + 16 g +
// 8 i .. + 7, the fp8 operand as measured.
//
// Work split, two forms of one kernel:
//  * row split (T > 16), gemm_w8a8_kernel's: 4 waves, wave w owns m-tiles
//    w * MTW .. w * MTW + MTW - 1 (MTW = 1 .. 4) and all four share the
//    kW4MidNTW = 8 weight tiles of column group blockIdx.x;
//  * tile split (T <= 16): a row split would leave three waves moving weights
//    only, so all four waves load m-tile 0's rows and wave w multiplies tiles
//    2 w and 2 w + 1 (adjacent, so a gate tile and its up tile stay in one
//    wave) out of the same shared LDS tile.
// gridDim.y = S from plan_w4, a function of (N, K, epilogue) only.  Rows past
// T as gemm_w8a8_kernel: a whole m-tile past T is zeros by a wave-uniform
// predicate, a row past T in a live tile re-reads row T - 1, neither is
// stored.  Every load of the ring is unconditional (gemm_w4.hip says why).
//
// Per output element: the slice's quad steps in sequence, one MFMA each, then
// * a[t], then the direct epilogue or the [S][T][NP] slabs for
// launch_partials_reduce (slices 0 .. S-1 in order).  None of it depends on T,
// MTW, the form or the ring, so a row's bits are a function of the row, N, K
// and the epilogue.
//
// Ring depths w4a8_ring: 6, 4, 3, 2 quad steps at MTW = 1 .. 4 (a slot is 8
// VGPRs of nibbles, 1 of scales and 8 MTW of X beside MTW * 32 accumulators) --
// a first working choice, untuned, like the eight tiles per workgroup.
// Resource usage hipcc reports for gfx950 (every epilogue and load policy
// within 5 VGPRs): tile split: 139 VGPRs + 8 AGPRs; row split MTW = 1: 136 +
// 32, 2: 134 + 64, 3: 136 + 96, 4: 151 + 128 (the grid is plan_w4's, about one
// workgroup of 4 waves per CU); no scratch, no spills; LDS 17 KiB.  The
// registers would hold deeper rings at every MTW; that is the untuned part.
#include <algorithm>

#include "gemm_w4.h"

namespace ffmi {

typedef int v8i __attribute__((ext_vector_type(8)));

constexpr int w4a8_ring(int MTW) { return MTW == 1 ? 6 : MTW == 2 ? 4 : MTW == 3 ? 3 : 2; }

// TS: the tile-split form (MTW == 1, T <= 16); otherwise T <= 4 * MTW * 16 rows.
// X8 [T][K] bytes in block order, a [T]; W4 / scales / pitch and the EPI 1 tile
// pairing as gemm_w4_kernel's.
template <int MTW, bool TS, int EPI, bool NTL>
__global__ __launch_bounds__(256) void gemm_w4a8_kernel(
    const uint8_t *__restrict__ X8, const float *__restrict__ row_scales,
    const uint8_t *__restrict__ W4, const uint8_t *__restrict__ scales, uint16_t *__restrict__ Y,
    float *__restrict__ Ypart, int T, int N, int K, int KT4, int NTILES, int pitch) {
  static_assert(!TS || MTW == 1, "the tile split holds one m-tile");
  constexpr int NTW = kW4MidNTW, PF = w4a8_ring(MTW), WL = NTW / 4;  // WL: tiles a wave loads
  constexpr int NJ = TS ? NTW / 4 : NTW;                             // tiles a wave multiplies
  __shared__ __attribute__((aligned(16))) uint32_t sW[2][NTW][256];  // [piece][dword]
  __shared__ uint32_t sS[2][NTW][16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int ks = blockIdx.y, S = gridDim.y;
  const int tile0 = blockIdx.x * NTW, row0 = TS ? 0 : wave * (MTW * 16);
  const int jt0 = TS ? wave * NJ : 0;  // the wave's first tile of the group
  const int per = (KT4 + S - 1) / S;
  const int kb = min(KT4, ks * per), ke = min(KT4, kb + per);  // (workgroup-uniform)

  const uint8_t *wsrc[WL], *ssrc[WL];
#pragma unroll
  for (int q = 0; q < WL; ++q) {  // (a tile past the last re-reads it and is not stored)
    const size_t tile = (size_t)min(tile0 + wave + 4 * q, NTILES - 1);
    wsrc[q] = W4 + tile * 1024 + lane * 16;
    ssrc[q] = scales + tile * 64 + lr * 4;
  }
  const size_t wks = (size_t)pitch * 1024, sks = (size_t)pitch * 64;
  const uint8_t *xsrc[MTW];
  bool xok[MTW];  // (wave-uniform)
#pragma unroll
  for (int i = 0; i < MTW; ++i) {
    xok[i] = row0 + i * 16 < T;
    xsrc[i] = X8 + (size_t)min(row0 + i * 16 + lr, T - 1) * K + 32 * (lg & 1) + 8 * (lg >> 1);
  }

  f4 acc[MTW][NJ];
#pragma unroll
  for (int i = 0; i < MTW; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};

  if (kb < ke) {
    // A PF-deep register ring holds both operands of quad steps k..k+PF-1
    u4v wq[PF][WL];
    uint32_t sq[PF][WL];
    uint2 xq[PF][MTW][4];
    auto load = [&](int Q, int kq) {
#pragma unroll
      for (int q = 0; q < WL; ++q) {
        wq[Q][q] = ld_w8<NTL>(wsrc[q] + (size_t)kq * wks);
        sq[Q][q] = *reinterpret_cast<const uint32_t *>(ssrc[q] + (size_t)kq * sks);
      }
#pragma unroll
      for (int i = 0; i < MTW; ++i) {
        const uint8_t *p = xsrc[i] + (size_t)kq * 128;
#pragma unroll
        for (int c = 0; c < 4; ++c)  // (h, i) = (c >> 1, c & 1)
          xq[Q][i][c] = xok[i] ? *reinterpret_cast<const uint2 *>(p + 64 * (c >> 1) + 16 * (c & 1))
                               : make_uint2(0, 0);
      }
    };
    auto stage = [&](int Q, int buf) {  // this wave's tiles of one step, transposed
#pragma unroll
      for (int q = 0; q < WL; ++q) {
#pragma unroll
        for (int j = 0; j < 4; ++j) sW[buf][wave + 4 * q][(lr + 16 * j) * 4 + lg] = wq[Q][q][j];
        if (lane < 16) sS[buf][wave + 4 * q][lane] = sq[Q][q];
      }
    };
#pragma unroll
    for (int Q = 0; Q < PF; ++Q) load(Q, min(kb + Q, ke - 1));
    stage(0, 0);
    __syncthreads();
    int cur = 0;
    // one quad step on ring slot Q: the MFMAs read the slot's X in place and
    // the step's pieces from LDS, then the slot is refilled PF steps ahead and
    // the NEXT step's pieces go to the other LDS tile
    auto step = [&](int Q, int kt) {
      if (xok[0]) {  // (a wave without rows only moves weights)
        v8i x[MTW];
#pragma unroll
        for (int i = 0; i < MTW; ++i)
          x[i] = v8i{(int)xq[Q][i][0].x, (int)xq[Q][i][0].y, (int)xq[Q][i][1].x, (int)xq[Q][i][1].y,
                     (int)xq[Q][i][2].x, (int)xq[Q][i][2].y, (int)xq[Q][i][3].x, (int)xq[Q][i][3].y};
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const u4v b = *reinterpret_cast<const u4v *>(&sW[cur][jt0 + j][lane * 4]);
          const int sc = (int)(sS[cur][jt0 + j][lr] >> (8 * lg));
          const v8i w = {(int)b.x, (int)b.y, (int)b.z, (int)b.w, 0, 0, 0, 0};
#pragma unroll
          for (int i = 0; i < MTW; ++i)  // D = W . X^T
            acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w, x[i], acc[i][j], 4, 0, 0,
                                                                         sc, 0, 127);
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

  // Epilogue: the other W4 kernels' lane layout.  D: row m = row0 + i*16 +
  // (lane & 15), columns n = tile*16 + (lane >> 4)*4 + r; acc * a[t] first.
  const int mr = row0 + lr, nq = lg * 4;
  const int NP = NTILES * 16;
#pragma unroll
  for (int i = 0; i < MTW; ++i) {
    const float am = row_scales[min(i * 16 + mr, T - 1)];
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] *= am;
  }
  if (S > 1) {  // EPI == 0 only
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int tile = tile0 + jt0 + j;
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
  for (int j = 0; j < NJ; j += (EPI ? 2 : 1)) {
    const int tile = tile0 + jt0 + j;
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
size_t gemm_w4a8_workspace_bytes(int T, int N, int K, int epilogue) {
  if (T <= 0 || N <= 0 || K <= 0 || K % 128) return 0;
  const W4Plan p = plan_w4(N, K, epilogue);
  return p.S > 1 ? (size_t)p.S * std::min(T, kW4MidRows) * p.ntiles * 16 * sizeof(float) : 0;
}

template <int MTW, bool TS>
static void launch_w4a8_mtw(const W4Plan &p, bool silu, bool ntl, const uint8_t *X8, const float *a,
                            const uint8_t *W4, const uint8_t *scales, uint16_t *Y, float *ws, int T,
                            int N, int K, hipStream_t s) {
  const dim3 grid(p.nblk, p.S), block(256);
#define FFMI_W4A8(EPI, NTL)                                                                       \
  hipLaunchKernelGGL((gemm_w4a8_kernel<MTW, TS, EPI, NTL>), grid, block, 0, s, X8, a, W4, scales, \
                     Y, ws, T, N, K, p.KT4, p.ntiles, p.ntiles)
  if (silu && ntl) FFMI_W4A8(1, true);
  else if (silu) FFMI_W4A8(1, false);
  else if (ntl) FFMI_W4A8(0, true);
  else FFMI_W4A8(0, false);
#undef FFMI_W4A8
}

// One launch per kW4MidRows rows: the tile split for a pass of <= 16 rows,
// otherwise MTW = m-tiles of the pass over the 4 waves
hipError_t launch_gemm_w4a8(const uint8_t *X8, const float *row_scales, const uint8_t *W4,
                            const uint8_t *scales, uint16_t *Y, float *ws, size_t ws_bytes, int T,
                            int N, int K, int epilogue, hipStream_t s) {
  if (T <= 0) return hipSuccess;
  if (N <= 0 || K <= 0 || K % 128 || (epilogue & (FFMI_X_PACKED | FFMI_Y_PACKED)))
    return hipErrorInvalidValue;
  const int base = epilogue & ~FFMI_W_STREAM;
  if (base != FFMI_EPI_NONE && base != FFMI_EPI_SILU_MUL) return hipErrorInvalidValue;
  static_assert(kW4MidNTW == 4 * kW4NT, "plan_w4's column group is the workgroup's");
  const W4Plan p = plan_w4(N, K, epilogue);
  if (p.S > 1 && (!ws || ws_bytes < gemm_w4a8_workspace_bytes(T, N, K, epilogue)))
    return hipErrorInvalidValue;
  const bool silu = base == FFMI_EPI_SILU_MUL, ntl = (epilogue & FFMI_W_STREAM) != 0;
  for (int t0 = 0; t0 < T; t0 += kW4MidRows) {
    const int Tp = std::min(kW4MidRows, T - t0);
    const uint8_t *Xp = X8 + (size_t)t0 * K;
    const float *ap = row_scales + t0;
    uint16_t *Yp = Y + (size_t)t0 * N;
#define FFMI_W4A8_ROWS(MTW, TS) \
  launch_w4a8_mtw<MTW, TS>(p, silu, ntl, Xp, ap, W4, scales, Yp, ws, Tp, N, K, s)
    if (Tp <= 16) FFMI_W4A8_ROWS(1, true);
    else
      switch (((Tp + 15) / 16 + 3) / 4) {
        case 1: FFMI_W4A8_ROWS(1, false); break;
        case 2: FFMI_W4A8_ROWS(2, false); break;
        case 3: FFMI_W4A8_ROWS(3, false); break;
        default: FFMI_W4A8_ROWS(4, false); break;
      }
#undef FFMI_W4A8_ROWS
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
