// gemm_w4_mid.hip -- the MXFP4 weight GEMM for 65 .. 256 rows in one pass over
// the nibbles and scale bytes: the M-split sibling of gemm_w4.hip's
// gemm_w4_kernel, whose packed layout, plan (plan_w4: S a function of (N, K,
// flags) only) and epilogue it shares; the work split is gemm_w8_mid.hip's.
//
// A row's bits are those gemm_w4_kernel gives it: per output element the same
// v_mfma_f32_16x16x32_f16 with the weight fragment first, the same k -> lane
// slot mapping (dword b of a lane's 16 bytes: columns 32 b + 8 (lane >> 4) ..
// + 7, widened at the scale of block b of the lane's row), four MFMAs per quad
// step in k order, the quad steps of a slice in sequence, slice bounds per =
// ceil(KT4 / S), no epilogue multiply, then the direct epilogue or the
// [S][T][NP] slabs for launch_partials_reduce.  Only who holds which operand
// differs:
//  * a workgroup is 4 waves that split the ROWS: wave w owns m-tiles w * MTW ..
//    w * MTW + MTW - 1 (MTW = 2, 3, 4: 128 / 192 / 256 rows per workgroup) and
//    all four share the kW4MidNTW = 8 weight tiles of column group blockIdx.x
//    (the skinny kernel's group, so gridDim.x * S is the grid plan_w4 aims at
//    the CUs; 8 is even, so a gate tile and its up tile sit in one wave);
//  * weights go HBM -> registers -> LDS and are widened once per workgroup:
//    wave w loads the 1 KiB quad blocks and the 64-byte scale groups of tiles
//    j = w and w + 4 (16 bytes per lane plus its row's scale dword, non-temporal
//    under FFMI_W_STREAM) through a register ring, widens them at the block
//    scale (w4_widen, exact) and writes the four f16 fragments of each into a
//    double-buffered LDS tile [2][8][4][64] of h8 (64 KiB); every wave reads
//    all 32 fragments of a step with 16-byte LDS reads.  The alternative --
//    nibbles and scale bytes in LDS (8.5 KiB per buffer) and widening in every
//    wave -- costs four times the conversions (128 v_cvt_scalef32_pk per lane
//    and quad step beside MTW * 32 MFMAs) and an LDS scale read per fragment;
//    the 47 KiB it saves buy no occupancy, because the accumulators hold a
//    workgroup per CU anyway and 64 KiB fit gfx950's 160 KiB;
//  * a wave's activations never touch LDS: lane l loads row (l & 15) of each of
//    its m-tiles, columns 128 kt4 + 32 b + 8 (l >> 4) .. + 7 for b = 0..3,
//    straight from row-major X -- the MFMA's second operand as it stands --
//    into the same ring.  Rows >= T are never read: a whole m-tile past T is
//    zeros by a wave-uniform predicate, a row past T inside a live tile
//    re-reads row T - 1, and neither is stored (D = W . X^T: an X row reaches
//    only its own outputs);
//  * one barrier per quad step: step k's MFMAs read LDS buffer k & 1 while
//    step k + 1's fragments are written to the other.
// Every load of the ring is unconditional, as gemm_w4_kernel's and for its
// reason: past the end of a slice it re-reads the slice's last block.
//
// The ring is w4_mid_ring(MTW) = 4, 3, 2 quad steps deep at MTW = 2, 3, 4: a
// slot is 8 VGPRs of nibbles, 2 of scales and 16 MTW of X (four h8 per m-tile:
// X covers twice the k per weight byte of W8), beside MTW * 32 accumulator
// registers; four slots at MTW = 4 would be 296 + 128.  The depths and the
// eight tiles per workgroup are a first working choice, untuned.
// Resource usage hipcc reports for gfx950 (every epilogue and load policy the
// same): MTW = 2: 224 VGPRs + 92 AGPRs, 3: 246 + 192, 4: 232 + 198 (one
// workgroup of 4 waves per CU; a third slot at MTW = 4 would leave no room);
// no scratch, no spills; LDS 64 KiB.
#include "gemm_w4.h"

namespace ffmi {

// 64 < T <= 4 * MTW * 16 rows; the other arguments as gemm_w4_kernel's
template <int MTW, int EPI, bool NTL>
__global__ __launch_bounds__(256) void gemm_w4_mid_kernel(
    const uint16_t *__restrict__ X, const uint8_t *__restrict__ W4,
    const uint8_t *__restrict__ scales, uint16_t *__restrict__ Y, float *__restrict__ Ypart, int T,
    int N, int K, int KT4, int NTILES, int pitch) {
  constexpr int NTW = kW4MidNTW, PF = w4_mid_ring(MTW), WL = NTW / 4;  // WL: tiles a wave loads
  __shared__ __attribute__((aligned(16))) h8 sW[2][NTW][4][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ks = blockIdx.y, S = gridDim.y;
  const int tile0 = blockIdx.x * NTW, row0 = wave * (MTW * 16);
  const int per = (KT4 + S - 1) / S;
  const int kb = min(KT4, ks * per), ke = min(KT4, kb + per);  // (workgroup-uniform)

  const uint8_t *wsrc[WL], *ssrc[WL];
#pragma unroll
  for (int q = 0; q < WL; ++q) {  // (a tile past the last re-reads it and is not stored)
    const size_t tile = (size_t)min(tile0 + wave + 4 * q, NTILES - 1);
    wsrc[q] = W4 + tile * 1024 + lane * 16;
    ssrc[q] = scales + tile * 64 + (lane & 15) * 4;
  }
  const size_t wks = (size_t)pitch * 1024, sks = (size_t)pitch * 64;
  const uint16_t *xsrc[MTW];
  bool xok[MTW];  // (wave-uniform)
#pragma unroll
  for (int i = 0; i < MTW; ++i) {
    xok[i] = row0 + i * 16 < T;
    xsrc[i] = X + (size_t)min(row0 + i * 16 + (lane & 15), T - 1) * K + 8 * (lane >> 4);
  }

  f4 acc[MTW][NTW];
#pragma unroll
  for (int i = 0; i < MTW; ++i)
#pragma unroll
    for (int j = 0; j < NTW; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};

  if (kb < ke) {
    // A PF-deep register ring holds both operands of quad steps k..k+PF-1
    u4v wq[PF][WL];
    uint32_t sq[PF][WL];
    h8 xq[PF][MTW][4];
    const h8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    auto load = [&](int Q, int kq) {
#pragma unroll
      for (int q = 0; q < WL; ++q) {
        wq[Q][q] = ld_w8<NTL>(wsrc[q] + (size_t)kq * wks);
        sq[Q][q] = *reinterpret_cast<const uint32_t *>(ssrc[q] + (size_t)kq * sks);
      }
#pragma unroll
      for (int i = 0; i < MTW; ++i) {
        const uint16_t *p = xsrc[i] + (size_t)kq * 128;
#pragma unroll
        for (int b = 0; b < 4; ++b)
          xq[Q][i][b] = xok[i] ? *reinterpret_cast<const h8 *>(p + 32 * b) : zero;
      }
    };
    auto stage = [&](int Q, int buf) {  // this wave's tiles of one step, widened once
#pragma unroll
      for (int q = 0; q < WL; ++q)
#pragma unroll
        for (int b = 0; b < 4; ++b)
          sW[buf][wave + 4 * q][b][lane] =
              w4_widen(wq[Q][q][b], e8m0_f32((sq[Q][q] >> (8 * b)) & 0xffu));
    };
#pragma unroll
    for (int Q = 0; Q < PF; ++Q) load(Q, min(kb + Q, ke - 1));
    stage(0, 0);
    __syncthreads();
    int cur = 0;
    // one quad step on ring slot Q: the MFMAs read the slot's X in place and
    // the step's fragments from LDS, block by block, then the slot is refilled
    // PF steps ahead and the NEXT step's fragments go to the other LDS tile
    auto step = [&](int Q, int kt) {
#pragma unroll
      for (int b = 0; b < 4; ++b) {
#pragma unroll
        for (int j = 0; j < NTW; ++j) {
          const h8 w = sW[cur][j][b][lane];
#pragma unroll
          for (int i = 0; i < MTW; ++i)  // D = W . X^T
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w, xq[Q][i][b], acc[i][j], 0, 0, 0);
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

  // Epilogue: gemm_w4_kernel's with the wave's row offset.  D layout: row m =
  // row0 + i*16 + (lane & 15), columns n = tile*16 + (lane >> 4)*4 + r.
  const int mr = row0 + (lane & 15), nq = (lane >> 4) * 4;
  const int NP = NTILES * 16;
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

template <int MTW>
static void launch_mtw(const W4Plan &p, bool silu, bool ntl, const uint16_t *X, const uint8_t *W4,
                       const uint8_t *scales, uint16_t *Y, float *ws, int T, int N, int K,
                       hipStream_t s) {
  const dim3 grid(p.nblk, p.S), block(256);
#define FFMI_W4M(EPI, NTL)                                                                        \
  hipLaunchKernelGGL((gemm_w4_mid_kernel<MTW, EPI, NTL>), grid, block, 0, s, X, W4, scales, Y, ws, \
                     T, N, K, p.KT4, p.ntiles, p.ntiles)
  if (silu && ntl) FFMI_W4M(1, true);
  else if (silu) FFMI_W4M(1, false);
  else if (ntl) FFMI_W4M(0, true);
  else FFMI_W4M(0, false);
#undef FFMI_W4M
}

void launch_w4_mid_rows(const W4Plan &p, int MTW, bool silu, bool ntl, const uint16_t *X,
                        const uint8_t *W4, const uint8_t *scales, uint16_t *Y, float *ws, int T,
                        int N, int K, hipStream_t s) {
  switch (MTW) {
    case 2: launch_mtw<2>(p, silu, ntl, X, W4, scales, Y, ws, T, N, K, s); break;
    case 3: launch_mtw<3>(p, silu, ntl, X, W4, scales, Y, ws, T, N, K, s); break;
    default: launch_mtw<4>(p, silu, ntl, X, W4, scales, Y, ws, T, N, K, s); break;
  }
}

}  // namespace ffmi
