// gemm_w4.hip -- OCP MXFP4 weight-only linear layers: the W4A16 GEMM, its
// quantiser / packer and its launch plan.
//
//   Y[t][n] = sum_k X[t][k] * deq[n][k],   deq[n][k] = e2m1(nibble) * 2^e(n, k / 32)
// X, Y fp16; one e8m0 scale byte (e + 127) per 32 consecutive k of a row: 4.25
// bits per weight.  The quantiser's rule is stated in include/ffmi.h; its lower
// clamp e >= -12 makes every nonzero deq at least 2^-13, a normal f16, and
// 6 * 2^13 is finite, so v_cvt_scalef32_pk_f16_fp4 widens two nibbles at scale
// 2^e exactly and the MFMA (v_mfma_f32_16x16x32_f16, fp32 accumulate) never
// sees a subnormal operand.  A 32-k scale block is the K extent of that MFMA
// and a lane's A-fragment is 8 elements of one row inside one block: one scale
// per lane and MFMA, applied by the conversion -- no epilogue multiply.
//
// Packed layout, the nibble analogue of gemm_w8.hip's double blocks: the [N][K]
// matrix is cut into 16 x 128 QUAD BLOCKS of 1 KiB; lane l owns 16 contiguous
// bytes, dword j (j = 0..3, the 32-k block) = row nt*16 + (l&15), columns
// kt4*128 + 32j + 8*(l>>4) + 0..7, element i in bits 4i..4i+3: one 16-byte
// load per lane feeds four MFMAs, a wave reads 1 KiB contiguous per step.  The
// scales are a separate array, 64 bytes per quad block: row r's four scale
// bytes (block j in byte j) at 4r, so a lane reads its row's scales as one
// dword and a scale becomes a float by byte << 23.  Both arrays are K-major
// (quad block (nt, kt4) at (kt4 * P + nt) KiB / * 64 bytes, P = tiles per
// k-row of the allocation).  in_dim % 128 == 0; out_dim is padded to 16
// (padding rows: zero nibbles, scale byte 127).
//
// The GEMM of this file (T <= 64 rows per launch: the decode regime;
// gemm_w4_mid.hip holds the M-split kernel for 65 .. 256 rows, with the same
// numerics per row, and plan_w4_launch below chooses between them) follows
// gemm_w8_kernel: 4 waves, wave w owns kW4NT adjacent n-tiles, gridDim.y = S
// splits K (plan_w4: a function of (N, K, epilogue), never of T); weights and
// scales go from global memory straight to registers through a ring kW4Ring
// quad blocks deep per tile, non-temporal under FFMI_W_STREAM; the activation
// chunk (MT*16 rows x 128 k) is loaded cooperatively through the same ring,
// staged in a double-buffered LDS tile in A-fragment order (MT * 8 KiB per
// buffer pair) and read by every wave with 16-byte LDS reads; D = W_tile .
// X_tile^T, a lane holds 4 consecutive output columns of one row.
//
// kW4NT = 2, kW4Ring = 6: 4 waves x 2 x 6 KiB = 48 KiB of weight loads in
// flight per workgroup, gemm_w8_kernel's figure.  X covers twice the k per
// weight byte, so a ring slot carries 4 MT VGPRs of X per thread beside 10 of
// weights and scales: at MT = 4 the ring is 96 + 60 VGPRs.  Four tiles per
// wave at ring depth 3 would halve the X registers and LDS reads for the same
// bytes in flight, but also the column groups: N = 4096 would start 16 groups
// x S = 8 = 128 workgroups on 256 CUs.  Two tiles keep plan_w8's grid (8 tiles
// per workgroup), and a slice keeps at least kW4MinSteps = 2 quad steps, the
// 256 k of W8's four double steps.  Every load of the ring is unconditional
// (past the end of a slice it re-reads the last block, as gemm_w8_kernel's):
// with the loads behind workgroup-uniform predicates instead, the compiler
// drained the memory counter at every join (no wait deeper than vmcnt(3)) and
// a step waited a whole HBM latency.  Only the tail's steps, which have
// nothing a ring ahead, issue none.
// Resource usage hipcc reports for gfx950 (every epilogue and load policy the
// same): MT = 1: 112 VGPRs + 12 AGPRs, 2: 150 + 20, 3: 184 + 36, 4: 208 + 56
// (one workgroup of 4 waves per CU, as the plan assumes); no scratch, no
// spills; LDS MT * 8 KiB.
// Per output element the order is: the quad steps of the slice in sequence
// (four MFMAs each, in k order), then slices 0..S-1 (launch_partials_reduce)
// -- fixed by (N, K, epilogue).
#include <algorithm>
#include <cstdlib>

#include "gemm_w4.h"

namespace ffmi {

// T <= MT*16 <= 64 rows; X row-major [T][K], K = 128 KT4; W4 / scales as above
// (pitch = tiles per k-row of the allocation); EPI 1: tiles (2p, 2p+1) =
// (gate, up) of output columns [16p, 16p+16), S == 1 (host-checked).
template <int MT, int EPI, bool NTL>
__global__ __launch_bounds__(256) void gemm_w4_kernel(
    const uint16_t *__restrict__ X, const uint8_t *__restrict__ W4,
    const uint8_t *__restrict__ scales, uint16_t *__restrict__ Y, float *__restrict__ Ypart, int T,
    int N, int K, int KT4, int NTILES, int pitch) {
  constexpr int NT = kW4NT, PF = kW4Ring;
  // the chunk is MT*256 pieces of 16 bytes (row r = p / 16, columns 8 (p % 16) ..):
  // thread t takes pieces t + 256 q, row (t >> 4) of m-tile q
  __shared__ __attribute__((aligned(16))) h8 sX[2][MT][4][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ks = blockIdx.y, S = gridDim.y;
  const int tile0 = (blockIdx.x * 4 + wave) * NT;
  const int per = (KT4 + S - 1) / S;
  const int kb = min(KT4, ks * per), ke = min(KT4, kb + per);  // (workgroup-uniform)

  const uint8_t *wsrc[NT], *ssrc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {  // (a wave past the last tile re-reads it and stores nothing)
    const size_t tile = (size_t)min(tile0 + j, NTILES - 1);
    wsrc[j] = W4 + tile * 1024 + lane * 16;
    ssrc[j] = scales + tile * 64 + (lane & 15) * 4;
  }
  const size_t wks = (size_t)pitch * 1024, sks = (size_t)pitch * 64;
  const int xr = tid >> 4, xc = tid & 15;
  const uint16_t *xsrc[MT];
  bool xok[MT];
#pragma unroll
  for (int q = 0; q < MT; ++q) {
    xok[q] = q * 16 + xr < T;
    xsrc[q] = X + (size_t)(xok[q] ? q * 16 + xr : 0) * K + xc * 8;
  }
  h8 *const xdst = &sX[0][0][xc >> 2][xr + 16 * (xc & 3)];  // (m-tile q: 4*64 fragments on)

  f4 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};

  if (kb < ke) {
    // A PF-deep register ring holds both operands of quad steps k..k+PF-1
    u4v wq[PF][NT];
    uint32_t sq[PF][NT];
    h8 xq[PF][MT];
    const h8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    auto load = [&](int Q, int kq) {
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        wq[Q][j] = ld_w8<NTL>(wsrc[j] + (size_t)kq * wks);
        sq[Q][j] = *reinterpret_cast<const uint32_t *>(ssrc[j] + (size_t)kq * sks);
      }
#pragma unroll
      for (int q = 0; q < MT; ++q)
        xq[Q][q] = xok[q] ? *reinterpret_cast<const h8 *>(xsrc[q] + (size_t)kq * 128) : zero;
    };
    auto stage = [&](int Q, int buf) {
#pragma unroll
      for (int q = 0; q < MT; ++q) xdst[(buf * MT + q) * (4 * 64)] = xq[Q][q];
    };
#pragma unroll
    for (int Q = 0; Q < PF; ++Q) load(Q, min(kb + Q, ke - 1));
    stage(0, 0);
    __syncthreads();
    int cur = 0;
    // one quad step on ring slot Q: the MFMAs read the slot in place, block by
    // block, then it is refilled PF steps ahead (never in the tail, whose steps
    // have nothing PF ahead) and the NEXT step's X goes to the other tile
    auto step = [&](int Q, int kt, bool refill) {
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        h8 a[MT];
#pragma unroll
        for (int i = 0; i < MT; ++i) a[i] = sX[cur][i][b][lane];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          const h8 w = w4_widen(wq[Q][j][b], e8m0_f32((sq[Q][j] >> (8 * b)) & 0xffu));
#pragma unroll
          for (int i = 0; i < MT; ++i)  // D = W . X^T
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w, a[i], acc[i][j], 0, 0, 0);
        }
      }
      if (refill) load(Q, min(kt + PF, ke - 1));
      stage((Q + 1) % PF, cur ^ 1);
      __syncthreads();
      cur ^= 1;
    };
    int kt0 = kb;
    for (; kt0 + PF <= ke; kt0 += PF) {  // steady state: whole ring turns
#pragma unroll
      for (int Q = 0; Q < PF; ++Q) step(Q, kt0 + Q, true);
    }
#pragma unroll
    for (int Q = 0; Q < PF - 1; ++Q)  // tail: < PF steps, slots 0..
      if (kt0 + Q < ke) step(Q, kt0 + Q, false);
  }

  // Epilogue.  D layout: row m = i*16 + (lane & 15), columns n = tile*16 +
  // (lane >> 4)*4 + r.
  const int mr = lane & 15, nq = (lane >> 4) * 4;
  const int NP = NTILES * 16;
  if (S > 1) {  // EPI == 0 only
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int tile = tile0 + j;
      if (tile >= NTILES) continue;
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        const int m = i * 16 + mr;
        if (m < T)
          *reinterpret_cast<f4 *>(Ypart + ((size_t)ks * T + m) * NP + tile * 16 + nq) = acc[i][j];
      }
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < NT; j += (EPI ? 2 : 1)) {
    const int tile = tile0 + j;
    if (tile >= NTILES) continue;
    const int n = (EPI ? (tile >> 1) : tile) * 16 + nq;
    if (n >= N) continue;
#pragma unroll
    for (int i = 0; i < MT; ++i) {
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

// ---------------------------------------------------------------------------
// Quantise and pack: one workgroup per 16-row tile of a row-major fp16 matrix
// (row stride ld); a wave takes every fourth quad block.  Lane l reads its 4 x
// 8 columns of row l & 15; the four lanes of a row (l >> 4 = 0..3) share each
// 32-k block, so the block's amax is two shuffles.  With E the biased exponent
// of amax as fp16, floor(log2 amax) = E - 15 for a normal amax and below -14
// for a subnormal one, so e = max(E, 5) - 17 (amax == 0: e = 0).  The code of
// |w| / 2^e (exact in fp32) is the count of thresholds it passes, the ties
// 0.25, 1.25, 2.5, 5 staying below (even code) and 0.75, 1.75, 3.5 going up.
// Destination tile tile_step * nt + tile_offset of an allocation of `pitch`
// tiles per k-row, for the nibbles and for the scales alike.
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t w4_code(uint32_t hbits, float inv) {
  const float v = fabsf(h2f((uint16_t)hbits)) * inv;
  const uint32_t c = (v > 0.25f) + (v >= 0.75f) + (v > 1.25f) + (v >= 1.75f) + (v > 2.5f) +
                     (v >= 3.5f) + (v > 5.0f);
  return ((hbits >> 12) & 8u) | c;
}

__global__ __launch_bounds__(256) void w4_quantize_pack_kernel(
    const uint16_t *__restrict__ src, int ld, int N, int K, uint8_t *__restrict__ dst,
    uint8_t *__restrict__ scales, int tile_step, int tile_offset, int pitch) {
  const int tid = threadIdx.x, nt = blockIdx.x, lane = tid & 63;
  const int dtile = tile_step * nt + tile_offset;
  const int row = lane & 15, g = lane >> 4, n = nt * 16 + row;
  for (int kt4 = tid >> 6; kt4 < K / 128; kt4 += 4) {
    uint32_t out[4] = {0, 0, 0, 0}, sc = 0x7f7f7f7fu;
    if (n < N) {  // (a row's four lanes take this branch together)
      sc = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint4 v =
            *reinterpret_cast<const uint4 *>(src + (size_t)n * ld + kt4 * 128 + 32 * j + 8 * g);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        uint32_t m = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) m = max(m, max(w[e] & 0x7fffu, (w[e] >> 16) & 0x7fffu));
        m = max(m, (uint32_t)__shfl_xor((int)m, 16));
        m = max(m, (uint32_t)__shfl_xor((int)m, 32));
        const int e = m ? max((int)(m >> 10), 5) - 17 : 0;
        const float inv = __uint_as_float((uint32_t)(127 - e) << 23);  // 2^-e
        sc |= (uint32_t)(e + 127) << (8 * j);
#pragma unroll
        for (int i = 0; i < 4; ++i)
          out[j] |= (w4_code(w[i] & 0xffffu, inv) | (w4_code(w[i] >> 16, inv) << 4)) << (8 * i);
      }
    }
    const size_t blk = (size_t)kt4 * pitch + dtile;
    *reinterpret_cast<uint4 *>(dst + blk * 1024 + lane * 16) = make_uint4(out[0], out[1], out[2], out[3]);
    if (g == 0) *reinterpret_cast<uint32_t *>(scales + blk * 64 + row * 4) = sc;
  }
}

// tests: row-major [N][K] nibble values (one per byte) and [N][K/32] scale
// bytes of tiles tile_step * nt + tile_offset
__global__ void w4_unpack_kernel(const uint8_t *__restrict__ src, const uint8_t *__restrict__ scales,
                                 int N, int K, uint8_t *__restrict__ nib, uint8_t *__restrict__ sc,
                                 int tile_step, int tile_offset, int pitch) {
  const long idx = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (idx >= (long)N * K) return;
  const int n = (int)(idx / K), k = (int)(idx % K);
  const int tile = tile_step * (n >> 4) + tile_offset, c = k & 127, j = c >> 5, i = c & 7;
  const int lane = (n & 15) + 16 * ((c >> 3) & 3);
  const size_t blk = (size_t)(k >> 7) * pitch + tile;
  nib[idx] = (src[blk * 1024 + lane * 16 + 4 * j + (i >> 1)] >> (4 * (i & 1))) & 15;
  if ((k & 31) == 0) sc[(size_t)n * (K / 32) + (k >> 5)] = scales[blk * 64 + (n & 15) * 4 + j];
}

size_t w4_packed_bytes(int N, int K) { return (size_t)((N + 15) / 16) * (size_t)(K / 128) * 1024; }
size_t w4_scale_bytes(int N, int K) { return (size_t)((N + 15) / 16) * (size_t)(K / 128) * 64; }

hipError_t launch_w4_quantize_pack(const uint16_t *src, int ld, int N, int K, uint8_t *dst,
                                   uint8_t *scales, int tile_step, int tile_offset, int pitch,
                                   hipStream_t s) {
  if (N <= 0 || K <= 0 || K % 128 || ld % 8) return hipErrorInvalidValue;
  hipLaunchKernelGGL(w4_quantize_pack_kernel, dim3((N + 15) / 16), dim3(256), 0, s, src, ld, N, K,
                     dst, scales, tile_step, tile_offset, pitch);
  return hipGetLastError();
}

hipError_t launch_w4_unpack(const uint8_t *src, const uint8_t *scales, int N, int K, uint8_t *nib,
                            uint8_t *sc, int tile_step, int tile_offset, int pitch, hipStream_t s) {
  if (N <= 0 || K <= 0 || K % 128) return hipErrorInvalidValue;
  const long total = (long)N * K;
  hipLaunchKernelGGL(w4_unpack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, src,
                     scales, N, K, nib, sc, tile_step, tile_offset, pitch);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Plan: plan_w8's, in quad steps.  S depends on (N, K, epilogue) only; gate/up
// is never split; otherwise K is split until the grid holds about one
// workgroup per CU, a slice keeping at least kW4MinSteps quad steps, and no
// slice is empty.
// ---------------------------------------------------------------------------
W4Plan plan_w4(int N, int K, int epilogue) {
  W4Plan p;
  const bool silu = (epilogue & 0xf) == FFMI_EPI_SILU_MUL;
  p.ntiles = (silu ? 2 : 1) * ((N + 15) / 16);
  p.nblk = (p.ntiles + 4 * kW4NT - 1) / (4 * kW4NT);
  p.KT4 = K / 128;
  p.S = 1;
  if (!silu) {
    const int want = kW4Groups / p.nblk;
    const int S = std::max(1, std::min({want, kW4MaxS, p.KT4 / kW4MinSteps}));
    const int per = (p.KT4 + S - 1) / S;
    p.S = (p.KT4 + per - 1) / per;
  }
  return p;
}

size_t gemm_w4_workspace_bytes(int T, int N, int K, int epilogue) {
  if (T <= 0 || N <= 0 || K <= 0 || K % 128) return 0;
  const W4Plan p = plan_w4(N, K, epilogue);
  return p.S > 1 ? (size_t)p.S * std::min(T, kW4Rows) * p.ntiles * 16 * sizeof(float) : 0;
}

template <int MT>
static void launch_w4_rows(const W4Plan &p, bool silu, bool ntl, const uint16_t *X,
                           const uint8_t *W4, const uint8_t *scales, uint16_t *Y, float *ws, int T,
                           int N, int K, hipStream_t s) {
  const dim3 grid(p.nblk, p.S), block(256);
#define FFMI_W4(EPI, NTL)                                                                      \
  hipLaunchKernelGGL((gemm_w4_kernel<MT, EPI, NTL>), grid, block, 0, s, X, W4, scales, Y, ws, T, \
                     N, K, p.KT4, p.ntiles, p.ntiles)
  if (silu && ntl) FFMI_W4(1, true);
  else if (silu) FFMI_W4(1, false);
  else if (ntl) FFMI_W4(0, true);
  else FFMI_W4(0, false);
#undef FFMI_W4
}

size_t gemm_w4_onepass_workspace_bytes(int T, int N, int K, int epilogue) {
  if (T <= 0 || N <= 0 || K <= 0 || K % 128) return 0;
  const W4Plan p = plan_w4(N, K, epilogue);
  return p.S > 1 ? (size_t)p.S * std::min(T, kW4MidRows) * p.ntiles * 16 * sizeof(float) : 0;
}

// FFMI_W4_MULTIPASS=1: rows above 64 keep one skinny pass per 64 rows, whatever
// the workspace (A/B against the M-split kernel in one build); once
static bool sw_w4_multipass() {
  static const bool v = [] { const char *e = getenv("FFMI_W4_MULTIPASS"); return e && atoi(e) != 0; }();
  return v;
}

// The launch plan: what launch_gemm_w4 does and ffmi_debug_linear_w4_plan
// reports -- plan_w8_launch's rule.  Above 64 rows the M-split kernel
// (gemm_w4_mid.hip) covers 256 rows per weight pass where the workspace holds
// its slabs (a shape that does not split K needs none); a split shape given
// only the minimum, the skinny kernel's 64 rows of slabs, keeps one skinny
// pass per 64 rows.  The bits are the same.
W4Launch plan_w4_launch(int T, int N, int K, int epilogue, size_t ws_bytes) {
  W4Launch l;
  const W4Plan p = plan_w4(N, K, epilogue);
  l.path = T > kW4Rows && !sw_w4_multipass() &&
           ws_bytes >= gemm_w4_onepass_workspace_bytes(T, N, K, epilogue);
  l.rows = l.path ? kW4MidRows : kW4Rows;
  const int mt = (std::min(T, l.rows) + 15) / 16;  // m-tiles of the first pass
  l.MTW = l.path ? std::max(2, (mt + 3) / 4) : mt;
  l.NTW = l.path ? kW4MidNTW : kW4NT;
  l.S = p.S, l.passes = (T + l.rows - 1) / l.rows, l.nblk = p.nblk;
  return l;
}

// One launch (and, for a split shape, one reduce) per l.rows rows: the M-split
// kernel for a pass of more than 64 rows, the skinny kernel for a shorter
// (last) one
hipError_t launch_gemm_w4(const uint16_t *X, const uint8_t *W4, const uint8_t *scales, uint16_t *Y,
                          float *ws, size_t ws_bytes, int T, int N, int K, int epilogue,
                          hipStream_t s) {
  if (T <= 0) return hipSuccess;
  if (N <= 0 || K <= 0 || K % 128 || (epilogue & (FFMI_X_PACKED | FFMI_Y_PACKED)))
    return hipErrorInvalidValue;
  const int base = epilogue & ~FFMI_W_STREAM;
  if (base != FFMI_EPI_NONE && base != FFMI_EPI_SILU_MUL) return hipErrorInvalidValue;
  const W4Plan p = plan_w4(N, K, epilogue);
  if (p.S > 1 && (!ws || ws_bytes < gemm_w4_workspace_bytes(T, N, K, epilogue)))
    return hipErrorInvalidValue;
  const W4Launch l = plan_w4_launch(T, N, K, epilogue, ws ? ws_bytes : 0);
  const bool silu = base == FFMI_EPI_SILU_MUL, ntl = (epilogue & FFMI_W_STREAM) != 0;
  for (int t0 = 0; t0 < T; t0 += l.rows) {
    const int Tp = std::min(l.rows, T - t0), mt = (Tp + 15) / 16;
    const uint16_t *Xp = X + (size_t)t0 * K;
    uint16_t *Yp = Y + (size_t)t0 * N;
    if (Tp > kW4Rows) {
      launch_w4_mid_rows(p, std::max(2, (mt + 3) / 4), silu, ntl, Xp, W4, scales, Yp, ws, Tp, N, K,
                         s);
    } else {
      switch (mt) {
        case 1: launch_w4_rows<1>(p, silu, ntl, Xp, W4, scales, Yp, ws, Tp, N, K, s); break;
        case 2: launch_w4_rows<2>(p, silu, ntl, Xp, W4, scales, Yp, ws, Tp, N, K, s); break;
        case 3: launch_w4_rows<3>(p, silu, ntl, Xp, W4, scales, Yp, ws, Tp, N, K, s); break;
        default: launch_w4_rows<4>(p, silu, ntl, Xp, W4, scales, Yp, ws, Tp, N, K, s); break;
      }
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
