// gemm_w8.hip -- fp8 (e4m3) weight-only linear layers: the W8A16 GEMM, its
// quantiser / packer and its launch plan.
//
//   Y[t][n] = s[n] * sum_k X[t][k] * q[n][k]
// X, Y fp16; q[n][k] the OCP e4m3fn byte of W[n][k] / s[n], s[n] = absmax of
// row n / 448 (fp32, one per output channel).  e4m3 -> f16 is exact, so the
// MFMA (v_mfma_f32_16x16x32_f16, fp32 accumulate) runs on exactly widened
// operands and s[n] is one multiply in the epilogue.
//
// Packed layout, the byte analogue of weights.hip's "MFMA B-fragment order":
// the [N][K] byte matrix is cut into 16 x 64 DOUBLE BLOCKS of 1 KiB; lane l
// owns 16 contiguous bytes, the first 8 = q[nt*16 + (l&15)][kt2*64 + 8*(l>>4)
// + 0..7], the second 8 the same columns + 32: one 16-byte load per lane feeds
// two MFMAs, a wave reads 1 KiB contiguous per step.  Double blocks are stored
// K-major (block (nt, kt2) at (kt2 * P + nt) KiB, P = tiles per k-row of the
// allocation), for weights.hip's reason: every workgroup walks k in step, so
// the chip reads one contiguous band at a time.  in_dim % 64 == 0; out_dim is
// padded to 16 (padding rows: zero bytes, scale 1).
//
// The GEMM of this file (T <= 64 rows per launch: the weight-bandwidth-bound
// regime; gemm_w8_mid.hip holds the M-split kernel for 65 .. 256 rows, with
// the same numerics per row, and plan_w8_launch below chooses between them):
//  * a workgroup is 4 waves; wave w owns kW8NT adjacent n-tiles, columns
//    distinct from the other waves', and all four walk the same k-range in
//    step.  gridDim.x covers the n-tile groups; gridDim.y = S splits K over
//    workgroups where the groups alone would leave the chip idle (plan_w8:
//    a function of (N, K, flags), never of T);
//  * weights go from global memory straight to registers (never LDS), through
//    a ring kW8Ring double blocks deep per tile: kW8NT * kW8Ring KiB of loads
//    in flight per wave, non-temporal under FFMI_W_STREAM; bytes are widened
//    with v_cvt_scalef32_pk_f16_fp8 at scale 1, four conversions per 8 bytes;
//  * the activation chunk (MT*16 rows x 64 k, MT = ceil(T/16) <= 4) is shared
//    by the four waves: loaded cooperatively once from row-major X (through
//    the same-depth register ring: loads retire in order, so X must be issued
//    as early as the weights it meets), written to a double-buffered LDS tile
//    in A-fragment order and read by every wave with 16-byte LDS reads: X
//    traffic per weight byte is MT / (2 kW8NT) from LDS, not from L2 once per
//    wave.  Rows >= T are zeros by predicate and never read from memory;
//  * the MFMAs compute D = W_tile . X_tile^T, so a lane holds 4 consecutive
//    output columns of one row (gemm.hip mid_store): s[n] comes in as one
//    16-byte load, Y goes out as 8-byte stores, a split-K partial as 16-byte
//    stores into the Partials slab layout [S][T][NP], which the existing
//    launch_partials_reduce sums in slab order and rounds once.
// Per output element the order is: the k-steps of the slice in sequence (two
// MFMAs each), times s[n], then slices 0..S-1 -- fixed by (N, K, flags).
#include <stdlib.h>

#include <algorithm>

#include "gemm_w8.h"

namespace ffmi {

// T <= MT*16 <= 64 rows; X row-major [T][K], K = 64 KT2; W8 / scales as above
// (pitch = tiles per k-row of the allocation); EPI 1: tiles (2p, 2p+1) =
// (gate, up) of output columns [16p, 16p+16), S == 1 (host-checked).
template <int MT, int EPI, bool NTL>
__global__ __launch_bounds__(256) void gemm_w8_kernel(
    const uint16_t *__restrict__ X, const uint8_t *__restrict__ W8,
    const float *__restrict__ scales, uint16_t *__restrict__ Y, float *__restrict__ Ypart, int T,
    int N, int K, int KT2, int NTILES, int pitch) {
  constexpr int NT = kW8NT, PF = kW8Ring;
  // the chunk is MT*128 pieces of 16 bytes (row r = p / 8, columns 8 (p % 8) ..):
  // thread t takes pieces t, t + 256 (MT = 1: the first 128 threads one each)
  constexpr int XPT = (MT * 128 + 255) / 256;
  __shared__ __attribute__((aligned(16))) h8 sX[2][MT][2][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ks = blockIdx.y, S = gridDim.y;
  const int tile0 = (blockIdx.x * 4 + wave) * NT;
  const int per = (KT2 + S - 1) / S;
  const int kb = min(KT2, ks * per), ke = min(KT2, kb + per);  // (workgroup-uniform)

  const uint8_t *wsrc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j)  // (a wave past the last tile re-reads it and stores nothing)
    wsrc[j] = W8 + (size_t)min(tile0 + j, NTILES - 1) * 1024 + lane * 16;
  const size_t wks = (size_t)pitch * 1024;
  const uint16_t *xsrc[XPT];
  bool xok[XPT];
  h8 *xdst[XPT];  // (in buffer 0; buffer 1 is MT*2*64 fragments on)
#pragma unroll
  for (int q = 0; q < XPT; ++q) {
    const int p = tid + 256 * q, r = p >> 3, c = p & 7;
    xok[q] = p < MT * 128 && r < T;
    xsrc[q] = X + (size_t)(xok[q] ? r : 0) * K + c * 8;
    xdst[q] = &sX[0][min(r >> 4, MT - 1)][c >> 2][(r & 15) + 16 * (c & 3)];
  }
  const bool xmine[2] = {tid < MT * 128, tid + 256 < MT * 128};

  f4 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};

  if (kb < ke) {
    // A PF-deep register ring holds both operands of double steps k..k+PF-1
    u4v wq[PF][NT];
    h8 xq[PF][XPT];
    const h8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    auto load = [&](int Q, int kq) {
#pragma unroll
      for (int j = 0; j < NT; ++j) wq[Q][j] = ld_w8<NTL>(wsrc[j] + (size_t)kq * wks);
#pragma unroll
      for (int q = 0; q < XPT; ++q)
        xq[Q][q] = xok[q] ? *reinterpret_cast<const h8 *>(xsrc[q] + (size_t)kq * 64) : zero;
    };
    auto stage = [&](int Q, int buf) {
#pragma unroll
      for (int q = 0; q < XPT; ++q)
        if (xmine[q]) xdst[q][buf * (MT * 2 * 64)] = xq[Q][q];
    };
#pragma unroll
    for (int Q = 0; Q < PF; ++Q) load(Q, min(kb + Q, ke - 1));
    stage(0, 0);
    __syncthreads();
    int cur = 0;
    // one double step on ring slot Q: the MFMAs read the slot in place, then it
    // is refilled PF steps ahead and the NEXT step's X goes to the other tile
    auto step = [&](int Q, int kt) {
      h8 a[MT][2];
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        a[i][0] = sX[cur][i][0][lane];
        a[i][1] = sX[cur][i][1][lane];
      }
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const h8 b0 = w8_widen(wq[Q][j].x, wq[Q][j].y), b1 = w8_widen(wq[Q][j].z, wq[Q][j].w);
#pragma unroll
        for (int i = 0; i < MT; ++i) {  // D = W . X^T
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(b0, a[i][0], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(b1, a[i][1], acc[i][j], 0, 0, 0);
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

  // Epilogue.  D layout: row m = i*16 + (lane & 15), columns n = tile*16 +
  // (lane >> 4)*4 + r.
  const int mr = lane & 15, nq = (lane >> 4) * 4;
  const int NP = NTILES * 16;
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    if (tile0 + j >= NTILES) continue;
    const f4 sc = *reinterpret_cast<const f4 *>(scales + (size_t)(tile0 + j) * 16 + nq);
#pragma unroll
    for (int i = 0; i < MT; ++i) acc[i][j] *= sc;
  }
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
// (row stride ld).  16 threads per row find its absmax; s = absmax / 448 (IEEE
// fp32 division; an all-zero row and a padding row: s = 1); then every thread
// writes 16-byte lane pieces of the tile's double blocks, each byte the rule
// of attention_util.h (kv8_quant4: x / s in fp32, clamped, nearest even; the
// NaN byte is never written).  Destination tile tile_step * nt + tile_offset
// of an allocation of `pitch` tiles per k-row (gate/up: step 2, offsets 0/1;
// qkv: offsets 0, Hl/16, ...); scales[16 * destination tile + row].
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void w8_quantize_pack_kernel(
    const uint16_t *__restrict__ src, int ld, int N, int K, uint8_t *__restrict__ dst,
    float *__restrict__ scales, int tile_step, int tile_offset, int pitch) {
  __shared__ float sS[16];
  const int tid = threadIdx.x, nt = blockIdx.x;
  const int dtile = tile_step * nt + tile_offset;
  {
    const int row = tid >> 4, sub = tid & 15, n = nt * 16 + row;
    float amax = 0.f;
    if (n < N)
      for (int k = sub * 8; k < K; k += 128) {
        const uint4 v = *reinterpret_cast<const uint4 *>(src + (size_t)n * ld + k);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 4; ++e)
          amax = fmaxf(amax, fmaxf(fabsf(h2f(w[e] & 0xffff)), fabsf(h2f(w[e] >> 16))));
      }
#pragma unroll
    for (int d = 1; d < 16; d <<= 1) amax = fmaxf(amax, __shfl_xor(amax, d));
    if (sub == 0) {
      const float s = amax > 0.f ? __fdiv_rn(amax, 448.f) : 1.f;
      sS[row] = s;
      scales[(size_t)dtile * 16 + row] = s;
    }
  }
  __syncthreads();
  const int lane = tid & 63, row = lane & 15, n = nt * 16 + row;
  const float s = sS[row];
  for (int kt2 = tid >> 6; kt2 < K / 64; kt2 += 4) {
    uint4 out = make_uint4(0, 0, 0, 0);
    if (n < N) {
      const uint16_t *p = src + (size_t)n * ld + kt2 * 64 + 8 * (lane >> 4);
      const uint4 a = *reinterpret_cast<const uint4 *>(p), b = *reinterpret_cast<const uint4 *>(p + 32);
      auto q4 = [&](uint32_t lo, uint32_t hi) {
        return kv8_quant_h4(lo & 0xffff, lo >> 16, hi & 0xffff, hi >> 16, s);
      };
      out = make_uint4(q4(a.x, a.y), q4(a.z, a.w), q4(b.x, b.y), q4(b.z, b.w));
    }
    *reinterpret_cast<uint4 *>(dst + ((size_t)kt2 * pitch + dtile) * 1024 + lane * 16) = out;
  }
}

// tests: row-major [N][K] bytes of tiles tile_step * nt + tile_offset
__global__ void w8_unpack_kernel(const uint8_t *__restrict__ src, int N, int K,
                                 uint8_t *__restrict__ dst, int tile_step, int tile_offset,
                                 int pitch) {
  const long idx = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (idx >= (long)N * K) return;
  const int n = (int)(idx / K), k = (int)(idx % K);
  const int tile = tile_step * (n >> 4) + tile_offset, c = k & 63;
  const int lane = (n & 15) + 16 * ((c >> 3) & 3);
  dst[idx] = src[((size_t)(k >> 6) * pitch + tile) * 1024 + lane * 16 + 8 * (c >> 5) + (c & 7)];
}

size_t w8_packed_bytes(int N, int K) { return (size_t)((N + 15) / 16) * (size_t)(K / 64) * 1024; }

hipError_t launch_w8_quantize_pack(const uint16_t *src, int ld, int N, int K, uint8_t *dst,
                                   float *scales, int tile_step, int tile_offset, int pitch,
                                   hipStream_t s) {
  if (N <= 0 || K <= 0 || K % 64 || ld % 8) return hipErrorInvalidValue;
  hipLaunchKernelGGL(w8_quantize_pack_kernel, dim3((N + 15) / 16), dim3(256), 0, s, src, ld, N, K,
                     dst, scales, tile_step, tile_offset, pitch);
  return hipGetLastError();
}

hipError_t launch_w8_unpack(const uint8_t *src, int N, int K, uint8_t *dst, int tile_step,
                            int tile_offset, int pitch, hipStream_t s) {
  if (N <= 0 || K <= 0 || K % 64) return hipErrorInvalidValue;
  const long total = (long)N * K;
  hipLaunchKernelGGL(w8_unpack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, src,
                     N, K, dst, tile_step, tile_offset, pitch);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Plan: tiles, n-tile groups (gridDim.x) and k-slices (gridDim.y).  S depends
// on (N, K, epilogue) only, so a row's bits do not depend on the batch around
// it.  gate/up (N to spare, and its epilogue needs whole sums) is never split;
// otherwise K is split until the grid holds about one workgroup per CU, a
// slice keeping at least kW8MinSteps double steps, and no slice is empty.
// ---------------------------------------------------------------------------
W8Plan plan_w8(int N, int K, int epilogue) {
  W8Plan p;
  const bool silu = (epilogue & 0xf) == FFMI_EPI_SILU_MUL;
  p.ntiles = (silu ? 2 : 1) * ((N + 15) / 16);
  p.nblk = (p.ntiles + 4 * kW8NT - 1) / (4 * kW8NT);
  p.KT2 = K / 64;
  p.S = 1;
  if (!silu) {
    const int want = kW8Groups / p.nblk;  // (rounded down: 250 groups stay unsplit)
    const int S = std::max(1, std::min({want, kW8MaxS, p.KT2 / kW8MinSteps}));
    const int per = (p.KT2 + S - 1) / S;
    p.S = (p.KT2 + per - 1) / per;
  }
  return p;
}

size_t gemm_w8_workspace_bytes(int T, int N, int K, int epilogue) {
  if (T <= 0 || N <= 0 || K <= 0 || K % 64) return 0;
  const W8Plan p = plan_w8(N, K, epilogue);
  return p.S > 1 ? (size_t)p.S * std::min(T, kW8Rows) * p.ntiles * 16 * sizeof(float) : 0;
}

template <int MT>
static void launch_w8_rows(const W8Plan &p, bool silu, bool ntl, const uint16_t *X,
                           const uint8_t *W8, const float *scales, uint16_t *Y, float *ws, int T,
                           int N, int K, hipStream_t s) {
  const dim3 grid(p.nblk, p.S), block(256);
#define FFMI_W8(EPI, NTL)                                                                      \
  hipLaunchKernelGGL((gemm_w8_kernel<MT, EPI, NTL>), grid, block, 0, s, X, W8, scales, Y, ws, T, \
                     N, K, p.KT2, p.ntiles, p.ntiles)
  if (silu && ntl) FFMI_W8(1, true);
  else if (silu) FFMI_W8(1, false);
  else if (ntl) FFMI_W8(0, true);
  else FFMI_W8(0, false);
#undef FFMI_W8
}

size_t gemm_w8_onepass_workspace_bytes(int T, int N, int K, int epilogue) {
  if (T <= 0 || N <= 0 || K <= 0 || K % 64) return 0;
  const W8Plan p = plan_w8(N, K, epilogue);
  return p.S > 1 ? (size_t)p.S * std::min(T, kW8MidRows) * p.ntiles * 16 * sizeof(float) : 0;
}

// FFMI_W8_MULTIPASS=1: rows above 64 keep one skinny pass per 64 rows, whatever
// the workspace (A/B against the M-split kernel in one build); once
static bool sw_w8_multipass() {
  static const bool v = [] { const char *e = getenv("FFMI_W8_MULTIPASS"); return e && atoi(e) != 0; }();
  return v;
}

// The launch plan: what launch_gemm_w8 does and ffmi_debug_linear_w8_plan
// reports.  Above 64 rows the M-split kernel (gemm_w8_mid.hip) covers 256 rows
// per weight pass where the workspace holds its slabs (a shape that does not
// split K needs none); a split shape given only the minimum, the skinny
// kernel's 64 rows of slabs, keeps one skinny pass per 64 rows -- as plan_gemm
// un-splits a plan whose workspace is missing.  The bits are the same.
W8Launch plan_w8_launch(int T, int N, int K, int epilogue, size_t ws_bytes) {
  W8Launch l;
  const W8Plan p = plan_w8(N, K, epilogue);
  l.path = T > kW8Rows && !sw_w8_multipass() &&
           ws_bytes >= gemm_w8_onepass_workspace_bytes(T, N, K, epilogue);
  l.rows = l.path ? kW8MidRows : kW8Rows;
  const int mt = (std::min(T, l.rows) + 15) / 16;  // m-tiles of the first pass
  l.MTW = l.path ? std::max(2, (mt + 3) / 4) : mt;
  l.NTW = l.path ? kW8MidNTW : kW8NT;
  l.S = p.S, l.passes = (T + l.rows - 1) / l.rows, l.nblk = p.nblk;
  return l;
}

// One launch per l.rows rows: the M-split kernel for a pass of more than 64
// rows, the skinny kernel for a shorter (last) one
hipError_t launch_gemm_w8(const uint16_t *X, const uint8_t *W8, const float *scales, uint16_t *Y,
                          float *ws, size_t ws_bytes, int T, int N, int K, int epilogue,
                          hipStream_t s) {
  if (T <= 0) return hipSuccess;
  if (N <= 0 || K <= 0 || K % 64 || (epilogue & (FFMI_X_PACKED | FFMI_Y_PACKED)))
    return hipErrorInvalidValue;
  const int base = epilogue & ~FFMI_W_STREAM;
  if (base != FFMI_EPI_NONE && base != FFMI_EPI_SILU_MUL) return hipErrorInvalidValue;
  const W8Plan p = plan_w8(N, K, epilogue);
  if (p.S > 1 && (!ws || ws_bytes < gemm_w8_workspace_bytes(T, N, K, epilogue)))
    return hipErrorInvalidValue;
  const W8Launch l = plan_w8_launch(T, N, K, epilogue, ws ? ws_bytes : 0);
  const bool silu = base == FFMI_EPI_SILU_MUL, ntl = (epilogue & FFMI_W_STREAM) != 0;
  for (int t0 = 0; t0 < T; t0 += l.rows) {
    const int Tp = std::min(l.rows, T - t0), mt = (Tp + 15) / 16;
    const uint16_t *Xp = X + (size_t)t0 * K;
    uint16_t *Yp = Y + (size_t)t0 * N;
    if (Tp > kW8Rows) {
      launch_w8_mid_rows(p, std::max(2, (mt + 3) / 4), silu, ntl, Xp, W8, scales, Yp, ws, Tp, N, K,
                         s);
    } else {
      switch (mt) {
        case 1: launch_w8_rows<1>(p, silu, ntl, Xp, W8, scales, Yp, ws, Tp, N, K, s); break;
        case 2: launch_w8_rows<2>(p, silu, ntl, Xp, W8, scales, Yp, ws, Tp, N, K, s); break;
        case 3: launch_w8_rows<3>(p, silu, ntl, Xp, W8, scales, Yp, ws, Tp, N, K, s); break;
        default: launch_w8_rows<4>(p, silu, ntl, Xp, W8, scales, Yp, ws, Tp, N, K, s); break;
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
