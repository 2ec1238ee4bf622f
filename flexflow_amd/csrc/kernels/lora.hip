// lora.hip -- LoRA update of a projection output, per-row adapters (gfx950).
//
// The reference's LoraLinear inference path (lora_linear_kernels.cu:174-278):
// per request two small GEMMs, h = x A^T held in the activation type, then
// y += scaling * h B^T in place.  Here one pair of launches serves a whole
// mixed batch: every row names its adapter through slots[t] (-1: none), read
// on the device so that a replayed graph sees fresh assignments.
//
//   shrink      h_part[c][t][j] = sum over part c of F of x[t][k] A[j][k]
//               (MFMA, fp32).  F is cut into kLoraChunk-column parts, fixed by
//               F alone; one workgroup per (part, 16-row tile), one wave per
//               16 ranks.  A tile whose rows name several adapters runs the
//               part once per adapter present and keeps, per row, the result
//               of the row's own adapter: an MFMA output element depends on
//               its own row and column only, so a row's bits do not depend on
//               its neighbours.
//   expand-add  h[t][j] = fp16(sum of the parts in part order), then
//               y[t][n] = fp16(float(y) + scale * sum_j h[t][j] B[n][j]),
//               j in order, fp32, one thread per output column; a run of rows
//               of one adapter keeps its B row in registers.
//
// The qkv site (ffmi_lora_apply_qkv) is the same pair over three modules at
// once: y is the fused row [Q | K | V] and every segment has its own table.
//   shrink      the same kernel, instantiated with the segment as the grid's z: it writes
//               h_part[segment][part][t][j] from the segment's table.
//   expand-add  over the 256-column blocks of the whole row: a column finds
//               its segment and takes that segment's h, B and scale, so a
//               block that straddles a boundary serves both sides.  A row whose
//               adapter lacks a segment's module is not written there.
#include "../ffmi_internal.h"

namespace ffmi {

namespace {

constexpr int kLoraChunk = 256;  // columns of F per part
constexpr int kLoraR = FFMI_LORA_MAX_RANK;

// the row's adapter, or -1 (none, out of range, not loaded)
__device__ __forceinline__ int lora_slot(const int32_t *slots, const ffmi_lora_entry *table, int row,
                                         int T) {
  if (row >= T) return -1;
  const int a = slots[row];
  if (a < 0 || a >= FFMI_LORA_MAX_ADAPTERS) return -1;
  return table[a].A && table[a].B ? a : -1;
}

__device__ __forceinline__ int lora_rank16(const ffmi_lora_entry &e) {
  return min(kLoraR, (max(e.rank, 1) + 15) & ~15);
}

// the tables of a launch: one, or the qkv site's three (q, k, v)
struct LoraTables {
  const ffmi_lora_entry *t[3];
};

// the shrink's table argument: the one table of ffmi_lora_apply, or the three
// of the qkv site
template <bool SEG> struct LoraTableArg { typedef const ffmi_lora_entry *__restrict__ type; };
template <> struct LoraTableArg<true> { typedef LoraTables type; };

// SEG = false: the kernel of ffmi_lora_apply, its arguments and code as they
// were before the qkv site came.  SEG = true (the qkv site): one table and one
// [part][T][64] block of the workspace per segment, the grid's z.
template <bool SEG>
__global__ __launch_bounds__(256) void lora_shrink_kernel(const uint16_t *__restrict__ x, int T,
                                                          int F, const int32_t *__restrict__ slots,
                                                          typename LoraTableArg<SEG>::type tab,
                                                          float *__restrict__ part, int x_packed) {
  const ffmi_lora_entry *__restrict__ table;
  if constexpr (SEG) {
    table = blockIdx.z == 0 ? tab.t[0] : blockIdx.z == 1 ? tab.t[1] : tab.t[2];
    part += (size_t)blockIdx.z * gridDim.x * T * kLoraR;
  } else {
    table = tab;
  }
  const int c = blockIdx.x, tile = blockIdx.y;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int KT = F >> 5;
  const int kt0 = c * (kLoraChunk / 32), kt1 = min(KT, kt0 + kLoraChunk / 32);
  const int row = tile * 16 + (lane & 15);  // the token this lane's MFMA column is
  const int a_row = lora_slot(slots, table, row, T);
  unsigned present = 0;
  for (int i = 0; i < 16; ++i) {
    const int a = __shfl(a_row, i);
    if (a >= 0) present |= 1u << a;
  }
  for (int a = 0; a < FFMI_LORA_MAX_ADAPTERS; ++a) {
    if (!((present >> a) & 1u)) continue;
    const ffmi_lora_entry e = table[a];
    if (wave * 16 >= lora_rank16(e)) continue;  // (ranks of this wave: zero padding)
    const uint16_t *A = static_cast<const uint16_t *>(e.A);
    f4 acc = {0.f, 0.f, 0.f, 0.f};
    // the part's fragments are all loaded before the first MFMA (one memory
    // round trip, not one per k-step); steps past the end of F load nothing
    constexpr int NS = kLoraChunk / 32;
    h8 xf[NS], af[NS];
#pragma unroll
    for (int u = 0; u < NS; ++u) {
      const int kt = kt0 + u;
      xf[u] = af[u] = h8{0, 0, 0, 0, 0, 0, 0, 0};
      if (kt >= kt1) continue;
      if (x_packed)
        xf[u] = *reinterpret_cast<const h8 *>(x + (((size_t)tile * KT + kt) * 64 + lane) * 8);
      else if (row < T)
        xf[u] = *reinterpret_cast<const h8 *>(x + (size_t)row * F + kt * 32 + 8 * (lane >> 4));
      af[u] = *reinterpret_cast<const h8 *>(A + (((size_t)wave * KT + kt) * 64 + lane) * 8);
    }
#pragma unroll
    for (int u = 0; u < NS; ++u)  // (uniform: kt1 depends on the part only)
      // D = A . x^T: this lane holds ranks wave * 16 + 4 * (lane >> 4) + 0..3 of token lane & 15
      if (kt0 + u < kt1) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[u], xf[u], acc, 0, 0, 0);
    if (a_row == a)
      *reinterpret_cast<f4 *>(part + ((size_t)c * T + row) * kLoraR + wave * 16 + 4 * (lane >> 4)) =
          acc;
  }
}

// h of 16 rows into LDS: the parts in part order, rounded to fp16 (0 for a row
// without an adapter and beyond the rank); sa[tr] the row's adapter or -1
__device__ __forceinline__ void lora_finish_h(const float *__restrict__ part, int nch, int T,
                                              int tile, const int32_t *__restrict__ slots,
                                              const ffmi_lora_entry *__restrict__ table,
                                              float (*hs)[kLoraR], int *sa, uint16_t *h_out) {
  for (int idx = threadIdx.x; idx < 16 * kLoraR; idx += 256) {
    const int tr = idx / kLoraR, j = idx % kLoraR;
    const int row = tile * 16 + tr;
    const int a = lora_slot(slots, table, row, T);
    float hv = 0.f;
    if (a >= 0) {
      __half hh = __float2half_rn(0.f);
      if (j < lora_rank16(table[a])) {
        // the parts in part order, eight loads in flight at a time
        const float *p = part + (size_t)row * kLoraR + j;
        const size_t stride = (size_t)T * kLoraR;
        float sum = 0.f;
        for (int c0 = 0; c0 < nch; c0 += 8) {
          float v[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) v[u] = c0 + u < nch ? p[(size_t)(c0 + u) * stride] : 0.f;
#pragma unroll
          for (int u = 0; u < 8; ++u)
            if (c0 + u < nch) sum += v[u];
        }
        hh = __float2half_rn(sum);
      }
      hv = __half2float(hh);
      if (h_out) h_out[(size_t)row * kLoraR + j] = __half_as_ushort(hh);
    }
    hs[tr][j] = hv;
    if (j == 0) sa[tr] = a;
  }
}

__global__ __launch_bounds__(256) void lora_expand_kernel(const float *__restrict__ part, int nch,
                                                          int T, int H,
                                                          const int32_t *__restrict__ slots,
                                                          const ffmi_lora_entry *__restrict__ table,
                                                          uint16_t *__restrict__ y,
                                                          uint16_t *__restrict__ h_out) {
  __shared__ float hs[16][kLoraR];
  __shared__ int sa[16];
  const int tile = blockIdx.y;
  // (the body of lora_finish_h, kept in line here: this kernel is the one
  // ffmi_lora_apply has always launched, instruction for instruction)
  for (int idx = threadIdx.x; idx < 16 * kLoraR; idx += 256) {
    const int tr = idx / kLoraR, j = idx % kLoraR;
    const int row = tile * 16 + tr;
    const int a = lora_slot(slots, table, row, T);
    float hv = 0.f;
    if (a >= 0) {
      __half hh = __float2half_rn(0.f);
      if (j < lora_rank16(table[a])) {
        // the parts in part order, eight loads in flight at a time
        const float *p = part + (size_t)row * kLoraR + j;
        const size_t stride = (size_t)T * kLoraR;
        float sum = 0.f;
        for (int c0 = 0; c0 < nch; c0 += 8) {
          float v[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) v[u] = c0 + u < nch ? p[(size_t)(c0 + u) * stride] : 0.f;
#pragma unroll
          for (int u = 0; u < 8; ++u)
            if (c0 + u < nch) sum += v[u];
        }
        hh = __float2half_rn(sum);
      }
      hv = __half2float(hh);
      if (h_out && blockIdx.x == 0) h_out[(size_t)row * kLoraR + j] = __half_as_ushort(hh);
    }
    hs[tr][j] = hv;
    if (j == 0) sa[tr] = a;
  }
  __syncthreads();
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= H) return;
  int cur = -1;
  float scale = 0.f;
  h8 b[kLoraR / 8];
  for (int tr = 0; tr < 16; ++tr) {
    const int a = sa[tr];
    if (a < 0) continue;
    if (a != cur) {  // (rows of one request are contiguous: one B row per run)
      const ffmi_lora_entry e = table[a];
      const h8 *B = reinterpret_cast<const h8 *>(static_cast<const uint16_t *>(e.B) +
                                                 (size_t)n * kLoraR);
#pragma unroll
      for (int q = 0; q < kLoraR / 8; ++q) b[q] = B[q];
      scale = e.scale;
      cur = a;
    }
    float d = 0.f;
#pragma unroll
    for (int q = 0; q < kLoraR / 8; ++q)
#pragma unroll
      for (int i = 0; i < 8; ++i) d += hs[tr][q * 8 + i] * (float)b[q][i];
    uint16_t *yp = y + (size_t)(tile * 16 + tr) * H + n;
    const float yv = __half2float(__ushort_as_half(*yp));
    *yp = __half_as_ushort(__float2half_rn(yv + scale * d));
  }
}

// the qkv site's expand-add: y [T][ldy] holds [Q | K | V], w0 / w1 / w2 wide;
// one table per segment, part [3][nch][T][64], h_out [3][T][64]
__global__ __launch_bounds__(256) void lora_expand_qkv_kernel(
    const float *__restrict__ part, int nch, int T, int w0, int w1, int w2, int ldy,
    const int32_t *__restrict__ slots, LoraTables tables, uint16_t *__restrict__ y,
    uint16_t *__restrict__ h_out) {
  __shared__ float hs[3][16][kLoraR];
  __shared__ int sa[3][16];
  const int tile = blockIdx.y;
  const int c0 = blockIdx.x * 256, c1 = c0 + 256;  // this block's columns of the row
  const int beg[3] = {0, w0, w0 + w1}, end[3] = {w0, w0 + w1, w0 + w1 + w2};
#pragma unroll
  for (int g = 0; g < 3; ++g) {
    if (end[g] <= c0 || beg[g] >= c1) continue;  // (uniform: the block has no column of it)
    // h_out of a segment comes from the block that holds the segment's first column
    lora_finish_h(part + (size_t)g * nch * T * kLoraR, nch, T, tile, slots,
                  tables.t[g], hs[g], sa[g],
                  h_out && beg[g] >= c0 ? h_out + (size_t)g * T * kLoraR : nullptr);
  }
  __syncthreads();
  const int n = c0 + threadIdx.x;
  if (n >= end[2]) return;
  const int g = n < end[0] ? 0 : n < end[1] ? 1 : 2;
  const int nl = n - (g == 0 ? 0 : g == 1 ? w0 : w0 + w1);  // the column within its module
  const ffmi_lora_entry *table = g == 0 ? tables.t[0] : g == 1 ? tables.t[1] : tables.t[2];
  int cur = -1;
  float scale = 0.f;
  h8 b[kLoraR / 8];
  for (int tr = 0; tr < 16; ++tr) {
    const int a = sa[g][tr];
    if (a < 0) continue;
    if (a != cur) {
      const ffmi_lora_entry e = table[a];
      const h8 *B = reinterpret_cast<const h8 *>(static_cast<const uint16_t *>(e.B) +
                                                 (size_t)nl * kLoraR);
#pragma unroll
      for (int q = 0; q < kLoraR / 8; ++q) b[q] = B[q];
      scale = e.scale;
      cur = a;
    }
    float d = 0.f;
#pragma unroll
    for (int q = 0; q < kLoraR / 8; ++q)
#pragma unroll
      for (int i = 0; i < 8; ++i) d += hs[g][tr][q * 8 + i] * (float)b[q][i];
    uint16_t *yp = y + (size_t)(tile * 16 + tr) * ldy + n;
    const float yv = __half2float(__ushort_as_half(*yp));
    *yp = __half_as_ushort(__float2half_rn(yv + scale * d));
  }
}

}  // namespace

size_t lora_workspace_bytes(int T, int F) {
  if (T <= 0 || F <= 0) return 0;
  return (size_t)((F + kLoraChunk - 1) / kLoraChunk) * (size_t)T * kLoraR * sizeof(float);
}

hipError_t launch_lora(const uint16_t *x, int T, int F, int H, const int32_t *slots,
                       const ffmi_lora_entry *table, uint16_t *y, bool x_packed, float *ws,
                       uint16_t *h_out, hipStream_t s) {
  if (T <= 0) return hipSuccess;
  const int nch = (F + kLoraChunk - 1) / kLoraChunk, tiles = (T + 15) / 16;
  lora_shrink_kernel<false><<<dim3(nch, tiles), 256, 0, s>>>(x, T, F, slots, table, ws,
                                                             x_packed ? 1 : 0);
  lora_expand_kernel<<<dim3((H + 255) / 256, tiles), 256, 0, s>>>(ws, nch, T, H, slots, table, y,
                                                                  h_out);
  return hipGetLastError();
}

hipError_t launch_lora_qkv(const uint16_t *x, int T, int F, const int *w, int ldy,
                           const int32_t *slots, const ffmi_lora_entry *const *tables,
                           uint16_t *y, bool x_packed, float *ws, uint16_t *h_out,
                           hipStream_t s) {
  if (T <= 0) return hipSuccess;
  const LoraTables tb{{tables[0], tables[1], tables[2]}};
  const int nch = (F + kLoraChunk - 1) / kLoraChunk, tiles = (T + 15) / 16;
  lora_shrink_kernel<true><<<dim3(nch, tiles, 3), 256, 0, s>>>(x, T, F, slots, tb, ws,
                                                               x_packed ? 1 : 0);
  lora_expand_qkv_kernel<<<dim3((w[0] + w[1] + w[2] + 255) / 256, tiles), 256, 0, s>>>(
      ws, nch, T, w[0], w[1], w[2], ldy, slots, tb, y, h_out);
  return hipGetLastError();
}

}  // namespace ffmi
