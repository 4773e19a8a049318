// QK-norm attention prologue (Qwen3 / OLMo-2 / Gemma-3): per-head RMSNorm of
// Q and of K followed by rotate-half RoPE, forward and backward, bf16 in and
// out, fp32 arithmetic, one rounding at the store.
//
//   inv = rsqrt(mean(x^2) + eps)          n = x * inv * w
//   y[:D/2] = n1*cos[p] - n2*sin[p]       y[D/2:] = n2*cos[p] + n1*sin[p]
//
// cos/sin are the host fp32 [max_pos, D/2] tables of rope.hip.
//
// Work split. The unit of work is a head row: the nh + nkv head vectors of a
// token, flattened over tokens, Q heads first. D/16 lanes own one head row
// (8 lanes for D=128, 4 for D=64); lane j holds x[8j, 8j+8) and
// x[D/2+8j, D/2+8j+8) as two b128 loads, so both members of every rotation
// pair sit in one lane and the rotation needs no cross-lane traffic. The sum
// of squares (forward) and the dot product (backward) are DPP reductions
// inside the lane group: two quad permutes, plus a half-row mirror for the
// 8-lane group. A 256-thread block takes 32 (D=128) or 64 (D=64) head rows
// per iteration of a grid-stride loop over row groups; the grid is capped at
// 2048 blocks like the other memory-bound kernels. Tail rows are predicated
// at the loads and stores: every lane reaches every DPP op and barrier.
//
// q and k are read in place from wherever they live (the slices of the
// packed QKV projection): each has its own base pointer and token stride,
// heads*D contiguous inside a token, as rope_oop_kernel addresses its source.
//
// cos/sin: a token's table row is shared by its nh + nkv head rows.
// The kernels read it straight from global memory and rely on the caches: a
// wave's 8 or 16 head rows almost always belong to one token, so its table
// loads touch the same two cache lines per table. Measured that way the
// forward moves 5.7 TB/s and the backward 5.0 TB/s at T=8192, nh=32, nkv=8,
// D=128 (profiles/qk_norm_rope.txt), where HBM is the bound; staging the
// rows in LDS once per block was not built, so it has no measurement.
//
// Backward. g = inverse rotation of dy (in-lane), dot = sum(g*w*x) over the
// lane group, dx = g*w*inv - x*dot*inv^3/D. The weight gradient
// dw = sum_rows g*x*inv accumulates in registers across a thread's
// grid-stride iterations (its column set is fixed by its lane-in-group
// index; Q and K rows have separate accumulators). At block end the threads
// that share a column set combine through LDS in a fixed order and the block
// writes its own [2, D] fp32 slice with plain stores; qk_norm_dw_kernel then
// sums the slices in a fixed order and casts to bf16. No floating-point
// atomics: dwq/dwk are bit-identical from run to run.
#include "kern_common.h"

// Packed fp32 arithmetic is kept out of this file's device code. A function
// whose target features differ from its caller's is called, not inlined,
// unless it is __forceinline__: the device code below uses builtins and
// kern_common.h's __forceinline__ helpers, not the runtime header's plain
// inline functions (rsqrtf, __shfl_xor, __syncthreads, ...).
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#define QKNR_THREADS 256
#define QKNR_MAX_BLOCKS 2048
#define QKNR_DW_COLS 32     // columns per block of the dw reduction
#define QKNR_DW_STRIPES 32  // slice stripes per block of the dw reduction

namespace {

__device__ __forceinline__ void block_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) {
  union { int i; float f; } a, b;
  a.f = v;
  b.i = __builtin_amdgcn_update_dpp(0, a.i, CTRL, 0xF, 0xF, true);
  return b.f;
}

// Sum over the LPR consecutive lanes of a head row; every lane of the group
// ends with the same bits. 0xB1 = quad_perm [1,0,3,2], 0x4E = quad_perm
// [2,3,0,1], 0x141 = row_half_mirror (lane i <-> 7 - i of each 8; after the
// two quad steps a quad is uniform, so the mirror brings in the other quad).
template <int LPR>
__device__ __forceinline__ float group_sum(float v) {
  v += dpp_f32<0xB1>(v);
  v += dpp_f32<0x4E>(v);
  if (LPR == 8) v += dpp_f32<0x141>(v);
  return v;
}

__device__ __forceinline__ void load8f(const float* p, float out[8]) {
  const float4_t a = reinterpret_cast<const float4_t*>(p)[0];
  const float4_t b = reinterpret_cast<const float4_t*>(p)[1];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    out[e] = a[e];
    out[4 + e] = b[e];
  }
}

// Which head row this lane group works on in row group `grp`.
template <int D>
struct HeadRow {
  bool ok, is_q;
  int t;   // token
  int hh;  // head index within q or within k
  __device__ __forceinline__ HeadRow(long long grp, int n_rows, int nh,
                                     int nkv) {
    constexpr int LPR = D / 16;
    const long long r = grp * (QKNR_THREADS / LPR) + threadIdx.x / LPR;
    ok = r < n_rows;
    const int ri = ok ? (int)r : 0;
    const int ht = nh + nkv;
    t = ri / ht;
    const int h = ri - t * ht;
    is_q = h < nh;
    hh = is_q ? h : h - nh;
  }
};

// cos/sin of position pos[t % n_pos], columns [8j, 8j+8)
template <int D>
__device__ __forceinline__ void load_tables(
    const int* __restrict__ pos, const float* __restrict__ cos_tab,
    const float* __restrict__ sin_tab, int t, int n_pos, int j, float c[8],
    float s[8]) {
  const long long off = (long long)pos[t % n_pos] * (D / 2) + 8 * j;
  load8f(cos_tab + off, c);
  load8f(sin_tab + off, s);
}

template <int D>
__global__ __launch_bounds__(QKNR_THREADS) void qk_norm_rope_fwd_kernel(
    const short* __restrict__ xq, const short* __restrict__ xk,
    long long q_stride, long long k_stride, const short* __restrict__ wq,
    const short* __restrict__ wk, const int* __restrict__ pos,
    const float* __restrict__ cos_tab, const float* __restrict__ sin_tab,
    short* __restrict__ q_out, short* __restrict__ k_out,
    float* __restrict__ inv_out, int n_rows, int n_pos, int nh, int nkv,
    float eps) {
  constexpr int LPR = D / 16;
  constexpr int ROWS = QKNR_THREADS / LPR;
  const int j = threadIdx.x % LPR;
  // both weights stay packed (16 VGPRs); the row's one is widened per use
  const short8_t wq1 = *reinterpret_cast<const short8_t*>(wq + 8 * j);
  const short8_t wq2 = *reinterpret_cast<const short8_t*>(wq + D / 2 + 8 * j);
  const short8_t wk1 = *reinterpret_cast<const short8_t*>(wk + 8 * j);
  const short8_t wk2 = *reinterpret_cast<const short8_t*>(wk + D / 2 + 8 * j);
  const long long n_groups = ((long long)n_rows + ROWS - 1) / ROWS;
  for (long long grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
    const HeadRow<D> row(grp, n_rows, nh, nkv);
    const short* src =
        row.is_q ? xq + row.t * q_stride + (long long)row.hh * D
                 : xk + row.t * k_stride + (long long)row.hh * D;
    short* dst = row.is_q
                     ? q_out + ((long long)row.t * nh + row.hh) * D
                     : k_out + ((long long)row.t * nkv + row.hh) * D;
    float x1[8], x2[8], c[8], s[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) x1[e] = x2[e] = c[e] = s[e] = 0.f;
    if (row.ok) {
      load8(src + 8 * j, x1);
      load8(src + D / 2 + 8 * j, x2);
      load_tables<D>(pos, cos_tab, sin_tab, row.t, n_pos, j, c, s);
    }
    const short8_t w1 = row.is_q ? wq1 : wk1;
    const short8_t w2 = row.is_q ? wq2 : wk2;
    float ssq = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) ssq += x1[e] * x1[e] + x2[e] * x2[e];
    ssq = group_sum<LPR>(ssq);
    const float inv = __builtin_amdgcn_rsqf(ssq * (1.f / D) + eps);
    float o1[8], o2[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float n1 = x1[e] * inv * bf2f(w1[e]);
      const float n2 = x2[e] * inv * bf2f(w2[e]);
      o1[e] = n1 * c[e] - n2 * s[e];
      o2[e] = n2 * c[e] + n1 * s[e];
    }
    if (row.ok) {
      store8(dst + 8 * j, o1);
      store8(dst + D / 2 + 8 * j, o2);
      if (j == 0) inv_out[grp * ROWS + threadIdx.x / LPR] = inv;
    }
  }
}

template <int D>
__global__ __launch_bounds__(QKNR_THREADS) void qk_norm_rope_bwd_kernel(
    const short* __restrict__ dyq, const short* __restrict__ dyk,
    long long dyq_stride, long long dyk_stride,
    const short* __restrict__ xq, const short* __restrict__ xk,
    long long q_stride, long long k_stride, const float* __restrict__ inv_in,
    const short* __restrict__ wq, const short* __restrict__ wk,
    const int* __restrict__ pos, const float* __restrict__ cos_tab,
    const float* __restrict__ sin_tab, short* __restrict__ dxq,
    short* __restrict__ dxk, float* __restrict__ dw_partial, int n_rows,
    int n_pos, int nh, int nkv) {
  constexpr int LPR = D / 16;
  constexpr int ROWS = QKNR_THREADS / LPR;
  // red[a][tid]: consecutive threads hit consecutive banks
  __shared__ float red[16][QKNR_THREADS];
  const int j = threadIdx.x % LPR;
  // both weights stay packed (16 VGPRs); the row's one is widened per use
  const short8_t wq1 = *reinterpret_cast<const short8_t*>(wq + 8 * j);
  const short8_t wq2 = *reinterpret_cast<const short8_t*>(wq + D / 2 + 8 * j);
  const short8_t wk1 = *reinterpret_cast<const short8_t*>(wk + 8 * j);
  const short8_t wk2 = *reinterpret_cast<const short8_t*>(wk + D / 2 + 8 * j);
  // acc[0] = dwq, acc[1] = dwk; [.][e] columns 8j+e, [.][8+e] D/2+8j+e
  float acc[2][16];
#pragma unroll
  for (int a = 0; a < 16; ++a) acc[0][a] = acc[1][a] = 0.f;
  const long long n_groups = ((long long)n_rows + ROWS - 1) / ROWS;
  for (long long grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
    const HeadRow<D> row(grp, n_rows, nh, nkv);
    const long long in_head = (long long)row.hh * D;
    const short* dys = row.is_q ? dyq + row.t * dyq_stride + in_head
                                : dyk + row.t * dyk_stride + in_head;
    const short* xs = row.is_q ? xq + row.t * q_stride + in_head
                               : xk + row.t * k_stride + in_head;
    short* dst = row.is_q ? dxq + ((long long)row.t * nh + row.hh) * D
                          : dxk + ((long long)row.t * nkv + row.hh) * D;
    float dy1[8], dy2[8], x1[8], x2[8], c[8], s[8];
#pragma unroll
    for (int e = 0; e < 8; ++e)
      dy1[e] = dy2[e] = x1[e] = x2[e] = c[e] = s[e] = 0.f;
    float inv = 0.f;
    if (row.ok) {
      load8(dys + 8 * j, dy1);
      load8(dys + D / 2 + 8 * j, dy2);
      load8(xs + 8 * j, x1);
      load8(xs + D / 2 + 8 * j, x2);
      load_tables<D>(pos, cos_tab, sin_tab, row.t, n_pos, j, c, s);
      inv = inv_in[grp * ROWS + threadIdx.x / LPR];
    }
    // a tail row has dy = x = inv = 0: it adds exact zeros below
    const short8_t w1 = row.is_q ? wq1 : wk1;
    const short8_t w2 = row.is_q ? wq2 : wk2;
    float gw1[8], gw2[8];
    float dot = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float g1 = dy1[e] * c[e] + dy2[e] * s[e];
      const float g2 = dy2[e] * c[e] - dy1[e] * s[e];
      const float a1 = g1 * x1[e] * inv;
      const float a2 = g2 * x2[e] * inv;
      acc[0][e] += row.is_q ? a1 : 0.f;
      acc[0][8 + e] += row.is_q ? a2 : 0.f;
      acc[1][e] += row.is_q ? 0.f : a1;
      acc[1][8 + e] += row.is_q ? 0.f : a2;
      gw1[e] = g1 * bf2f(w1[e]);
      gw2[e] = g2 * bf2f(w2[e]);
      dot += gw1[e] * x1[e] + gw2[e] * x2[e];
    }
    dot = group_sum<LPR>(dot);
    const float kx = dot * inv * inv * inv * (1.f / D);
    float o1[8], o2[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      o1[e] = gw1[e] * inv - x1[e] * kx;
      o2[e] = gw2[e] * inv - x2[e] * kx;
    }
    if (row.ok) {
      store8(dst + 8 * j, o1);
      store8(dst + D / 2 + 8 * j, o2);
    }
  }
  // block combine, Q then K through the same 16 KB: thread `col` sums the
  // ROWS threads that own column `col`, in thread order
  float* slice = dw_partial + (long long)blockIdx.x * 2 * D;
#pragma unroll
  for (int which = 0; which < 2; ++which) {
#pragma unroll
    for (int a = 0; a < 16; ++a) red[a][threadIdx.x] = acc[which][a];
    block_sync();
    if (threadIdx.x < D) {
      const int col = threadIdx.x;
      const int hi = col >= D / 2;
      const int cc = col - hi * (D / 2);
      const float* src = &red[hi * 8 + (cc & 7)][cc >> 3];
      float sum = 0.f;
      for (int i = 0; i < ROWS; ++i) sum += src[i * LPR];
      slice[which * D + col] = sum;
    }
    block_sync();
  }
}

// dw_partial [n_slices, 2*D] fp32 -> dwq [D], dwk [D] bf16. A block takes 32
// columns; its 32 stripes each sum every 32nd slice in slice order, then the
// stripes combine in stripe order: fixed order, no atomics.
__global__ __launch_bounds__(QKNR_DW_COLS * QKNR_DW_STRIPES)
void qk_norm_dw_kernel(const float* __restrict__ dw_partial,
                       short* __restrict__ dwq, short* __restrict__ dwk,
                       int n_slices, int d) {
  __shared__ float red[QKNR_DW_STRIPES][QKNR_DW_COLS + 1];
  const int cl = threadIdx.x % QKNR_DW_COLS;
  const int stripe = threadIdx.x / QKNR_DW_COLS;
  const int col = blockIdx.x * QKNR_DW_COLS + cl;  // < 2*d: 2*d % 32 == 0
  float sum = 0.f;
#pragma unroll 8
  for (int p = stripe; p < n_slices; p += QKNR_DW_STRIPES)
    sum += dw_partial[(long long)p * 2 * d + col];
  red[stripe][cl] = sum;
  block_sync();
  if (stripe == 0) {
    float total = 0.f;
    for (int i = 0; i < QKNR_DW_STRIPES; ++i) total += red[i][cl];
    if (col < d)
      dwq[col] = f2bf(total);
    else
      dwk[col - d] = f2bf(total);
  }
}

int qknr_grid(long long n_rows, int d) {
  const int rows = QKNR_THREADS / (d / 16);
  long long g = (n_rows + rows - 1) / rows;
  if (g > QKNR_MAX_BLOCKS) g = QKNR_MAX_BLOCKS;
  return g < 1 ? 1 : (int)g;
}

}  // namespace

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

extern "C" {

// number of [2, D] fp32 slices the backward writes (= its grid)
int qk_norm_rope_bwd_slices(long long n_rows, int head_dim) {
  return qknr_grid(n_rows, head_dim);
}

void qk_norm_rope_fwd_launch(
    const void* xq, const void* xk, long long q_stride, long long k_stride,
    const void* wq, const void* wk, const void* pos, const void* cos_tab,
    const void* sin_tab, void* q_out, void* k_out, void* inv, int n_tokens,
    int n_pos, int nh, int nkv, int head_dim, float eps, hipStream_t stream) {
  const int n_rows = n_tokens * (nh + nkv);
  const dim3 grid(qknr_grid(n_rows, head_dim)), block(QKNR_THREADS);
#define QKNR_FWD(DD)                                                         \
  hipLaunchKernelGGL((qk_norm_rope_fwd_kernel<DD>), grid, block, 0, stream,  \
                     (const short*)xq, (const short*)xk, q_stride, k_stride, \
                     (const short*)wq, (const short*)wk, (const int*)pos,    \
                     (const float*)cos_tab, (const float*)sin_tab,           \
                     (short*)q_out, (short*)k_out, (float*)inv, n_rows,      \
                     n_pos, nh, nkv, eps)
  if (head_dim == 128)
    QKNR_FWD(128);
  else
    QKNR_FWD(64);
#undef QKNR_FWD
}

// dw_partial: [qk_norm_rope_bwd_slices(), 2, head_dim] fp32 scratch
void qk_norm_rope_bwd_launch(
    const void* dyq, const void* dyk, long long dyq_stride,
    long long dyk_stride, const void* xq, const void* xk, long long q_stride,
    long long k_stride, const void* inv, const void* wq, const void* wk,
    const void* pos, const void* cos_tab, const void* sin_tab, void* dxq,
    void* dxk, void* dw_partial, void* dwq, void* dwk, int n_tokens,
    int n_pos, int nh, int nkv, int head_dim, hipStream_t stream) {
  const int n_rows = n_tokens * (nh + nkv);
  const int n_slices = qknr_grid(n_rows, head_dim);
  const dim3 grid(n_slices), block(QKNR_THREADS);
#define QKNR_BWD(DD)                                                          \
  hipLaunchKernelGGL((qk_norm_rope_bwd_kernel<DD>), grid, block, 0, stream,   \
                     (const short*)dyq, (const short*)dyk, dyq_stride,        \
                     dyk_stride, (const short*)xq, (const short*)xk,          \
                     q_stride, k_stride, (const float*)inv, (const short*)wq, \
                     (const short*)wk, (const int*)pos,                       \
                     (const float*)cos_tab, (const float*)sin_tab,            \
                     (short*)dxq, (short*)dxk, (float*)dw_partial, n_rows,    \
                     n_pos, nh, nkv)
  if (head_dim == 128)
    QKNR_BWD(128);
  else
    QKNR_BWD(64);
#undef QKNR_BWD
  hipLaunchKernelGGL(qk_norm_dw_kernel, dim3(2 * head_dim / QKNR_DW_COLS),
                     dim3(QKNR_DW_COLS * QKNR_DW_STRIPES), 0, stream,
                     (const float*)dw_partial, (short*)dwq, (short*)dwk,
                     n_slices, head_dim);
}

}  // extern "C"
