// Mixture-of-experts routing around the library's grouped GEMMs: top-k router
// (forward and backward), stable token sort by expert, dispatch gather, and
// the weighted combine (forward and backward). bf16 activations, fp32 math,
// wave 64. No floating-point atomics and no host synchronisation: every
// reduction runs in a fixed order, so all outputs are bit-identical from call
// to call, and the per-expert counts never leave the device.
//
// Router: one wave per token, a 256-thread block takes 4 tokens per step of
// a grid-stride loop (grid capped at 2048). Lane l holds the logits of
// experts l, l+64, l+128, l+192 (E <= 256), so a row is read with coalesced
// 2-byte loads and never touches LDS. The softmax is two wave reductions.
// The selection is k rounds of a wave arg-max over (logit, expert) pairs on
// the *logits* (exact on bf16, independent of exp rounding): each lane offers
// its best untaken expert, a 6-step xor butterfly keeps the larger logit and
// on equal logits the lower expert, and the owner lane marks it taken. One
// wave per token was chosen over one lane group per token because E/64 <= 4
// values per lane keeps everything in registers for every supported E, and
// the arg-max butterfly costs the same 6 steps for E = 8 as for E = 256; at
// E < 64 the idle lanes cost nothing that matters, as the kernel is bound by
// its T*E*2 input bytes. probs_mean accumulates in the lanes' registers over
// a wave's tokens, the 4 waves of a block combine through LDS in wave order
// into one [E] slice per block, and a second kernel (one block per expert)
// sums the slices in a fixed tree and divides by T.
//
// Router backward: same mapping, recomputes p, builds dp in the owner lanes
// (scatter of d_topk_w, the renormalisation term, d_probs_mean / T) and
// writes p * (dp - <p, dp>) in one pass.
//
// Sort: a three-stage stable counting sort of the T*k slots. Blocks own
// contiguous chunks of slots (a multiple of 256, at most 128 blocks), so
// block order is slot order. (1) each block counts its chunk per expert with
// integer LDS counters (order-independent) and writes hist[e][block]; (2) one
// 1024-thread block turns hist into exclusive offsets in (expert, block)
// order and writes offs; (3) each block walks its chunk again in 256-slot
// tiles: a lane finds the lanes of its wave with the same expert from 8
// ballots over the bits of the expert id (there is no match-any on gfx950),
// its rank is the popcount of the matching lanes below it, and the 4 waves of
// a tile take their turn in order against running per-expert bases in LDS.
//
// Dispatch, combine: gathers by token, never scatter-adds. One thread moves
// 8 bf16 (16 B) of a row; the combine accumulates a token's k rows in fp32 in
// slot order and rounds once. The combine backward gives a token to a group
// of min(64, H/8 rounded up to a power of two) lanes, which reads dy[t] once,
// writes the k scaled rows and reduces the k dot products with xor shuffles
// inside the group.
//
// Row and slot indices come from the sort and are trusted for correctness;
// every index read from memory is still clamped into range before it
// addresses anything, so a corrupt index gives a wrong row, never a fault.
#include <climits>

#include "kern_common.h"
#include "moe_launch.h"

#define MOE_THREADS 256
#define MOE_WAVES (MOE_THREADS / WAVE_SIZE)
#define MOE_EPL (MOE_MAX_EXPERTS / WAVE_SIZE)  // experts per lane
#define MOE_MAX_BLOCKS 2048
#define MOE_SORT_TILE 256
#define MOE_SORT_MAX_BLOCKS 128
#define MOE_SCAN_THREADS 1024

namespace {

__device__ __forceinline__ int clamp_index(int i, int n) {
  return i < 0 ? 0 : (i >= n ? n - 1 : i);
}

// p[c] of a lane's value with a wave-uniform c
__device__ __forceinline__ float pick(const float p[MOE_EPL], int c) {
  return c == 0 ? p[0] : c == 1 ? p[1] : c == 2 ? p[2] : p[3];
}

// A wave loads one row of logits and its softmax: v[c], p[c] belong to expert
// lane + 64 c; both are -inf / 0 past E.
__device__ __forceinline__ void load_softmax(const short* __restrict__ row,
                                             int E, int lane,
                                             float v[MOE_EPL],
                                             float p[MOE_EPL]) {
  float m = -INFINITY;
#pragma unroll
  for (int c = 0; c < MOE_EPL; ++c) {
    const int e = lane + WAVE_SIZE * c;
    v[c] = e < E ? bf2f(row[e]) : -INFINITY;
    m = fmaxf(m, v[c]);
  }
  m = wave_reduce_max(m);
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < MOE_EPL; ++c) {
    p[c] = lane + WAVE_SIZE * c < E ? expf(v[c] - m) : 0.f;
    s += p[c];
  }
  s = wave_reduce_sum(s);
#pragma unroll
  for (int c = 0; c < MOE_EPL; ++c) p[c] = p[c] / s;
}

__global__ __launch_bounds__(MOE_THREADS) void moe_router_fwd_kernel(
    const short* __restrict__ logits, int* __restrict__ topk_idx,
    float* __restrict__ topk_w, float* __restrict__ partials, long long T,
    int E, int k, int norm_topk) {
  __shared__ float red[MOE_WAVES][MOE_MAX_EXPERTS];
  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  const int wid = threadIdx.x >> 6;
  float acc[MOE_EPL] = {0.f, 0.f, 0.f, 0.f};
  for (long long t = (long long)blockIdx.x * MOE_WAVES + wid; t < T;
       t += (long long)gridDim.x * MOE_WAVES) {
    float v[MOE_EPL], p[MOE_EPL];
    load_softmax(logits + t * E, E, lane, v, p);
#pragma unroll
    for (int c = 0; c < MOE_EPL; ++c) acc[c] += p[c];
    unsigned taken = 0;
    int my_idx = 0;
    float my_w = 0.f, sel_sum = 0.f;
    for (int j = 0; j < k; ++j) {
      // this lane's best untaken expert; a NaN logit sorts as -inf. Experts
      // ascend with c, so a strict > keeps the lower one of equal logits
      float bv = -INFINITY;
      int bi = INT_MAX;
#pragma unroll
      for (int c = 0; c < MOE_EPL; ++c) {
        const int e = lane + WAVE_SIZE * c;
        if (e < E && !((taken >> c) & 1u)) {
          const float key = v[c] == v[c] ? v[c] : -INFINITY;
          if (bi == INT_MAX || key > bv) {
            bv = key;
            bi = e;
          }
        }
      }
      // (logit descending, expert ascending) is a total order: every lane
      // ends the butterfly with the same pair
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(bv, off, WAVE_SIZE);
        const int oi = __shfl_xor(bi, off, WAVE_SIZE);
        if (ov > bv || (ov == bv && oi < bi)) {
          bv = ov;
          bi = oi;
        }
      }
      const int c = (bi >> 6) & (MOE_EPL - 1);
      const int owner = bi & (WAVE_SIZE - 1);
      const float pw = __shfl(pick(p, c), owner, WAVE_SIZE);
      if (lane == owner) taken |= 1u << c;
      if (lane == j) {
        my_idx = bi;
        my_w = pw;
      }
      sel_sum += pw;
    }
    if (lane < k) {
      topk_idx[t * k + lane] = my_idx;
      topk_w[t * k + lane] = norm_topk ? my_w / sel_sum : my_w;
    }
  }
  // block combine in wave order, one [E] slice per block
#pragma unroll
  for (int c = 0; c < MOE_EPL; ++c) red[wid][lane + WAVE_SIZE * c] = acc[c];
  __syncthreads();
  if ((int)threadIdx.x < E) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < MOE_WAVES; ++w) s += red[w][threadIdx.x];
    partials[(long long)blockIdx.x * E + threadIdx.x] = s;
  }
}

// probs_mean[e] = sum over the slices / T. One block per expert: thread i
// sums slices i, i + 256, ..., then a fixed-order block reduction.
__global__ __launch_bounds__(MOE_THREADS) void moe_router_mean_kernel(
    const float* __restrict__ partials, float* __restrict__ probs_mean,
    int n_slices, int E, float inv_T) {
  __shared__ float scratch[MOE_WAVES];
  const int e = blockIdx.x;
  float s = 0.f;
  for (int b = threadIdx.x; b < n_slices; b += MOE_THREADS)
    s += partials[(long long)b * E + e];
  s = block_reduce_sum(s, scratch);
  if (threadIdx.x == 0) probs_mean[e] = s * inv_T;
}

__global__ __launch_bounds__(MOE_THREADS) void moe_router_bwd_kernel(
    const short* __restrict__ logits, const int* __restrict__ topk_idx,
    const float* __restrict__ d_topk_w, const float* __restrict__ d_probs_mean,
    short* __restrict__ dlogits, long long T, int E, int k, int norm_topk,
    float inv_T) {
  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  const int wid = threadIdx.x >> 6;
  float dpm[MOE_EPL];
#pragma unroll
  for (int c = 0; c < MOE_EPL; ++c) {
    const int e = lane + WAVE_SIZE * c;
    dpm[c] = e < E ? d_probs_mean[e] * inv_T : 0.f;
  }
  for (long long t = (long long)blockIdx.x * MOE_WAVES + wid; t < T;
       t += (long long)gridDim.x * MOE_WAVES) {
    float v[MOE_EPL], p[MOE_EPL], dp[MOE_EPL];
    load_softmax(logits + t * E, E, lane, v, p);
#pragma unroll
    for (int c = 0; c < MOE_EPL; ++c) dp[c] = dpm[c];
    // lane j < k holds slot j
    int my_idx = 0;
    float my_g = 0.f;
    if (lane < k) {
      my_idx = clamp_index(topk_idx[t * k + lane], E);
      my_g = d_topk_w[t * k + lane];
    }
    // w_j = p_j / S: dL/dp_j = (g_j - sum_i g_i w_i) / S
    float S = 0.f, gw = 0.f;
    if (norm_topk) {
      for (int j = 0; j < k; ++j) {
        const int idx = __shfl(my_idx, j, WAVE_SIZE);
        const float g = __shfl(my_g, j, WAVE_SIZE);
        const float pj = __shfl(pick(p, idx >> 6), idx & 63, WAVE_SIZE);
        S += pj;
        gw += g * pj;
      }
      gw = gw / S;
    }
    for (int j = 0; j < k; ++j) {
      const int idx = __shfl(my_idx, j, WAVE_SIZE);
      const float g = __shfl(my_g, j, WAVE_SIZE);
      const float d = norm_topk ? (g - gw) / S : g;
      if (lane == (idx & 63)) {
        const int c = idx >> 6;
#pragma unroll
        for (int cc = 0; cc < MOE_EPL; ++cc)
          if (cc == c) dp[cc] += d;
      }
    }
    float dot = 0.f;
#pragma unroll
    for (int c = 0; c < MOE_EPL; ++c) dot += p[c] * dp[c];
    dot = wave_reduce_sum(dot);
#pragma unroll
    for (int c = 0; c < MOE_EPL; ++c) {
      const int e = lane + WAVE_SIZE * c;
      if (e < E) dlogits[t * E + e] = f2bf(p[c] * (dp[c] - dot));
    }
  }
}

// ---- sort -----------------------------------------------------------------

// Blocks and slots per block (a multiple of the tile) for n_slots >= 1.
void sort_geometry(long long n_slots, int* blocks, int* chunk) {
  long long nb = (n_slots + MOE_SORT_TILE - 1) / MOE_SORT_TILE;
  if (nb > MOE_SORT_MAX_BLOCKS) nb = MOE_SORT_MAX_BLOCKS;
  if (nb < 1) nb = 1;
  long long per = (n_slots + nb - 1) / nb;
  per = (per + MOE_SORT_TILE - 1) / MOE_SORT_TILE * MOE_SORT_TILE;
  if (per < MOE_SORT_TILE) per = MOE_SORT_TILE;
  *chunk = (int)per;
  nb = (n_slots + per - 1) / per;
  *blocks = nb < 1 ? 1 : (int)nb;
}

__device__ __forceinline__ int load_expert(const int* __restrict__ topk_idx,
                                           long long s, int E) {
  return clamp_index(topk_idx[s], E);
}

// stage 1: hist[e * gridDim.x + block] = slots of expert e in the block's chunk
__global__ __launch_bounds__(MOE_SORT_TILE) void moe_sort_hist_kernel(
    const int* __restrict__ topk_idx, int* __restrict__ hist,
    long long n_slots, int E, int chunk) {
  __shared__ int cnt[MOE_MAX_EXPERTS];
  cnt[threadIdx.x] = 0;
  __syncthreads();
  const long long lo = (long long)blockIdx.x * chunk;
  const long long hi = lo + chunk < n_slots ? lo + chunk : n_slots;
  for (long long s = lo + threadIdx.x; s < hi; s += MOE_SORT_TILE)
    atomicAdd(&cnt[load_expert(topk_idx, s, E)], 1);
  __syncthreads();
  if ((int)threadIdx.x < E)
    hist[threadIdx.x * gridDim.x + blockIdx.x] = cnt[threadIdx.x];
}

// stage 2: exclusive scan of hist in place, in (expert, block) order, by one
// block; offs[e] = slots of experts 0..e.
__global__ __launch_bounds__(MOE_SCAN_THREADS) void moe_sort_scan_kernel(
    int* __restrict__ hist, int* __restrict__ offs, int n_slots, int E,
    int nb) {
  __shared__ int wave_sum[MOE_SCAN_THREADS / WAVE_SIZE];
  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  const int wid = threadIdx.x >> 6;
  const int M = E * nb;
  const int per = (M + MOE_SCAN_THREADS - 1) / MOE_SCAN_THREADS;
  const int lo = min((int)threadIdx.x * per, M);
  const int hi = min(lo + per, M);
  int s = 0;
  for (int i = lo; i < hi; ++i) s += hist[i];
  int inc = s;
#pragma unroll
  for (int off = 1; off < WAVE_SIZE; off <<= 1) {
    const int o = __shfl_up(inc, off, WAVE_SIZE);
    if (lane >= off) inc += o;
  }
  if (lane == WAVE_SIZE - 1) wave_sum[wid] = inc;
  __syncthreads();
  int run = inc - s;
  for (int w = 0; w < wid; ++w) run += wave_sum[w];
  for (int i = lo; i < hi; ++i) {
    const int c = hist[i];
    hist[i] = run;
    run += c;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < E; e += MOE_SCAN_THREADS)
    offs[e] = e + 1 < E ? hist[(e + 1) * nb] : n_slots;
}

// stage 3: placement. hist holds the exclusive offsets of stage 2.
__global__ __launch_bounds__(MOE_SORT_TILE) void moe_sort_place_kernel(
    const int* __restrict__ topk_idx, const int* __restrict__ hist,
    int* __restrict__ row_of_slot, int* __restrict__ slot_of_row,
    long long n_slots, int E, int chunk) {
  __shared__ int base[MOE_MAX_EXPERTS];
  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  const int wid = threadIdx.x >> 6;
  base[threadIdx.x] =
      (int)threadIdx.x < E ? hist[threadIdx.x * gridDim.x + blockIdx.x] : 0;
  __syncthreads();
  const long long lo = (long long)blockIdx.x * chunk;
  const long long hi = lo + chunk < n_slots ? lo + chunk : n_slots;
  // lo, hi and the tile count are uniform over the block
  for (long long tile = lo; tile < hi; tile += MOE_SORT_TILE) {
    const long long s = tile + threadIdx.x;
    const bool valid = s < hi;
    const int e = valid ? load_expert(topk_idx, s, E) : 0;
    // lanes of this wave with the same expert
    unsigned long long same = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const bool on = (e >> bit) & 1;
      const unsigned long long b = __ballot(on);
      same &= on ? b : ~b;
    }
    const int rank = __popcll(same & ((1ull << lane) - 1ull));
    const int count = __popcll(same);
    // the tile's waves in order; inside a wave the lanes of one expert read
    // its base, then the first of them advances it
    for (int w = 0; w < MOE_SORT_TILE / WAVE_SIZE; ++w) {
      if (w == wid) {
        const int first = valid ? base[e] : 0;
        __builtin_amdgcn_wave_barrier();
        if (valid) {
          const int row = first + rank;
          if (rank == 0) base[e] = first + count;
          if (row >= 0 && row < n_slots) {
            row_of_slot[s] = row;
            slot_of_row[row] = (int)s;
          }
        }
      }
      __syncthreads();
    }
  }
}

// ---- dispatch and combine -------------------------------------------------

__global__ __launch_bounds__(MOE_THREADS) void moe_dispatch_kernel(
    const short* __restrict__ x, const int* __restrict__ slot_of_row,
    short* __restrict__ xp, long long n_rows, int T, int k, int hc) {
  const long long total = n_rows * hc;
  for (long long i = (long long)blockIdx.x * MOE_THREADS + threadIdx.x;
       i < total; i += (long long)gridDim.x * MOE_THREADS) {
    const long long r = i / hc;
    const int c = (int)(i - r * hc);
    const int t = clamp_index(slot_of_row[r] / k, T);
    reinterpret_cast<short8_t*>(xp)[i] =
        reinterpret_cast<const short8_t*>(x)[(long long)t * hc + c];
  }
}

template <bool HAS_W>
__global__ __launch_bounds__(MOE_THREADS) void moe_combine_fwd_kernel(
    const short* __restrict__ yp, const float* __restrict__ w,
    const int* __restrict__ row_of_slot, short* __restrict__ y, long long T,
    int n_rows, int k, int hc) {
  const long long total = T * hc;
  for (long long i = (long long)blockIdx.x * MOE_THREADS + threadIdx.x;
       i < total; i += (long long)gridDim.x * MOE_THREADS) {
    const long long t = i / hc;
    const int c = (int)(i - t * hc);
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    for (int j = 0; j < k; ++j) {
      const int row = clamp_index(row_of_slot[t * k + j], n_rows);
      const float wj = HAS_W ? w[t * k + j] : 1.f;
      float v[8];
      load8(yp + ((long long)row * hc + c) * 8, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += wj * v[e];
    }
    store8(y + i * 8, acc);
  }
}

// lpt lanes per token: a power of two, 1..64
__global__ __launch_bounds__(MOE_THREADS) void moe_combine_bwd_kernel(
    const short* __restrict__ dy, const short* __restrict__ yp,
    const float* __restrict__ w, const int* __restrict__ row_of_slot,
    short* __restrict__ dyp, float* __restrict__ dw, long long T, int n_rows,
    int k, int hc, int lpt) {
  const int tpb = MOE_THREADS / lpt;  // tokens per block and step
  const int g = threadIdx.x / lpt;
  const int l = threadIdx.x - g * lpt;
  const long long n_groups = (T + tpb - 1) / tpb;
  for (long long grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
    const long long t = grp * tpb + g;
    const bool ok = t < T;
    int rows[MOE_MAX_TOPK];
    float ws[MOE_MAX_TOPK], dot[MOE_MAX_TOPK];
#pragma unroll
    for (int j = 0; j < MOE_MAX_TOPK; ++j) {
      const bool on = ok && j < k;
      rows[j] = on ? clamp_index(row_of_slot[t * k + j], n_rows) : 0;
      ws[j] = on ? w[t * k + j] : 0.f;
      dot[j] = 0.f;
    }
    if (ok) {
      for (int c = l; c < hc; c += lpt) {
        float d[8];
        load8(dy + (t * hc + c) * 8, d);
#pragma unroll
        for (int j = 0; j < MOE_MAX_TOPK; ++j) {
          if (j < k) {
            const long long at = ((long long)rows[j] * hc + c) * 8;
            float v[8], o[8];
            load8(yp + at, v);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              dot[j] += d[e] * v[e];
              o[e] = ws[j] * d[e];
            }
            store8(dyp + at, o);
          }
        }
      }
    }
    // every lane of the wave reaches the shuffles; groups are lpt-aligned
#pragma unroll
    for (int j = 0; j < MOE_MAX_TOPK; ++j) {
      if (j < k) {
        float s = dot[j];
        for (int off = lpt >> 1; off > 0; off >>= 1)
          s += __shfl_xor(s, off, WAVE_SIZE);
        if (ok && l == 0) dw[t * k + j] = s;
      }
    }
  }
}

int router_grid(long long T) {
  return grid_capped(T, MOE_WAVES);  // MOE_WAVES tokens per block and step
}

}  // namespace

extern "C" {

int moe_router_num_partials(long long T) { return router_grid(T); }

void moe_router_fwd_launch(const void* logits, int* topk_idx, float* topk_w,
                           float* probs_mean, float* partials, long long T,
                           int E, int k, int norm_topk, hipStream_t stream) {
  const int grid = router_grid(T);
  hipLaunchKernelGGL(moe_router_fwd_kernel, dim3(grid), dim3(MOE_THREADS), 0,
                     stream, (const short*)logits, topk_idx, topk_w, partials,
                     T, E, k, norm_topk);
  HIP_CHECK_KERNEL();
  hipLaunchKernelGGL(moe_router_mean_kernel, dim3(E), dim3(MOE_THREADS), 0,
                     stream, (const float*)partials, probs_mean, grid, E,
                     1.f / (float)T);
  HIP_CHECK_KERNEL();
}

void moe_router_bwd_launch(const void* logits, const int* topk_idx,
                           const float* d_topk_w, const float* d_probs_mean,
                           void* dlogits, long long T, int E, int k,
                           int norm_topk, hipStream_t stream) {
  hipLaunchKernelGGL(moe_router_bwd_kernel, dim3(router_grid(T)),
                     dim3(MOE_THREADS), 0, stream, (const short*)logits,
                     topk_idx, d_topk_w, d_probs_mean, (short*)dlogits, T, E,
                     k, norm_topk, 1.f / (float)T);
  HIP_CHECK_KERNEL();
}

int moe_sort_num_blocks(long long n_slots) {
  int blocks, chunk;
  sort_geometry(n_slots, &blocks, &chunk);
  return blocks;
}

void moe_sort_launch(const int* topk_idx, int* hist, int* offs,
                     int* row_of_slot, int* slot_of_row, long long n_slots,
                     int E, hipStream_t stream) {
  int blocks, chunk;
  sort_geometry(n_slots, &blocks, &chunk);
  hipLaunchKernelGGL(moe_sort_hist_kernel, dim3(blocks), dim3(MOE_SORT_TILE),
                     0, stream, topk_idx, hist, n_slots, E, chunk);
  HIP_CHECK_KERNEL();
  hipLaunchKernelGGL(moe_sort_scan_kernel, dim3(1), dim3(MOE_SCAN_THREADS), 0,
                     stream, hist, offs, (int)n_slots, E, blocks);
  HIP_CHECK_KERNEL();
  hipLaunchKernelGGL(moe_sort_place_kernel, dim3(blocks), dim3(MOE_SORT_TILE),
                     0, stream, topk_idx, (const int*)hist, row_of_slot,
                     slot_of_row, n_slots, E, chunk);
  HIP_CHECK_KERNEL();
}

void moe_dispatch_launch(const void* x, const int* slot_of_row, void* xp,
                         long long T, int k, int H, hipStream_t stream) {
  const int hc = H / 8;
  const long long n_rows = T * k;
  hipLaunchKernelGGL(moe_dispatch_kernel,
                     dim3(grid_capped(n_rows * hc, MOE_THREADS)),
                     dim3(MOE_THREADS), 0, stream, (const short*)x,
                     slot_of_row, (short*)xp, n_rows, (int)T, k, hc);
  HIP_CHECK_KERNEL();
}

void moe_combine_fwd_launch(const void* yp, const float* w,
                            const int* row_of_slot, void* y, long long T,
                            int k, int H, hipStream_t stream) {
  const int hc = H / 8;
  const dim3 grid(grid_capped(T * hc, MOE_THREADS)), block(MOE_THREADS);
  if (w != nullptr)
    hipLaunchKernelGGL(moe_combine_fwd_kernel<true>, grid, block, 0, stream,
                       (const short*)yp, w, row_of_slot, (short*)y, T,
                       (int)(T * k), k, hc);
  else
    hipLaunchKernelGGL(moe_combine_fwd_kernel<false>, grid, block, 0, stream,
                       (const short*)yp, w, row_of_slot, (short*)y, T,
                       (int)(T * k), k, hc);
  HIP_CHECK_KERNEL();
}

void moe_combine_bwd_launch(const void* dy, const void* yp, const float* w,
                            const int* row_of_slot, void* dyp, float* dw,
                            long long T, int k, int H, hipStream_t stream) {
  const int hc = H / 8;
  int lpt = 1;
  while (lpt < hc && lpt < WAVE_SIZE) lpt <<= 1;
  const int tpb = MOE_THREADS / lpt;
  hipLaunchKernelGGL(moe_combine_bwd_kernel, dim3(grid_capped(T, tpb)),
                     dim3(MOE_THREADS), 0, stream, (const short*)dy,
                     (const short*)yp, w, row_of_slot, (short*)dyp, dw, T,
                     (int)(T * k), k, hc, lpt);
  HIP_CHECK_KERNEL();
}

}  // extern "C"
