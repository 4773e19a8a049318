// Grouped GEMMs of the MoE experts for gfx950: bf16 operands, fp32
// accumulation on v_mfma_f32_32x32x16_bf16, one rounding to bf16 at the
// store. Three forms over R rows in expert order, offs [E] the inclusive
// cumulative row counts of moe_sort, w [E, K, N]:
//   fwd    y[r, :]  = a(r) @ w[e(r)]                 reduction over K
//   dgrad  da[r, :] = dy[r, :] @ w[e(r)]^T           reduction over N, same w
//   wgrad  dw[e]    = sum_{r of e} a(r)^T dy[r, :]   reduction over e's rows
// a(r) is row r of `a`, or with the dispatch fused in, row slot_of_row[r] / k
// of the token tensor: the gather happens while the A tile is loaded, so the
// expert-ordered copy of the tokens is never written.
//
// Work split. No atomics, no workspace, grids from the shapes alone:
//   fwd, dgrad: grid (ceil(R / 128) + E, column tiles). Expert e owns
//     ceil(count_e / 128) row tiles, so a tile never straddles two experts and
//     the sum is at most R / 128 + E. Every block scans offs once (one thread
//     per expert, a wave scan plus the wave sums through LDS), finds the expert
//     and the row range of its tile index and exits when the index lies past
//     the real tile count. Rows past the range load as zeros and are skipped
//     at the store. Row tiles run along grid x, so neighbouring blocks share
//     an expert's column panel of w in L2.
//   wgrad: grid (N tiles, K tiles, E). A block walks all rows of its expert in
//     steps of 32 and keeps the 128x128 sum in registers, rounds once and
//     always stores (zeros for an expert without rows). The rows are not
//     split over blocks, which keeps the bits reproducible and costs balance:
//     the expert with the most rows sets the time.
//
// Tile design. 256 threads, block tile 128x128, wave (wm, wn) owns 64x64 as
// 2x2 MFMA tiles: 64 accumulator VGPRs. The reduction step is 32, not 64:
// K % 32 == 0 and N % 32 == 0 are the supported range, so no step of fwd or
// dgrad has a tail and nothing in the inner loop is masked along the
// reduction; two buffers of 2 x 8 KiB are 32 KiB of LDS, which leaves room for
// several blocks per CU to cover each other's barriers. A step is 8 MFMAs per
// wave behind 4 16-byte global loads per thread; the loads of step s + 1 are
// issued before the MFMAs of step s and stored to the other buffer after
// them, one barrier per step.
//   An operand whose reduction index is contiguous in memory (a and dy in fwd
//   and dgrad, w in dgrad) is a "direct" tile [128][32], 64-byte rows, read as
//   one ds_read_b128 per fragment. 16-byte chunk c of row r sits at chunk
//   c ^ ((r >> 2) & 3): rows r and r + 4 are 256 B apart, so this spreads 16
//   consecutive rows of one chunk column over all 16 chunk positions.
//   An operand whose reduction index is strided (w in fwd, both operands of
//   wgrad) is a "transposed" tile [32][128] in attention_frag.h's layout
//   (256-byte rows, swz), read with the probe-verified gather table of
//   tr_colT_frag, i.e. ds_read_b64_tr_b16. Storing transposed instead would
//   cost 8 2-byte LDS stores per global load.
//   The MFMA operands are swapped (A operand = the column fragment): a lane
//   then holds 4 consecutive output columns of one row per register quad, the
//   epilogue packs them to 8 bytes, stages the tile through the (now idle)
//   32 KiB of LDS and writes rows with 16-byte stores.
//
// Indices read from memory (offs, slot_of_row) are clamped into range before
// they address anything: a corrupt index gives a wrong row, never a fault.
#include "attention_frag.h"
#include "moe_gemm_launch.h"

#define MG_THREADS 256
#define MG_WAVES (MG_THREADS / WAVE_SIZE)
#define MG_BM 128                      // tile edge, both output dimensions
#define MG_BK 32                       // reduction step
#define MG_TILE_BYTES (MG_BM * MG_BK * 2)
#define MG_LDS_BYTES (4 * MG_TILE_BYTES)  // 2 buffers x (A tile, B tile)

static_assert(MG_LDS_BYTES == MG_BM * MG_BM * 2, "the epilogue stages a tile");
static_assert(MOE_GEMM_MAX_EXPERTS <= MG_THREADS, "one thread per expert");

namespace {

__device__ __forceinline__ int clamp_index(int i, int n) {
  return i < 0 ? 0 : (i >= n ? n - 1 : i);
}

// byte offset of 16-byte chunk c (0..3) of row `row` in a direct tile
__device__ __forceinline__ int d_off(int row, int c) {
  return row * 64 + ((c ^ ((row >> 2) & 3)) << 4);
}

// byte offset of 16-byte chunk c (0..15) of row `row` in a transposed tile
__device__ __forceinline__ int t_off(int row, int c) {
  return row * 256 + swz(row, c << 4);
}

// tr_colT_frag's gather (attention_frag.h: same tile layout, same address
// table) with early-clobber outputs. Without them the allocator may give the
// second read's address the upper half of the first read's destination. That
// holds only while the second read issues before the first one's data comes
// back, and with several blocks per CU competing for a SIMD it does not: the
// forward kernel read stray LDS words at the benchmark shapes.
__device__ __forceinline__ bf16x8 tr_frag(const char* tile, int rb, int n,
                                          int lane, int half) {
  const int j = (lane & 15) >> 2;
  const int dq = n * 8 + ((lane & 16) >> 2) + (lane & 3);
  const int r0 = rb + half * 8 + j;
  const int r1 = r0 + 4;
  const unsigned base = (unsigned)(uintptr_t)tile;
  const unsigned a0 = base + r0 * 256 + swz(r0, dq * 8);
  const unsigned a1 = base + r1 * 256 + swz(r1, dq * 8);
  u32x2_t w0, w1;
  asm volatile(
      "ds_read_b64_tr_b16 %0, %2\n\t"
      "ds_read_b64_tr_b16 %1, %3\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(w0), "=&v"(w1)
      : "v"(a0), "v"(a1));
  u32x4_t frag = u32x4_t{w0.x, w0.y, w1.x, w1.y};
  return *reinterpret_cast<bf16x8*>(&frag);
}

// Fragment of outer block ob (32 rows or columns of the output) and k-slice
// ks of a step: element i is operand[outer = ob * 32 + (lane & 31)]
// [red = ks * 16 + half * 8 + i].
template <bool TR>
__device__ __forceinline__ bf16x8 read_frag(const char* tile, int ob, int ks,
                                            int lane, int half) {
  if constexpr (TR) {
    return tr_frag(tile, ks * 16, ob, lane, half);
  } else {
    const int row = ob * 32 + (lane & 31);
    return *reinterpret_cast<const bf16x8*>(tile +
                                            d_off(row, ks * 2 + half));
  }
}

// One reduction step of a wave's 64x64. Operands swapped: acc[i][j] holds the
// transpose, register r of a lane is output row i * 32 + (lane & 31) and
// column j * 32 + (r & 3) + 8 * (r >> 2) + 4 * half of the wave's tile.
template <bool A_TR, bool B_TR>
__device__ __forceinline__ void mma_step(const char* ta, const char* tb,
                                         f32x16_t acc[2][2], int wm, int wn,
                                         int lane, int half) {
#pragma unroll
  for (int ks = 0; ks < MG_BK / 16; ++ks) {
    bf16x8 fa[2], fb[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      fa[i] = read_frag<A_TR>(ta, wm * 2 + i, ks, lane, half);
      fb[i] = read_frag<B_TR>(tb, wn * 2 + i, ks, lane, half);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            fb[j], fa[i], acc[i][j], 0, 0, 0);
  }
}

// Rounds the block's tile to bf16, stages it through LDS and writes the
// first `rows` rows and `cols` columns (a multiple of 8, may exceed 128) to
// out, row pitch ld elements.
__device__ __forceinline__ void store_tile(char* lds,
                                           const f32x16_t acc[2][2],
                                           short* __restrict__ out,
                                           long long ld, int rows, int cols,
                                           int wm, int wn, int lane,
                                           int half) {
  __syncthreads();  // every wave is done with the operand tiles
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int m = wm * 64 + i * 32 + (lane & 31);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int n = wn * 64 + j * 32 + 8 * q + 4 * half;
        const u32x2_t v = {
            pack_bf16(acc[i][j][4 * q], acc[i][j][4 * q + 1]),
            pack_bf16(acc[i][j][4 * q + 2], acc[i][j][4 * q + 3])};
        const int chunk = (n >> 3) ^ (m & 15);
        *reinterpret_cast<u32x2_t*>(lds + m * 256 + chunk * 16 +
                                    (n & 4) * 2) = v;
      }
    }
  }
  __syncthreads();
  const int c = threadIdx.x & 15;
  if (c * 8 >= cols) return;
#pragma unroll
  for (int it = 0; it < MG_BM / 16; ++it) {
    const int m = (threadIdx.x >> 4) + 16 * it;
    if (m < rows)
      *reinterpret_cast<short8_t*>(out + m * ld + c * 8) =
          *reinterpret_cast<const short8_t*>(lds + m * 256 +
                                             ((c ^ (m & 15)) << 4));
  }
}

// The expert, first row and valid rows (1..128) of row tile `tile`; false
// when the index lies past the real tile count. Block-uniform; sh holds
// MG_WAVES + 3 ints.
__device__ __forceinline__ bool find_tile(const int* __restrict__ offs, int E,
                                          int R, int tile, int* sh, int& e,
                                          int& row0, int& rows) {
  const int i = threadIdx.x;
  const int lane = i & (WAVE_SIZE - 1);
  const int wid = i >> 6;
  int lo = 0, hi = 0;
  if (i < E) {
    lo = i ? offs[i - 1] : 0;
    hi = offs[i];
    lo = min(max(lo, 0), R);
    hi = min(max(hi, lo), R);
  }
  const int cnt = hi - lo;
  const int nt = cnt / MG_BM + (cnt % MG_BM != 0);
  int inc = nt;
#pragma unroll
  for (int off = 1; off < WAVE_SIZE; off <<= 1) {
    const int o = __shfl_up(inc, off, WAVE_SIZE);
    if (lane >= off) inc += o;
  }
  if (lane == WAVE_SIZE - 1) sh[wid] = inc;
  if (i == 0) sh[MG_WAVES] = -1;
  __syncthreads();
  for (int w = 0; w < wid; ++w) inc += sh[w];
  const int excl = inc - nt;
  if (i < E && tile >= excl && tile < inc) {  // at most one thread
    sh[MG_WAVES] = i;
    sh[MG_WAVES + 1] = lo + (tile - excl) * MG_BM;
    sh[MG_WAVES + 2] = hi;
  }
  __syncthreads();
  e = sh[MG_WAVES];
  if (e < 0) return false;
  row0 = sh[MG_WAVES + 1];
  rows = min(MG_BM, sh[MG_WAVES + 2] - row0);
  return true;
}

// fwd (DGRAD = false): out [R, N] = a(r) @ w[e], `a` rows of K.
// dgrad (DGRAD = true): out [R, K] = a[r] @ w[e]^T, `a` = dy, rows of N.
template <bool DGRAD>
__global__ __launch_bounds__(MG_THREADS) void moe_gemm_rows_kernel(
    const short* __restrict__ a, const short* __restrict__ w,
    const int* __restrict__ offs, const int* __restrict__ slot_of_row,
    short* __restrict__ out, int R, int T, int topk, int E, int K, int N) {
  __shared__ __attribute__((aligned(16))) char lds[MG_LDS_BYTES];
  __shared__ int sh[MG_WAVES + 3];
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63, half = lane >> 5;
  const int wm = wave >> 1, wn = wave & 1;

  int e, row0, rows;
  if (!find_tile(offs, E, R, blockIdx.x, sh, e, row0, rows)) return;
  const int red = DGRAD ? N : K;   // reduction length
  const int cols = DGRAD ? K : N;  // output columns
  const int c0 = blockIdx.y * MG_BM;
  const short* we = w + (size_t)e * K * N;

  // A, a direct tile: this thread moves chunk ac of rows ar and ar + 64
  const int ac = tid & 3, ar = tid >> 2;
  const short* asrc[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int lr = ar + 64 * h;
    asrc[h] = nullptr;
    if (lr < rows) {
      long long src = (long long)row0 + lr;
      if (slot_of_row != nullptr)
        src = clamp_index(slot_of_row[src] / topk, T);
      asrc[h] = a + src * red + ac * 8;
    }
  }
  // B: fwd, a transposed tile, chunk tc of reduction rows tr and tr + 16;
  // dgrad, a direct tile of w's rows c0 + ar, c0 + ar + 64
  const int tc = tid & 15, tr = tid >> 4;
  const short* bsrc[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    if (DGRAD) {
      const int kr = c0 + ar + 64 * h;
      bsrc[h] = kr < K ? we + (size_t)kr * N + ac * 8 : nullptr;
    } else {
      bsrc[h] = c0 + tc * 8 < N
                    ? we + (size_t)(tr + 16 * h) * N + c0 + tc * 8
                    : nullptr;
    }
  }
  const size_t bstep = DGRAD ? MG_BK : (size_t)MG_BK * N;

  const short8_t zero = {0, 0, 0, 0, 0, 0, 0, 0};
  short8_t pa[2], pb[2];
  auto fetch = [&](int s) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      pa[h] = asrc[h] != nullptr
                  ? *reinterpret_cast<const short8_t*>(asrc[h] + s * MG_BK)
                  : zero;
      pb[h] = bsrc[h] != nullptr
                  ? *reinterpret_cast<const short8_t*>(bsrc[h] + s * bstep)
                  : zero;
    }
  };
  auto stash = [&](char* buf) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      *reinterpret_cast<short8_t*>(buf + d_off(ar + 64 * h, ac)) = pa[h];
      const int boff = DGRAD ? d_off(ar + 64 * h, ac) : t_off(tr + 16 * h, tc);
      *reinterpret_cast<short8_t*>(buf + MG_TILE_BYTES + boff) = pb[h];
    }
  };

  f32x16_t acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int steps = red / MG_BK;
  fetch(0);
  stash(lds);
  __syncthreads();
  for (int s = 0; s < steps; ++s) {
    char* cur = lds + (s & 1) * 2 * MG_TILE_BYTES;
    const bool more = s + 1 < steps;
    if (more) fetch(s + 1);
    mma_step<false, !DGRAD>(cur, cur + MG_TILE_BYTES, acc, wm, wn, lane, half);
    if (more) stash(lds + ((s + 1) & 1) * 2 * MG_TILE_BYTES);
    __syncthreads();
  }
  store_tile(lds, acc, out + (long long)row0 * cols + c0, cols, rows,
             cols - c0, wm, wn, lane, half);
}

// dw[e][k0.., n0..] = sum over the rows of e of a(r)^T dy[r]
__global__ __launch_bounds__(MG_THREADS) void moe_gemm_wgrad_kernel(
    const short* __restrict__ a, const short* __restrict__ dy,
    const int* __restrict__ offs, const int* __restrict__ slot_of_row,
    short* __restrict__ dw, int R, int T, int topk, int K, int N) {
  __shared__ __attribute__((aligned(16))) char lds[MG_LDS_BYTES];
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63, half = lane >> 5;
  const int wm = wave >> 1, wn = wave & 1;
  const int e = blockIdx.z;
  const int k0 = blockIdx.y * MG_BM, n0 = blockIdx.x * MG_BM;

  int lo = e ? offs[e - 1] : 0;
  int hi = offs[e];
  lo = min(max(lo, 0), R);
  hi = min(max(hi, lo), R);
  const int cnt = hi - lo;
  const int steps = cnt / MG_BK + (cnt % MG_BK != 0);

  // both operands are transposed tiles: chunk tc of rows tr and tr + 16 of a
  // step's 32 rows
  const int tc = tid & 15, tr = tid >> 4;
  const bool a_ok = k0 + tc * 8 < K, b_ok = n0 + tc * 8 < N;
  const short* acol = a + k0 + tc * 8;
  const short* bcol = dy + n0 + tc * 8;

  // source rows of a for step s; -1 past the expert's range
  auto source = [&](int s, long long src[2]) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const long long r = (long long)lo + (long long)s * MG_BK + tr + 16 * h;
      src[h] = -1;
      if (s < steps && r < hi)
        src[h] = slot_of_row != nullptr
                     ? clamp_index(slot_of_row[r] / topk, T)
                     : r;
    }
  };
  const short8_t zero = {0, 0, 0, 0, 0, 0, 0, 0};
  short8_t pa[2], pb[2];
  auto fetch = [&](int s, const long long src[2]) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const long long r = (long long)lo + (long long)s * MG_BK + tr + 16 * h;
      const bool on = src[h] >= 0;
      pa[h] = on && a_ok
                  ? *reinterpret_cast<const short8_t*>(acol + src[h] * K)
                  : zero;
      pb[h] = on && b_ok ? *reinterpret_cast<const short8_t*>(bcol + r * N)
                         : zero;
    }
  };
  auto stash = [&](char* buf) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int off = t_off(tr + 16 * h, tc);
      *reinterpret_cast<short8_t*>(buf + off) = pa[h];
      *reinterpret_cast<short8_t*>(buf + MG_TILE_BYTES + off) = pb[h];
    }
  };

  f32x16_t acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // the row indices of a gather run one step ahead of the rows themselves
  long long src[2];
  source(0, src);
  if (steps > 0) {
    fetch(0, src);
    source(1, src);
    stash(lds);
  }
  __syncthreads();
  for (int s = 0; s < steps; ++s) {
    char* cur = lds + (s & 1) * 2 * MG_TILE_BYTES;
    const bool more = s + 1 < steps;
    if (more) {
      fetch(s + 1, src);
      source(s + 2, src);
    }
    mma_step<true, true>(cur, cur + MG_TILE_BYTES, acc, wm, wn, lane, half);
    if (more) stash(lds + ((s + 1) & 1) * 2 * MG_TILE_BYTES);
    __syncthreads();
  }
  store_tile(lds, acc, dw + ((size_t)e * K + k0) * N + n0, N, K - k0, N - n0,
             wm, wn, lane, half);
}

int tiles(long long n) { return (int)((n + MG_BM - 1) / MG_BM); }

}  // namespace

extern "C" {

void moe_gemm_fwd_launch(const void* a, const void* w, const int* offs,
                         const int* slot_of_row, void* y, long long R,
                         long long T, int k, int E, int K, int N,
                         hipStream_t stream) {
  hipLaunchKernelGGL(moe_gemm_rows_kernel<false>, dim3(tiles(R) + E, tiles(N)),
                     dim3(MG_THREADS), 0, stream, (const short*)a,
                     (const short*)w, offs, slot_of_row, (short*)y, (int)R,
                     (int)T, k, E, K, N);
  HIP_CHECK_KERNEL();
}

void moe_gemm_dgrad_launch(const void* dy, const void* w, const int* offs,
                           void* da, long long R, int E, int K, int N,
                           hipStream_t stream) {
  hipLaunchKernelGGL(moe_gemm_rows_kernel<true>, dim3(tiles(R) + E, tiles(K)),
                     dim3(MG_THREADS), 0, stream, (const short*)dy,
                     (const short*)w, offs, (const int*)nullptr, (short*)da,
                     (int)R, (int)R, 1, E, K, N);
  HIP_CHECK_KERNEL();
}

void moe_gemm_wgrad_launch(const void* a, const void* dy, const int* offs,
                           const int* slot_of_row, void* dw, long long R,
                           long long T, int k, int E, int K, int N,
                           hipStream_t stream) {
  hipLaunchKernelGGL(moe_gemm_wgrad_kernel, dim3(tiles(N), tiles(K), E),
                     dim3(MG_THREADS), 0, stream, (const short*)a,
                     (const short*)dy, offs, slot_of_row, (short*)dw, (int)R,
                     (int)T, k, K, N);
  HIP_CHECK_KERNEL();
}

}  // extern "C"
