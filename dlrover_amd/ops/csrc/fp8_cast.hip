// FP8 operands for the linear layers: tensor-wise absmax scale, and a cast
// that writes the codes row-major and transposed from one read of the input.
//
// Format (the adamw_fp8.hip convention, one scale per tensor): for t[R, C]
// and FMAX = 448 (e4m3fn) or 57344 (e5m2), scale = absmax(t) / FMAX by fp32
// division with a NaN-propagating absmax; a scale below FLT_MIN (the all-zero
// tensor included) is flushed to 0 and every code is 0, nothing is divided;
// otherwise code = RNE(float(t) / scale) and the dequantised value is
// float(code) * scale. An inf or NaN element makes the scale inf or NaN.
//
// fp8_amax: two stages over a caller-owned u32 workspace, no atomics. Stage 1
// is a grid-stride loop of 16-byte loads; a block's maximum of |x| bit
// patterns goes to partials[blockIdx.x]. Stage 2 (one block) reduces them and
// writes the scale.
//
// fp8_cast_transpose: a 256-thread block owns a 128 x 128 tile (R and C are
// multiples of 16, so a partial edge tile ends on a 16-element boundary).
//   cast phase: thread (rg = t / 8, cc = t % 8) converts rows 4 rg .. 4 rg + 3,
//     columns 16 cc .. 16 cc + 15: 16-byte loads, one 16-byte store of codes
//     per row — eight lanes cover 128 contiguous bytes of a codes row — and
//     the same 16 bytes go to the LDS tile.
//   transpose phase: thread (rch = t % 8, cq = t / 8) reads the dwords of
//     rows 16 rch .. 16 rch + 15 at column quad cq (ds_read_b32), transposes
//     the 16 x 4 bytes in registers and stores four 16-byte pieces, one per
//     column, each 16 consecutive rows — eight lanes cover 128 contiguous
//     bytes of a codes_t row.
// LDS tile: 128 rows of 128 bytes, no padding; the 16-byte chunk index of a
// row is XORed with (row / 16) % 8. ds_write_b128 is served in groups of
// eight consecutive lanes (one row, eight different chunks); ds_read_b32 in
// 32-lane halves, banks (a / 4) % 32 = cq ^ (rch << 2) over cq in a group of
// four and rch in 0..7: 32 different banks. Both are conflict-free.
#include "kern_common.h"
#include "fp8_cast_launch.h"

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

#define FC_THREADS 256
#define FC_WAVES (FC_THREADS / WAVE_SIZE)
#define FC_TILE 128
#define FC_MIN_SCALE 1.17549435e-38f  // FLT_MIN, the smallest normal fp32

// Bit pattern of |x|. As unsigned integers these order like the values they
// encode, with every NaN above inf: an integer maximum is an absmax that
// propagates NaN (fmaxf would drop it), like torch.amax.
__device__ __forceinline__ unsigned int fc_abs_bits(float x) {
  return __float_as_uint(x) & 0x7fffffffu;
}

__device__ __forceinline__ unsigned int fc_umax(unsigned int a,
                                                unsigned int b) {
  return a > b ? a : b;
}

// Maximum over the block, valid in every thread; scratch holds FC_WAVES words.
__device__ __forceinline__ unsigned int fc_block_umax(unsigned int v,
                                                      unsigned int* scratch) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    v = fc_umax(v, (unsigned int)__shfl_xor((int)v, off, WAVE_SIZE));
  if ((threadIdx.x & (WAVE_SIZE - 1)) == 0) scratch[threadIdx.x >> 6] = v;
  __syncthreads();
  unsigned int m = 0;
#pragma unroll
  for (int i = 0; i < FC_WAVES; ++i) m = fc_umax(m, scratch[i]);
  return m;
}

// ---------------------------------------------------------------------------
// absmax -> scale
// ---------------------------------------------------------------------------

// n_vec 16-byte vectors: 8 bf16 or 4 fp32 each
template <bool BF16>
__global__ __launch_bounds__(FC_THREADS) void fp8_amax_partial_kernel(
    const u32x4* __restrict__ x, long long n_vec,
    unsigned int* __restrict__ partials) {
  __shared__ unsigned int scratch[FC_WAVES];
  const long long stride = (long long)gridDim.x * FC_THREADS;
  unsigned int m = 0;
  for (long long i = (long long)blockIdx.x * FC_THREADS + threadIdx.x;
       i < n_vec; i += stride) {
    const u32x4 v = x[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (BF16) {
        // two bf16 per dword, each widened to its fp32 bit pattern
        m = fc_umax(m, (v[j] << 16) & 0x7fffffffu);
        m = fc_umax(m, v[j] & 0x7fff0000u);
      } else {
        m = fc_umax(m, v[j] & 0x7fffffffu);
      }
    }
  }
  m = fc_block_umax(m, scratch);
  if (threadIdx.x == 0) partials[blockIdx.x] = m;
}

__global__ __launch_bounds__(FC_THREADS) void fp8_amax_final_kernel(
    const unsigned int* __restrict__ partials, int n, float fmax,
    float* __restrict__ scale) {
  __shared__ unsigned int scratch[FC_WAVES];
  unsigned int m = 0;
  for (int i = threadIdx.x; i < n; i += FC_THREADS) m = fc_umax(m, partials[i]);
  m = fc_block_umax(m, scratch);
  if (threadIdx.x == 0) {
    float s = __uint_as_float(m) / fmax;
    // A scale below the smallest normal fp32 has too few bits to keep
    // x / scale within +-FMAX: the tensor is flushed. A NaN scale is not below
    // anything and goes on to poison the product.
    if (s < FC_MIN_SCALE) s = 0.f;
    scale[0] = s;
  }
}

// ---------------------------------------------------------------------------
// cast + transpose
// ---------------------------------------------------------------------------

template <int FMT>
__device__ __forceinline__ unsigned int fc_encode4(float a, float b, float c,
                                                   float d) {
  int w;
  if (FMT == FP8_FMT_E4M3) {
    w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
  } else {
    w = __builtin_amdgcn_cvt_pk_bf8_f32(a, b, 0, false);
    w = __builtin_amdgcn_cvt_pk_bf8_f32(c, d, w, true);
  }
  return (unsigned int)w;
}

// 16 consecutive elements at p (16-byte aligned) as fp32
template <bool BF16>
__device__ __forceinline__ void fc_load16(const void* p, float out[16]) {
  if (BF16) {
    const short8_t* q = reinterpret_cast<const short8_t*>(p);
    const short8_t a = q[0], b = q[1];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      out[j] = bf2f(a[j]);
      out[8 + j] = bf2f(b[j]);
    }
  } else {
    const float4_t* q = reinterpret_cast<const float4_t*>(p);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float4_t a = q[k];
#pragma unroll
      for (int j = 0; j < 4; ++j) out[4 * k + j] = a[j];
    }
  }
}

// Byte j of four dwords, gathered into one: the register half of the
// transpose (the compiler emits byte permutes).
__device__ __forceinline__ unsigned int fc_gather_byte(unsigned int d0,
                                                       unsigned int d1,
                                                       unsigned int d2,
                                                       unsigned int d3,
                                                       int j) {
  const int sh = 8 * j;
  return ((d0 >> sh) & 0xffu) | (((d1 >> sh) & 0xffu) << 8) |
         (((d2 >> sh) & 0xffu) << 16) | (((d3 >> sh) & 0xffu) << 24);
}

template <bool BF16, int FMT>
__global__ __launch_bounds__(FC_THREADS) void fp8_cast_transpose_kernel(
    const void* __restrict__ x, const float* __restrict__ scale_ptr,
    unsigned char* __restrict__ codes, unsigned char* __restrict__ codes_t,
    long long R, long long C, long long tiles_c, long long n_tiles) {
  // 128 rows x 8 chunks of 16 bytes
  __shared__ u32x4 tile[FC_TILE * (FC_TILE / 16)];
  const unsigned int* tile32 = reinterpret_cast<const unsigned int*>(tile);
  const int elem = BF16 ? 2 : 4;
  const float scale = scale_ptr[0];
  const bool flushed = scale == 0.f;  // NaN is not: it poisons the codes

  const int t = threadIdx.x;
  const int cc = t & 7, rg = t >> 3;   // cast phase
  const int rch = t & 7, cq = t >> 3;  // transpose phase

  for (long long tile_id = blockIdx.x; tile_id < n_tiles;
       tile_id += gridDim.x) {
    const long long r0 = (tile_id / tiles_c) * FC_TILE;
    const long long c0 = (tile_id % tiles_c) * FC_TILE;

    const long long col = c0 + 16 * cc;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int lr = 4 * rg + i;  // row within the tile
      const long long row = r0 + lr;
      // R % 16 == 0 and C % 16 == 0: a thread's 16 columns are all inside or
      // all outside
      if (row < R && col < C) {
        u32x4 w = {0u, 0u, 0u, 0u};
        if (!flushed) {
          float v[16];
          fc_load16<BF16>(
              (const char*)x + (row * C + col) * elem, v);
#pragma unroll
          for (int k = 0; k < 4; ++k)
            w[k] = fc_encode4<FMT>(v[4 * k] / scale, v[4 * k + 1] / scale,
                                   v[4 * k + 2] / scale, v[4 * k + 3] / scale);
        }
        if (codes) *reinterpret_cast<u32x4*>(codes + row * C + col) = w;
        if (codes_t) tile[lr * 8 + (cc ^ ((lr >> 4) & 7))] = w;
      }
    }
    if (codes_t) {  // uniform over the grid
      __syncthreads();
      const long long row = r0 + 16 * rch;
      const long long colq = c0 + 4 * cq;
      if (row < R && colq < C) {
        unsigned int d[16];
#pragma unroll
        for (int i = 0; i < 16; ++i)
          d[i] = tile32[(16 * rch + i) * 32 + (cq ^ (rch << 2))];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          u32x4 w;
#pragma unroll
          for (int k = 0; k < 4; ++k)
            w[k] = fc_gather_byte(d[4 * k], d[4 * k + 1], d[4 * k + 2],
                                  d[4 * k + 3], j);
          *reinterpret_cast<u32x4*>(codes_t + (colq + j) * R + row) = w;
        }
      }
      __syncthreads();  // the next tile overwrites the LDS image
    }
  }
}

// ---------------------------------------------------------------------------
// host side. Nothing here allocates, copies or synchronises.
// ---------------------------------------------------------------------------

static long long fc_n_vec(long long numel, int is_bf16) {
  return numel / (is_bf16 ? 8 : 4);
}

extern "C" long long fp8_amax_num_partials(long long numel, int is_bf16) {
  return grid_capped(fc_n_vec(numel, is_bf16), FC_THREADS);
}

extern "C" void fp8_amax_scale_launch(const void* x, long long numel,
                                      int is_bf16, int fmt,
                                      unsigned int* partials, float* scale,
                                      hipStream_t stream) {
  const long long n_vec = fc_n_vec(numel, is_bf16);
  const int grid = grid_capped(n_vec, FC_THREADS);
  if (is_bf16) {
    hipLaunchKernelGGL((fp8_amax_partial_kernel<true>), dim3(grid),
                       dim3(FC_THREADS), 0, stream, (const u32x4*)x, n_vec,
                       partials);
  } else {
    hipLaunchKernelGGL((fp8_amax_partial_kernel<false>), dim3(grid),
                       dim3(FC_THREADS), 0, stream, (const u32x4*)x, n_vec,
                       partials);
  }
  const float fmax = fmt == FP8_FMT_E5M2 ? 57344.f : 448.f;
  hipLaunchKernelGGL(fp8_amax_final_kernel, dim3(1), dim3(FC_THREADS), 0,
                     stream, partials, grid, fmax, scale);
}

template <bool BF16, int FMT>
static void fc_launch(const void* x, const float* scale, void* codes,
                      void* codes_t, long long R, long long C,
                      hipStream_t stream) {
  const long long tiles_r = (R + FC_TILE - 1) / FC_TILE;
  const long long tiles_c = (C + FC_TILE - 1) / FC_TILE;
  const long long n_tiles = tiles_r * tiles_c;
  const int grid = grid_capped(n_tiles, 1);
  hipLaunchKernelGGL((fp8_cast_transpose_kernel<BF16, FMT>), dim3(grid),
                     dim3(FC_THREADS), 0, stream, x, scale,
                     (unsigned char*)codes, (unsigned char*)codes_t, R, C,
                     tiles_c, n_tiles);
}

extern "C" void fp8_cast_transpose_launch(const void* x, const float* scale,
                                          void* codes, void* codes_t,
                                          long long R, long long C,
                                          int is_bf16, int fmt,
                                          hipStream_t stream) {
  if (R <= 0 || C <= 0 || (!codes && !codes_t)) return;
  if (fmt == FP8_FMT_E5M2) {
    if (is_bf16)
      fc_launch<true, FP8_FMT_E5M2>(x, scale, codes, codes_t, R, C, stream);
    else
      fc_launch<false, FP8_FMT_E5M2>(x, scale, codes, codes_t, R, C, stream);
  } else {
    if (is_bf16)
      fc_launch<true, FP8_FMT_E4M3>(x, scale, codes, codes_t, R, C, stream);
    else
      fc_launch<false, FP8_FMT_E4M3>(x, scale, codes, codes_t, R, C, stream);
  }
}
