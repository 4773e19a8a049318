// AdamW with FP8 block-scaled moments, and the block quantiser it is built on.
//
// Format: a block is 256 consecutive elements of a contiguous tensor. Per
// block, scale = absmax / 448 (fp32 division) and every element is stored as
// the OCP e4m3fn code of x / scale, round-to-nearest-even; dequantised value
// = float(code) * scale. A block whose scale would be below FLT_MIN (absmax
// under about 5.3e-36, the all-zero block included) has scale 0 and codes 0
// and nothing is divided; a NaN or inf element makes the scale NaN or inf
// and with it the whole block. The second moment is stored as its square root, so both
// moments cover the same dynamic range of gradient magnitudes under one
// block scale.
//
// Mapping: one wave per block, four elements per lane — one dword of codes
// per moment, one b128 of master, b64 (bf16) or b128 (fp32) of gradient. The
// two block maxima are wave reductions over lane shuffles: no LDS, no
// atomics, no allocation, no sync, so the launches are graph-capturable.
//
// The conversions are the gfx950 OCP FP8 instructions (v_cvt_pk_fp8_f32 /
// v_cvt_f32_fp8); tests/test_adamw_fp8_gpu.py compares them exhaustively and
// bitwise with torch's float8_e4m3fn cast.
#include "kern_common.h"
#include "mt_launch.h"

typedef __attribute__((ext_vector_type(4))) float f32x4;

#define F8_BLOCK 256
#define F8_E4M3_MAX 448.f
#define F8_MIN_SCALE 1.17549435e-38f  // FLT_MIN, the smallest normal fp32
// entries are 88 bytes (two more pointers than MTTensor), so fewer of them
// fit the kernel-argument segment
#define F8_MAX_TENSORS 24
#define F8_MAX_BLOCKS 1024
#define F8_THREADS 512
#define F8_WAVES (F8_THREADS / WAVE_SIZE)
#define F8_FLAG_UNALIGNED 1  // gradient or bf16 weight: scalar accesses

struct F8Tensor {
  float* master;
  const void* grad;
  unsigned int* m_codes;  // e4m3 codes of exp_avg, four per dword
  float* m_scale;         // one per 256-block
  unsigned int* r_codes;  // e4m3 codes of sqrt(exp_avg_sq)
  float* r_scale;
  short* param_bf16;
  long long numel;  // a multiple of F8_BLOCK
  float lr, weight_decay, bc1, bc2;
  int span_bias;  // span index within the tensor = blockIdx.x + span_bias
  int flags;
};

struct F8Batch {
  F8Tensor t[F8_MAX_TENSORS];
  unsigned int block_tensor[F8_MAX_BLOCKS / 4];  // u8 entry index per block
  long long span;                                // elements per span
  int partial_base;  // set by mt_cut_launches; unused here
  int pad_;
};

// kernel-argument limit; leave room for the other (and hidden) arguments
static_assert(sizeof(F8Batch) <= 4096 - 512, "F8Batch must fit kernel args");

// ---------------------------------------------------------------------------
// e4m3fn <-> fp32, four at a time (one dword of codes)
// ---------------------------------------------------------------------------

__device__ __forceinline__ void e4m3x4_decode(unsigned int codes, float out[4]) {
  out[0] = __builtin_amdgcn_cvt_f32_fp8((int)codes, 0);
  out[1] = __builtin_amdgcn_cvt_f32_fp8((int)codes, 1);
  out[2] = __builtin_amdgcn_cvt_f32_fp8((int)codes, 2);
  out[3] = __builtin_amdgcn_cvt_f32_fp8((int)codes, 3);
}

__device__ __forceinline__ unsigned int e4m3x4_encode(const float y[4]) {
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], w, true);
  return (unsigned int)w;
}

// Bit pattern of |x|. As unsigned integers these order like the values they
// encode, with every NaN above inf: an integer maximum is an absmax that
// propagates NaN (fmaxf would drop it), like torch.amax.
__device__ __forceinline__ unsigned int abs_bits(float x) {
  return __float_as_uint(x) & 0x7fffffffu;
}

__device__ __forceinline__ unsigned int umax(unsigned int a, unsigned int b) {
  return a > b ? a : b;
}

// Quantises the wave's block: x holds this lane's four values, the block
// scale is returned (identical in every lane).
__device__ __forceinline__ unsigned int f8_quantize_block(const float x[4],
                                                          float& scale) {
  unsigned int bits = umax(umax(abs_bits(x[0]), abs_bits(x[1])),
                           umax(abs_bits(x[2]), abs_bits(x[3])));
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    bits = umax(bits, (unsigned int)__shfl_xor((int)bits, off, WAVE_SIZE));
  scale = __uint_as_float(bits) / F8_E4M3_MAX;
  // A scale below the smallest normal fp32 has too few bits to keep x / scale
  // within +-448 (and may round to 0): such a block, the all-zero one
  // included, is flushed — scale 0, codes 0, nothing is divided. A NaN scale
  // is not below anything and goes on to poison its block.
  if (scale < F8_MIN_SCALE) {
    scale = 0.f;
    return 0u;
  }
  float y[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) y[j] = x[j] / scale;
  return e4m3x4_encode(y);
}

// ---------------------------------------------------------------------------
// stand-alone quantise / dequantise
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(F8_THREADS) void f8_quantize_kernel(
    const float* __restrict__ x, unsigned int* __restrict__ codes,
    float* __restrict__ scales, long long n_blocks) {
  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  const long long wave = (long long)blockIdx.x * F8_WAVES + (threadIdx.x >> 6);
  const long long stride = (long long)gridDim.x * F8_WAVES;
  for (long long b = wave; b < n_blocks; b += stride) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(x + b * F8_BLOCK + lane * 4);
    const float xv[4] = {v[0], v[1], v[2], v[3]};
    float scale;
    const unsigned int c = f8_quantize_block(xv, scale);
    codes[b * (F8_BLOCK / 4) + lane] = c;
    if (lane == 0) scales[b] = scale;
  }
}

__global__ __launch_bounds__(F8_THREADS) void f8_dequantize_kernel(
    const unsigned int* __restrict__ codes, const float* __restrict__ scales,
    float* __restrict__ out, long long n_blocks) {
  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  const long long wave = (long long)blockIdx.x * F8_WAVES + (threadIdx.x >> 6);
  const long long stride = (long long)gridDim.x * F8_WAVES;
  for (long long b = wave; b < n_blocks; b += stride) {
    float d[4];
    e4m3x4_decode(codes[b * (F8_BLOCK / 4) + lane], d);
    const float s = scales[b];
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = d[j] * s;
    *reinterpret_cast<f32x4*>(out + b * F8_BLOCK + lane * 4) = v;
  }
}

// ---------------------------------------------------------------------------
// AdamW over a batch. Same math as mt_adamw_kernel (multi_tensor.hip); the
// update uses the fresh fp32 moments, quantisation error enters only through
// the state the next step loads.
// ---------------------------------------------------------------------------

template <bool GRAD_BF16>
__global__ __launch_bounds__(F8_THREADS) void f8_adamw_kernel(
    const F8Batch b, float beta1, float beta2, float eps, float grad_scale,
    const float* __restrict__ norm_sq, float max_norm, int skip_nonfinite) {
  float coef = 1.f;
  if (norm_sq) {
    const float nsq = norm_sq[0];
    // inf or NaN norm: leave master, moments and bf16 weights untouched
    if (skip_nonfinite && !(fabsf(nsq) <= 3.402823466e+38f)) return;
    const float c = max_norm / (sqrtf(nsq) + 1e-6f);
    coef = (c > 1.f) ? 1.f : c;  // a NaN propagates, like torch.clamp
  }
  const float gs = grad_scale * coef;

  const F8Tensor& e = b.t[mt_block_entry(b.block_tensor)];
  const long long start = ((long long)blockIdx.x + e.span_bias) * b.span;
  long long n = e.numel - start;
  if (n > b.span) n = b.span;
  // span and numel are multiples of F8_BLOCK, so is n
  const long long first_block = start / F8_BLOCK;
  const int n_blocks = (int)(n / F8_BLOCK);
  const float lr = e.lr, weight_decay = e.weight_decay;
  const float bc1 = e.bc1, bc2 = e.bc2;
  const bool scalar_io = (e.flags & F8_FLAG_UNALIGNED) != 0;
  const int lane = threadIdx.x & (WAVE_SIZE - 1);

  for (int k = threadIdx.x >> 6; k < n_blocks; k += F8_WAVES) {
    const long long blk = first_block + k;
    const long long at = blk * F8_BLOCK + lane * 4;  // this lane's 4 elements
    const long long cw = blk * (F8_BLOCK / 4) + lane;
    float g[4];
    if (GRAD_BF16) {
      const short* gp = (const short*)e.grad + at;
      if (scalar_io) {
#pragma unroll
        for (int j = 0; j < 4; ++j) g[j] = bf2f(gp[j]) * gs;
      } else {
        const short4_t gv = *reinterpret_cast<const short4_t*>(gp);
#pragma unroll
        for (int j = 0; j < 4; ++j) g[j] = bf2f(gv[j]) * gs;
      }
    } else {
      const float* gp = (const float*)e.grad + at;
      if (scalar_io) {
#pragma unroll
        for (int j = 0; j < 4; ++j) g[j] = gp[j] * gs;
      } else {
        const f32x4 gv = *reinterpret_cast<const f32x4*>(gp);
#pragma unroll
        for (int j = 0; j < 4; ++j) g[j] = gv[j] * gs;
      }
    }
    f32x4 p = *reinterpret_cast<const f32x4*>(e.master + at);
    float m[4], r[4];
    e4m3x4_decode(e.m_codes[cw], m);
    e4m3x4_decode(e.r_codes[cw], r);
    const float ms = e.m_scale[blk], rs = e.r_scale[blk];
    short4_t pb;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float root = r[j] * rs;
      m[j] = beta1 * (m[j] * ms) + (1.f - beta1) * g[j];
      const float v = beta2 * (root * root) + (1.f - beta2) * g[j] * g[j];
      const float mhat = m[j] * bc1;
      const float vhat = v * bc2;
      p[j] -= lr * (mhat / (sqrtf(vhat) + eps) + weight_decay * p[j]);
      pb[j] = f2bf(p[j]);
      r[j] = sqrtf(v);
    }
    float ms_new, rs_new;
    const unsigned int mc = f8_quantize_block(m, ms_new);
    const unsigned int rc = f8_quantize_block(r, rs_new);
    e.m_codes[cw] = mc;
    e.r_codes[cw] = rc;
    *reinterpret_cast<f32x4*>(e.master + at) = p;
    if (e.param_bf16) {
      short* pp = e.param_bf16 + at;
      if (scalar_io) {
#pragma unroll
        for (int j = 0; j < 4; ++j) pp[j] = pb[j];
      } else {
        *reinterpret_cast<short4_t*>(pp) = pb;
      }
    }
    if (lane == 0) {
      e.m_scale[blk] = ms_new;
      e.r_scale[blk] = rs_new;
    }
  }
}

// ---------------------------------------------------------------------------
// host side. Nothing here allocates, copies or synchronises.
// ---------------------------------------------------------------------------

extern "C" int f8_max_tensors() { return F8_MAX_TENSORS; }
extern "C" int f8_block_elems() { return F8_BLOCK; }

// The multi-tensor rule (about 2048 blocks in total, capped at 65536
// elements; see mt_auto_span) in whole 256-blocks, at least one per wave.
extern "C" long long f8_auto_span(long long total_numel) {
  long long span = (total_numel + 2047) / 2048;
  span = (span + F8_BLOCK - 1) / F8_BLOCK * F8_BLOCK;
  const long long floor_span = (long long)F8_WAVES * F8_BLOCK;
  if (span < floor_span) span = floor_span;
  return span > 65536 ? 65536 : span;
}

extern "C" void f8_quantize_launch(const float* x, void* codes, float* scales,
                                   long long n_blocks, hipStream_t stream) {
  if (n_blocks <= 0) return;
  const int grid = grid_capped(n_blocks, F8_WAVES);
  hipLaunchKernelGGL(f8_quantize_kernel, dim3(grid), dim3(F8_THREADS), 0,
                     stream, x, (unsigned int*)codes, scales, n_blocks);
}

extern "C" void f8_dequantize_launch(const void* codes, const float* scales,
                                     float* out, long long n_blocks,
                                     hipStream_t stream) {
  if (n_blocks <= 0) return;
  const int grid = grid_capped(n_blocks, F8_WAVES);
  hipLaunchKernelGGL(f8_dequantize_kernel, dim3(grid), dim3(F8_THREADS), 0,
                     stream, (const unsigned int*)codes, scales, out, n_blocks);
}

extern "C" void f8_adamw_launch(
    int n, void* const* master, const void* const* grad, void* const* m_codes,
    void* const* m_scale, void* const* r_codes, void* const* r_scale,
    void* const* param_bf16, const long long* numel, const float* lr,
    const float* weight_decay, const int* step, int grad_is_bf16, float beta1,
    float beta2, float eps, float grad_scale, const float* norm_sq,
    float max_norm, int skip_nonfinite, long long span, hipStream_t stream) {
  const uintptr_t grad_mask = grad_is_bf16 ? 7u : 15u;  // b64 or b128 loads
  mt_cut_launches<F8Batch, F8_MAX_TENSORS, F8_MAX_BLOCKS>(
      n, numel, span,
      [&](int i, F8Tensor& e) {
        e.master = (float*)master[i];
        e.grad = grad[i];
        e.m_codes = (unsigned int*)m_codes[i];
        e.m_scale = (float*)m_scale[i];
        e.r_codes = (unsigned int*)r_codes[i];
        e.r_scale = (float*)r_scale[i];
        e.param_bf16 = (short*)param_bf16[i];
        e.numel = numel[i];
        e.lr = lr[i];
        e.weight_decay = weight_decay[i];
        // same expressions as adamw_launch, so all paths agree
        e.bc1 = 1.f / (1.f - powf(beta1, (float)step[i]));
        e.bc2 = 1.f / (1.f - powf(beta2, (float)step[i]));
        const bool unaligned = ((uintptr_t)grad[i] & grad_mask) != 0 ||
                               ((uintptr_t)param_bf16[i] & 7u) != 0;
        e.flags = unaligned ? F8_FLAG_UNALIGNED : 0;
      },
      [&](const F8Batch& batch, int n_blocks) {
        if (grad_is_bf16) {
          hipLaunchKernelGGL((f8_adamw_kernel<true>), dim3(n_blocks),
                             dim3(F8_THREADS), 0, stream, batch, beta1, beta2,
                             eps, grad_scale, norm_sq, max_norm,
                             skip_nonfinite);
        } else {
          hipLaunchKernelGGL((f8_adamw_kernel<false>), dim3(n_blocks),
                             dim3(F8_THREADS), 0, stream, batch, beta1, beta2,
                             eps, grad_scale, norm_sq, max_norm,
                             skip_nonfinite);
        }
      });
}
