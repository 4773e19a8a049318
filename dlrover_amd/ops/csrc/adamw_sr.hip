// Master-free AdamW: bf16 weights updated with stochastic rounding (SR).
//
// Rounding: for a finite fp32 w with bit pattern u and a uniform 16-bit
// integer r, the bf16 result is (u + r) >> 16 (one 32-bit unsigned add, which
// cannot wrap for finite w), so P(round away from zero) = (u & 0xffff) / 65536
// and a value that is exactly a bf16 never moves. inf and NaN get no noise:
// inf keeps its bits, a NaN keeps its sign and upper payload with the quiet
// bit set.
//
// Noise: counter-based, a function of (seed, stream, step, element index)
// and of nothing else. r of element i is 16-bit half i % 8 of the 128-bit
// Philox4x32-10 output for counter (lo32(i / 8), hi32(i / 8), step, stream)
// and key (lo32(seed), hi32(seed)): word (i % 8) / 2, low half when i is even.
// stream is the parameter's ordinal in the optimizer, step its step count and
// i the element's index in the tensor, so the grid, the span and the cut of
// a tensor list into launches never show in the result.
//
// Mapping. sr_round_kernel and sr_adamw_kernel give every lane one group of 8
// consecutive elements, which is one Philox call with all 128 bits used: the
// bf16 weight (and a bf16 gradient) travel as one b128, fp32 arrays as two.
// The last group of a span may be short and a tensor may be misaligned; both
// take scalar accesses through the same arithmetic. sr_f8_adamw_kernel keeps
// f8_adamw_kernel's one wave per 256-block with 4 elements per lane (the
// block maxima need the whole block in one wave), so a lane uses half of its
// Philox output. No LDS, no atomics, no allocation, no sync.
#include <hip/hip_runtime.h>

// Packed fp32 arithmetic is kept out of this file's device code: the update
// is to be bit-identical wherever it runs. A function with other target
// features than its caller is called, not inlined, unless it is
// __forceinline__: the device code below uses builtins and the project's own
// helpers, not the runtime header's plain inline functions (__umulhi,
// __shfl_xor, __float_as_uint, ...).
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#include "adamw_common.h"
#include "mt_launch.h"

#define SR_MAX_TENSORS 32
#define SR_MAX_BLOCKS 1024
#define SR_THREADS 512
#define SR_FLAG_UNALIGNED 1  // some array is not 16-byte aligned: scalar accesses

struct SRTensor {
  short* param;  // bf16 weight, read and written
  const void* grad;
  float* exp_avg;
  float* exp_avg_sq;
  long long numel;
  float lr, weight_decay, bc1, bc2;
  unsigned int stream, step;  // Philox counter words 3 and 2
  int span_bias;  // span index within the tensor = blockIdx.x + span_bias
  int flags;
};

struct SRBatch {
  SRTensor t[SR_MAX_TENSORS];
  unsigned int block_tensor[SR_MAX_BLOCKS / 4];  // u8 entry index per block
  long long span;                                // elements per span, % 8 == 0
  int partial_base;  // set by mt_cut_launches; unused here
  int pad_;
};

struct SRF8Tensor {
  short* param;
  const void* grad;
  unsigned int* m_codes;  // e4m3 codes of exp_avg, four per dword
  float* m_scale;         // one per 256-block
  unsigned int* r_codes;  // e4m3 codes of sqrt(exp_avg_sq)
  float* r_scale;
  long long numel;  // a multiple of F8_BLOCK
  float lr, weight_decay, bc1, bc2;
  unsigned int stream, step;
  int span_bias;
  int flags;
};

struct SRF8Batch {
  SRF8Tensor t[F8_MAX_TENSORS];
  unsigned int block_tensor[F8_MAX_BLOCKS / 4];
  long long span;  // a multiple of F8_BLOCK
  int partial_base;
  int pad_;
};

// kernel-argument limit; leave room for the other (and hidden) arguments
static_assert(sizeof(SRBatch) <= 4096 - 512, "SRBatch must fit kernel args");
static_assert(sizeof(SRF8Batch) <= 4096 - 512, "SRF8Batch must fit kernel args");

// ---------------------------------------------------------------------------
// Philox4x32-10 and the rounding
// ---------------------------------------------------------------------------

struct SRNoise {
  unsigned int k0, k1;  // lo32(seed), hi32(seed)
};

__device__ __forceinline__ void philox4x32_10(unsigned int c0, unsigned int c1,
                                              unsigned int c2, unsigned int c3,
                                              unsigned int k0, unsigned int k1,
                                              unsigned int out[4]) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const unsigned long long p0 = 0xD2511F53ull * c0;  // one 32x32 -> 64 each
    const unsigned long long p1 = 0xCD9E8D57ull * c2;
    c0 = (unsigned int)(p1 >> 32) ^ c1 ^ k0;
    c1 = (unsigned int)p1;
    c2 = (unsigned int)(p0 >> 32) ^ c3 ^ k1;
    c3 = (unsigned int)p0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0;
  out[1] = c1;
  out[2] = c2;
  out[3] = c3;
}

// the 128 bits that serve elements 8 * group .. 8 * group + 7 of one tensor
__device__ __forceinline__ void sr_group_bits(long long group, unsigned int step,
                                              unsigned int stream, SRNoise key,
                                              unsigned int out[4]) {
  philox4x32_10((unsigned int)group, (unsigned int)((unsigned long long)group >> 32),
                step, stream, key.k0, key.k1, out);
}

// half h (0..7) of the group's bits
__device__ __forceinline__ unsigned int sr_half(const unsigned int bits[4], int h) {
  return (bits[h >> 1] >> ((h & 1) * 16)) & 0xffffu;
}

__device__ __forceinline__ short sr_bf16(float w, unsigned int r16) {
  const unsigned int u = __builtin_bit_cast(unsigned int, w);
  if ((u & 0x7f800000u) == 0x7f800000u)  // inf, or NaN: quiet it
    return (short)((u >> 16) | ((u & 0x007fffffu) ? 0x40u : 0u));
  return (short)((u + r16) >> 16);
}

// ---------------------------------------------------------------------------
// stand-alone rounding: out[i] = SR(x[i]), i relative to the tensor
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(256) void sr_round_kernel(
    const float* __restrict__ x, short* __restrict__ out, long long n,
    SRNoise key, unsigned int stream, unsigned int step, int x_vec, int out_vec) {
  const long long groups = (n + 7) >> 3;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long grp = (long long)blockIdx.x * blockDim.x + threadIdx.x;
       grp < groups; grp += stride) {
    const long long at = grp * 8;
    const int cnt = (n - at) < 8 ? (int)(n - at) : 8;
    float w[8];
    if (x_vec && cnt == 8) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(x + at);
      const f32x4 b = *reinterpret_cast<const f32x4*>(x + at + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        w[j] = a[j];
        w[4 + j] = b[j];
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        w[j] = 0.f;
        if (j < cnt) w[j] = x[at + j];
      }
    }
    unsigned int bits[4];
    sr_group_bits(grp, step, stream, key, bits);
    short8_t o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = sr_bf16(w[j], sr_half(bits, j));
    if (out_vec && cnt == 8) {
      *reinterpret_cast<short8_t*>(out + at) = o;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (j < cnt) out[at + j] = o[j];
    }
  }
}

// ---------------------------------------------------------------------------
// AdamW on bf16 weights with fp32 moments. Same math as mt_adamw_kernel
// (multi_tensor.hip) with w = float(p) in the master's place; p = SR(w_new).
// ---------------------------------------------------------------------------

template <bool GRAD_BF16>
__global__ __launch_bounds__(SR_THREADS) void sr_adamw_kernel(
    const SRBatch b, float beta1, float beta2, float eps, float grad_scale,
    const float* __restrict__ norm_sq, float max_norm, int skip_nonfinite,
    SRNoise key) {
  // inf or NaN norm: leave moments and weights untouched
  float gs;
  if (!adamw_grad_scale(norm_sq, max_norm, skip_nonfinite, grad_scale, gs))
    return;

  const SRTensor& e = b.t[mt_block_entry(b.block_tensor)];
  // a multiple of 8, so the span's groups are the tensor's Philox groups
  const long long start = ((long long)blockIdx.x + e.span_bias) * b.span;
  long long n = e.numel - start;
  if (n > b.span) n = b.span;
  short* __restrict__ param = e.param + start;
  float* __restrict__ exp_avg = e.exp_avg + start;
  float* __restrict__ exp_avg_sq = e.exp_avg_sq + start;
  const short* grad_bf16 = (const short*)e.grad + start;
  const float* grad_f32 = (const float*)e.grad + start;
  const float lr = e.lr, weight_decay = e.weight_decay;
  const float bc1 = e.bc1, bc2 = e.bc2;
  const unsigned int stream = e.stream, step = e.step;
  const bool vec_ok = (e.flags & SR_FLAG_UNALIGNED) == 0;
  const long long first_group = start >> 3;
  const long long groups = (n + 7) >> 3;

  for (long long i = threadIdx.x; i < groups; i += SR_THREADS) {
    const long long at = i * 8;
    const int cnt = (n - at) < 8 ? (int)(n - at) : 8;
    const bool vec = vec_ok && cnt == 8;
    float w[8], g[8], m[8], v[8];
    if (vec) {
      const short8_t pv = *reinterpret_cast<const short8_t*>(param + at);
#pragma unroll
      for (int j = 0; j < 8; ++j) w[j] = bf2f(pv[j]);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const f32x4 mv = *reinterpret_cast<const f32x4*>(exp_avg + at + h * 4);
        const f32x4 vv = *reinterpret_cast<const f32x4*>(exp_avg_sq + at + h * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          m[h * 4 + j] = mv[j];
          v[h * 4 + j] = vv[j];
        }
      }
      if (GRAD_BF16) {
        const short8_t gv = *reinterpret_cast<const short8_t*>(grad_bf16 + at);
#pragma unroll
        for (int j = 0; j < 8; ++j) g[j] = bf2f(gv[j]);
      } else {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const f32x4 gv = *reinterpret_cast<const f32x4*>(grad_f32 + at + h * 4);
#pragma unroll
          for (int j = 0; j < 4; ++j) g[h * 4 + j] = gv[j];
        }
      }
    } else {
      // a short last group, or a tensor that is not 16-byte aligned
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        w[j] = g[j] = m[j] = v[j] = 0.f;
        if (j < cnt) {
          w[j] = bf2f(param[at + j]);
          g[j] = GRAD_BF16 ? bf2f(grad_bf16[at + j]) : grad_f32[at + j];
          m[j] = exp_avg[at + j];
          v[j] = exp_avg_sq[at + j];
        }
      }
    }
    unsigned int bits[4];
    sr_group_bits(first_group + i, step, stream, key, bits);
    short8_t pb;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float gj = g[j] * gs;
      m[j] = beta1 * m[j] + (1.f - beta1) * gj;
      v[j] = beta2 * v[j] + (1.f - beta2) * gj * gj;
      const float mhat = m[j] * bc1;
      const float vhat = v[j] * bc2;
      w[j] -= lr * (mhat / (sqrtf(vhat) + eps) + weight_decay * w[j]);
      pb[j] = sr_bf16(w[j], sr_half(bits, j));
    }
    if (vec) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        f32x4 mv, vv;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          mv[j] = m[h * 4 + j];
          vv[j] = v[h * 4 + j];
        }
        *reinterpret_cast<f32x4*>(exp_avg + at + h * 4) = mv;
        *reinterpret_cast<f32x4*>(exp_avg_sq + at + h * 4) = vv;
      }
      *reinterpret_cast<short8_t*>(param + at) = pb;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (j < cnt) {
          exp_avg[at + j] = m[j];
          exp_avg_sq[at + j] = v[j];
          param[at + j] = pb[j];
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// AdamW on bf16 weights with FP8 block-scaled moments: f8_adamw_kernel
// (adamw_fp8.hip) with w = float(p) in the master's place; p = SR(w_new).
// ---------------------------------------------------------------------------

template <bool GRAD_BF16>
__global__ __launch_bounds__(F8_THREADS) void sr_f8_adamw_kernel(
    const SRF8Batch b, float beta1, float beta2, float eps, float grad_scale,
    const float* __restrict__ norm_sq, float max_norm, int skip_nonfinite,
    SRNoise key) {
  float gs;
  if (!adamw_grad_scale(norm_sq, max_norm, skip_nonfinite, grad_scale, gs))
    return;

  const SRF8Tensor& e = b.t[mt_block_entry(b.block_tensor)];
  const long long start = ((long long)blockIdx.x + e.span_bias) * b.span;
  long long n = e.numel - start;
  if (n > b.span) n = b.span;
  // span and numel are multiples of F8_BLOCK, so is n
  const long long first_block = start / F8_BLOCK;
  const int n_blocks = (int)(n / F8_BLOCK);
  const float lr = e.lr, weight_decay = e.weight_decay;
  const float bc1 = e.bc1, bc2 = e.bc2;
  const unsigned int stream = e.stream, step = e.step;
  const bool scalar_io = (e.flags & F8_FLAG_UNALIGNED) != 0;
  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  // this lane's 4 elements are the low (even lane) or high half of a group
  const int half0 = (lane & 1) * 4;

  for (int k = threadIdx.x >> 6; k < n_blocks; k += F8_WAVES) {
    const long long blk = first_block + k;
    const long long at = blk * F8_BLOCK + lane * 4;  // index in the tensor
    const long long cw = blk * (F8_BLOCK / 4) + lane;
    float g[4], w[4];
    short* pp = e.param + at;
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
    if (scalar_io) {
#pragma unroll
      for (int j = 0; j < 4; ++j) w[j] = bf2f(pp[j]);
    } else {
      const short4_t pv = *reinterpret_cast<const short4_t*>(pp);
#pragma unroll
      for (int j = 0; j < 4; ++j) w[j] = bf2f(pv[j]);
    }
    float m[4], r[4];
    e4m3x4_decode(e.m_codes[cw], m);
    e4m3x4_decode(e.r_codes[cw], r);
    const float ms = e.m_scale[blk], rs = e.r_scale[blk];
    unsigned int bits[4];
    sr_group_bits(at >> 3, step, stream, key, bits);
    short4_t pb;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float root = r[j] * rs;
      m[j] = beta1 * (m[j] * ms) + (1.f - beta1) * g[j];
      const float v = beta2 * (root * root) + (1.f - beta2) * g[j] * g[j];
      const float mhat = m[j] * bc1;
      const float vhat = v * bc2;
      w[j] -= lr * (mhat / (sqrtf(vhat) + eps) + weight_decay * w[j]);
      pb[j] = sr_bf16(w[j], sr_half(bits, half0 + j));
      r[j] = sqrtf(v);
    }
    float ms_new, rs_new;
    const unsigned int mc = f8_quantize_block(m, ms_new);
    const unsigned int rc = f8_quantize_block(r, rs_new);
    e.m_codes[cw] = mc;
    e.r_codes[cw] = rc;
    if (scalar_io) {
#pragma unroll
      for (int j = 0; j < 4; ++j) pp[j] = pb[j];
    } else {
      *reinterpret_cast<short4_t*>(pp) = pb;
    }
    if (lane == 0) {
      e.m_scale[blk] = ms_new;
      e.r_scale[blk] = rs_new;
    }
  }
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

// ---------------------------------------------------------------------------
// host side. Nothing here allocates, copies or synchronises.
// ---------------------------------------------------------------------------

static SRNoise sr_key(unsigned long long seed) {
  return SRNoise{(unsigned int)seed, (unsigned int)(seed >> 32)};
}

extern "C" int sr_max_tensors() { return SR_MAX_TENSORS; }

extern "C" void sr_round_launch(const float* x, void* out, long long n,
                                unsigned long long seed, unsigned int stream_id,
                                unsigned int step, hipStream_t stream) {
  if (n <= 0) return;
  const int grid = grid_capped((n + 7) / 8, 256);
  hipLaunchKernelGGL(sr_round_kernel, dim3(grid), dim3(256), 0, stream, x,
                     (short*)out, n, sr_key(seed), stream_id, step,
                     misaligned16(x) ? 0 : 1, misaligned16(out) ? 0 : 1);
}

extern "C" void sr_adamw_launch(
    int n, void* const* param, const void* const* grad, void* const* exp_avg,
    void* const* exp_avg_sq, const long long* numel, const float* lr,
    const float* weight_decay, const int* step, const int* streams,
    int grad_is_bf16, float beta1, float beta2, float eps, float grad_scale,
    const float* norm_sq, float max_norm, int skip_nonfinite,
    unsigned long long seed, long long span, hipStream_t stream) {
  const SRNoise key = sr_key(seed);
  mt_cut_launches<SRBatch, SR_MAX_TENSORS, SR_MAX_BLOCKS>(
      n, numel, span,
      [&](int i, SRTensor& e) {
        e.param = (short*)param[i];
        e.grad = grad[i];
        e.exp_avg = (float*)exp_avg[i];
        e.exp_avg_sq = (float*)exp_avg_sq[i];
        e.numel = numel[i];
        e.lr = lr[i];
        e.weight_decay = weight_decay[i];
        // same expressions as adamw_launch, so all paths agree
        e.bc1 = 1.f / (1.f - powf(beta1, (float)step[i]));
        e.bc2 = 1.f / (1.f - powf(beta2, (float)step[i]));
        e.stream = (unsigned int)streams[i];
        e.step = (unsigned int)step[i];
        const bool unaligned = misaligned16(param[i]) || misaligned16(grad[i]) ||
                               misaligned16(exp_avg[i]) ||
                               misaligned16(exp_avg_sq[i]);
        e.flags = unaligned ? SR_FLAG_UNALIGNED : 0;
      },
      [&](const SRBatch& batch, int n_blocks) {
        if (grad_is_bf16) {
          hipLaunchKernelGGL((sr_adamw_kernel<true>), dim3(n_blocks),
                             dim3(SR_THREADS), 0, stream, batch, beta1, beta2,
                             eps, grad_scale, norm_sq, max_norm, skip_nonfinite,
                             key);
        } else {
          hipLaunchKernelGGL((sr_adamw_kernel<false>), dim3(n_blocks),
                             dim3(SR_THREADS), 0, stream, batch, beta1, beta2,
                             eps, grad_scale, norm_sq, max_norm, skip_nonfinite,
                             key);
        }
      });
}

extern "C" void sr_f8_adamw_launch(
    int n, void* const* param, const void* const* grad, void* const* m_codes,
    void* const* m_scale, void* const* r_codes, void* const* r_scale,
    const long long* numel, const float* lr, const float* weight_decay,
    const int* step, const int* streams, int grad_is_bf16, float beta1,
    float beta2, float eps, float grad_scale, const float* norm_sq,
    float max_norm, int skip_nonfinite, unsigned long long seed,
    long long span, hipStream_t stream) {
  const SRNoise key = sr_key(seed);
  const uintptr_t grad_mask = grad_is_bf16 ? 7u : 15u;  // b64 or b128 loads
  mt_cut_launches<SRF8Batch, F8_MAX_TENSORS, F8_MAX_BLOCKS>(
      n, numel, span,
      [&](int i, SRF8Tensor& e) {
        e.param = (short*)param[i];
        e.grad = grad[i];
        e.m_codes = (unsigned int*)m_codes[i];
        e.m_scale = (float*)m_scale[i];
        e.r_codes = (unsigned int*)r_codes[i];
        e.r_scale = (float*)r_scale[i];
        e.numel = numel[i];
        e.lr = lr[i];
        e.weight_decay = weight_decay[i];
        e.bc1 = 1.f / (1.f - powf(beta1, (float)step[i]));
        e.bc2 = 1.f / (1.f - powf(beta2, (float)step[i]));
        e.stream = (unsigned int)streams[i];
        e.step = (unsigned int)step[i];
        const bool unaligned = ((uintptr_t)grad[i] & grad_mask) != 0 ||
                               ((uintptr_t)param[i] & 7u) != 0;
        e.flags = unaligned ? F8_FLAG_UNALIGNED : 0;
      },
      [&](const SRF8Batch& batch, int n_blocks) {
        if (grad_is_bf16) {
          hipLaunchKernelGGL((sr_f8_adamw_kernel<true>), dim3(n_blocks),
                             dim3(F8_THREADS), 0, stream, batch, beta1, beta2,
                             eps, grad_scale, norm_sq, max_norm, skip_nonfinite,
                             key);
        } else {
          hipLaunchKernelGGL((sr_f8_adamw_kernel<false>), dim3(n_blocks),
                             dim3(F8_THREADS), 0, stream, batch, beta1, beta2,
                             eps, grad_scale, norm_sq, max_norm, skip_nonfinite,
                             key);
        }
      });
}
