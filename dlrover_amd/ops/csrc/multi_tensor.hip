// Multi-tensor (batched) kernels: global gradient squared-norm and AdamW.
//
// One launch covers up to MT_MAX_TENSORS tensors. The batch descriptor is a
// POD passed BY VALUE as the kernel argument — there is no table in device
// memory: with zero_grad(set_to_none=True) the gradient pointers change
// every step, and a device table would need an upload plus a lifetime rule
// per step. The kernel-argument segment is limited to 4096 B, which is what
// bounds tensors and blocks per launch.
//
// A "span" is a contiguous run of one tensor handled by one block. The
// descriptor maps block -> tensor (packed u8) and each tensor entry carries
// the bias that turns a block index into its span index, so one tensor may
// continue across launches.
//
// The squared norm uses no atomics: every block plain-stores one fp32
// partial into its own slot and a single-block finalize adds the slots in a
// fixed order (fp64), so the norm — and with it every clipped update — is
// bitwise reproducible from run to run.
#include "kern_common.h"
#include "mt_launch.h"

typedef __attribute__((ext_vector_type(4))) float f32x4;

#define MT_MAX_TENSORS 32
#define MT_MAX_BLOCKS 1024
// 512 threads x 1024 blocks puts as many waves in flight per launch as the
// per-parameter adamw_kernel's 256 x 2048
#define MT_THREADS 512
#define MT_FLAG_BF16 1
#define MT_FLAG_UNALIGNED 2

struct MTTensor {
  float* master;
  const void* grad;
  float* exp_avg;
  float* exp_avg_sq;
  short* param_bf16;
  long long numel;
  float lr, weight_decay, bc1, bc2;
  int span_bias;  // span index within the tensor = blockIdx.x + span_bias
  int flags;
};

struct MTBatch {
  MTTensor t[MT_MAX_TENSORS];
  unsigned int block_tensor[MT_MAX_BLOCKS / 4];  // u8 tensor index per block
  long long span;                                // elements per span
  int partial_base;  // global block index of this launch's block 0
  int pad_;
};

// kernel-argument limit; leave room for the other (and hidden) arguments
static_assert(sizeof(MTBatch) <= 4096 - 512, "MTBatch must fit kernel args");

__device__ __forceinline__ int mt_block_tensor(const MTBatch& b) {
  return mt_block_entry(b.block_tensor);
}

// ---------------------------------------------------------------------------
// squared norm
// ---------------------------------------------------------------------------

// sum of squares of 8 consecutive elements (one or two 16-byte loads)
__device__ __forceinline__ float sq8_bf16(const short* p) {
  float x[8];
  load8(p, x);
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) s += x[j] * x[j];
  return s;
}

__device__ __forceinline__ float sq8_f32(const float* p) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(p);
  const f32x4 b = *reinterpret_cast<const f32x4*>(p + 4);
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) s += a[j] * a[j];
#pragma unroll
  for (int j = 0; j < 4; ++j) s += b[j] * b[j];
  return s;
}

__global__ __launch_bounds__(MT_THREADS) void mt_sqnorm_kernel(
    const MTBatch b, float* __restrict__ partials) {
  __shared__ float scratch[MT_THREADS / WAVE_SIZE];
  const MTTensor& e = b.t[mt_block_tensor(b)];
  const long long start = ((long long)blockIdx.x + e.span_bias) * b.span;
  long long n = e.numel - start;
  if (n > b.span) n = b.span;
  const int flags = e.flags;
  const long long vecs = (flags & MT_FLAG_UNALIGNED) ? 0 : (n >> 3);
  // four independent accumulators: the loads of one trip do not wait for
  // each other's adds (a single chain leaves the read latency exposed). The
  // order of every add is fixed by the indices alone.
  float acc4[4] = {0.f, 0.f, 0.f, 0.f};
  long long i = threadIdx.x;
  if (flags & MT_FLAG_BF16) {
    const short* g = (const short*)e.grad + start;
    for (; i + 3 * MT_THREADS < vecs; i += 4 * MT_THREADS) {
#pragma unroll
      for (int u = 0; u < 4; ++u) acc4[u] += sq8_bf16(g + (i + u * MT_THREADS) * 8);
    }
    for (; i < vecs; i += MT_THREADS) acc4[0] += sq8_bf16(g + i * 8);
    for (i = vecs * 8 + threadIdx.x; i < n; i += MT_THREADS) {
      const float x = bf2f(g[i]);
      acc4[0] += x * x;
    }
  } else {
    const float* g = (const float*)e.grad + start;
    for (; i + 3 * MT_THREADS < vecs; i += 4 * MT_THREADS) {
#pragma unroll
      for (int u = 0; u < 4; ++u) acc4[u] += sq8_f32(g + (i + u * MT_THREADS) * 8);
    }
    for (; i < vecs; i += MT_THREADS) acc4[0] += sq8_f32(g + i * 8);
    for (i = vecs * 8 + threadIdx.x; i < n; i += MT_THREADS) {
      const float x = g[i];
      acc4[0] += x * x;
    }
  }
  const float acc = (acc4[0] + acc4[1]) + (acc4[2] + acc4[3]);
  const float total = block_reduce_sum(acc, scratch);
  if (threadIdx.x == 0) partials[b.partial_base + blockIdx.x] = total;
}

// One block; thread t adds partials t, t+256, ... (four interleaved chains)
// and the 256 sums go through a fixed tree: the order never depends on
// timing.
__global__ __launch_bounds__(256) void mt_sqnorm_finalize_kernel(
    const float* __restrict__ partials, int n_partials,
    float* __restrict__ norm_sq) {
  __shared__ double sh[256];
  double a4[4] = {0.0, 0.0, 0.0, 0.0};
  int i = threadIdx.x;
  for (; i + 3 * 256 < n_partials; i += 4 * 256) {
#pragma unroll
    for (int u = 0; u < 4; ++u) a4[u] += (double)partials[i + u * 256];
  }
  for (; i < n_partials; i += 256) a4[0] += (double)partials[i];
  sh[threadIdx.x] = (a4[0] + a4[1]) + (a4[2] + a4[3]);
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) norm_sq[0] = (float)sh[0];
}

// ---------------------------------------------------------------------------
// AdamW over a batch. Same math as adamw_kernel (adamw.hip): 8 elements per
// thread-iteration, two b128 chains per array, scalar tail.
// ---------------------------------------------------------------------------

template <bool GRAD_BF16>
__global__ __launch_bounds__(MT_THREADS) void mt_adamw_kernel(
    const MTBatch b, float beta1, float beta2, float eps, float grad_scale,
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

  const MTTensor& e = b.t[mt_block_tensor(b)];
  const long long start = ((long long)blockIdx.x + e.span_bias) * b.span;
  long long n = e.numel - start;
  if (n > b.span) n = b.span;
  float* __restrict__ param = e.master + start;
  float* __restrict__ exp_avg = e.exp_avg + start;
  float* __restrict__ exp_avg_sq = e.exp_avg_sq + start;
  short* __restrict__ param_bf16 = e.param_bf16 ? e.param_bf16 + start : nullptr;
  const void* grad_in = GRAD_BF16 ? (const void*)((const short*)e.grad + start)
                                  : (const void*)((const float*)e.grad + start);
  const float lr = e.lr, weight_decay = e.weight_decay;
  const float bc1 = e.bc1, bc2 = e.bc2;

  const long long vecs = (e.flags & MT_FLAG_UNALIGNED) ? 0 : (n >> 3);
  for (long long i = threadIdx.x; i < vecs; i += MT_THREADS) {
    f32x4 p[2], m[2], v[2];
    float g[8];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      p[h] = *reinterpret_cast<f32x4*>(param + i * 8 + h * 4);
      m[h] = *reinterpret_cast<f32x4*>(exp_avg + i * 8 + h * 4);
      v[h] = *reinterpret_cast<f32x4*>(exp_avg_sq + i * 8 + h * 4);
    }
    if (GRAD_BF16) {
      short8_t gv = *reinterpret_cast<const short8_t*>(
          (const short*)grad_in + i * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) g[j] = bf2f(gv[j]) * gs;
    } else {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        f32x4 gv =
            *reinterpret_cast<const f32x4*>((const float*)grad_in + i * 8 + h * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) g[h * 4 + j] = gv[j] * gs;
      }
    }
    short8_t pb;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float gj = g[h * 4 + j];
        m[h][j] = beta1 * m[h][j] + (1.f - beta1) * gj;
        v[h][j] = beta2 * v[h][j] + (1.f - beta2) * gj * gj;
        const float mhat = m[h][j] * bc1;
        const float vhat = v[h][j] * bc2;
        p[h][j] -= lr * (mhat / (sqrtf(vhat) + eps) + weight_decay * p[h][j]);
        pb[h * 4 + j] = f2bf(p[h][j]);
      }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      *reinterpret_cast<f32x4*>(param + i * 8 + h * 4) = p[h];
      *reinterpret_cast<f32x4*>(exp_avg + i * 8 + h * 4) = m[h];
      *reinterpret_cast<f32x4*>(exp_avg_sq + i * 8 + h * 4) = v[h];
    }
    if (param_bf16)
      *reinterpret_cast<short8_t*>(param_bf16 + i * 8) = pb;
  }
  // scalar tail (n % 8), or the whole span of a tensor that is not 16-byte
  // aligned
  for (long long i = vecs * 8 + threadIdx.x; i < n; i += MT_THREADS) {
    float g = GRAD_BF16 ? bf2f(((const short*)grad_in)[i])
                        : ((const float*)grad_in)[i];
    g *= gs;
    float m = beta1 * exp_avg[i] + (1.f - beta1) * g;
    float v = beta2 * exp_avg_sq[i] + (1.f - beta2) * g * g;
    float p = param[i];
    p -= lr * ((m * bc1) / (sqrtf(v * bc2) + eps) + weight_decay * p);
    param[i] = p;
    exp_avg[i] = m;
    exp_avg_sq[i] = v;
    if (param_bf16) param_bf16[i] = f2bf(p);
  }
}

// ---------------------------------------------------------------------------
// host side: cut a tensor list into launches. Nothing here allocates, copies
// or synchronises, so callers may capture these launches into a graph.
// ---------------------------------------------------------------------------

namespace {

inline bool misaligned16(const void* p) {
  return p != nullptr && ((uintptr_t)p & 15u) != 0;
}

// fill(i, entry) sets everything but numel and span_bias; launch(batch,
// n_blocks) fires one kernel. Zero-numel tensors are skipped. The cutting
// itself is mt_cut_launches (mt_launch.h), shared with ckpt_pack.hip.
template <class Fill, class Launch>
void mt_for_each_launch(int n, const long long* numel, long long span,
                        Fill fill, Launch launch) {
  mt_cut_launches<MTBatch, MT_MAX_TENSORS, MT_MAX_BLOCKS>(
      n, numel, span,
      [&](int i, MTTensor& e) {
        fill(i, e);
        e.numel = numel[i];
      },
      launch);
}

}  // namespace

extern "C" int mt_max_tensors() { return MT_MAX_TENSORS; }

// Span for a whole list: the grid_capped rule (about 2048 blocks in total),
// a multiple of 8 elements, never less than one block's worth of vector
// work — and never more than MT_SPAN_CAP. Without the cap a large model's
// ~2048 blocks are spread over total_tensors / MT_MAX_TENSORS launches that
// each fill a fraction of the GPU: measured on small_1b shapes (135 tensors,
// 1.12 G params, MI355X) the uncapped rule ran the update at 1.12x the
// per-parameter path and 65536 at 0.95x (16384: 0.97x); see
// profiles/adamw_multi_tensor.txt.
#define MT_SPAN_CAP 65536
extern "C" long long mt_auto_span(long long total_numel) {
  long long span = (total_numel + 2047) / 2048;
  span = (span + 7) / 8 * 8;
  const long long floor_span = (long long)MT_THREADS * 8;
  if (span < floor_span) span = floor_span;
  return span > MT_SPAN_CAP ? MT_SPAN_CAP : span;
}

extern "C" long long mt_num_blocks(int n, const long long* numel,
                                   long long span) {
  long long total = 0;
  for (int i = 0; i < n; ++i)
    if (numel[i] > 0) total += mt_spans_of(numel[i], span);
  return total;
}

extern "C" void mt_sqnorm_launch(int n, const void* const* ptrs,
                                 const long long* numel, const int* is_bf16,
                                 long long span, float* partials,
                                 float* norm_sq, hipStream_t stream) {
  mt_for_each_launch(
      n, numel, span,
      [&](int i, MTTensor& e) {
        e.grad = ptrs[i];
        e.flags = (is_bf16[i] ? MT_FLAG_BF16 : 0) |
                  (misaligned16(ptrs[i]) ? MT_FLAG_UNALIGNED : 0);
      },
      [&](const MTBatch& batch, int n_blocks) {
        hipLaunchKernelGGL(mt_sqnorm_kernel, dim3(n_blocks), dim3(MT_THREADS),
                           0, stream, batch, partials);
      });
  const int n_partials = (int)mt_num_blocks(n, numel, span);
  hipLaunchKernelGGL(mt_sqnorm_finalize_kernel, dim3(1), dim3(256), 0, stream,
                     (const float*)partials, n_partials, norm_sq);
}

extern "C" void mt_adamw_launch(
    int n, void* const* master, const void* const* grad, void* const* exp_avg,
    void* const* exp_avg_sq, void* const* param_bf16, const long long* numel,
    const float* lr, const float* weight_decay, const int* step,
    int grad_is_bf16, float beta1, float beta2, float eps, float grad_scale,
    const float* norm_sq, float max_norm, int skip_nonfinite, long long span,
    hipStream_t stream) {
  mt_for_each_launch(
      n, numel, span,
      [&](int i, MTTensor& e) {
        e.master = (float*)master[i];
        e.grad = grad[i];
        e.exp_avg = (float*)exp_avg[i];
        e.exp_avg_sq = (float*)exp_avg_sq[i];
        e.param_bf16 = (short*)param_bf16[i];
        e.lr = lr[i];
        e.weight_decay = weight_decay[i];
        // same expressions as adamw_launch, so both paths agree bit for bit
        e.bc1 = 1.f / (1.f - powf(beta1, (float)step[i]));
        e.bc2 = 1.f / (1.f - powf(beta2, (float)step[i]));
        const bool unaligned =
            misaligned16(master[i]) || misaligned16(grad[i]) ||
            misaligned16(exp_avg[i]) || misaligned16(exp_avg_sq[i]) ||
            misaligned16(param_bf16[i]);
        e.flags = (grad_is_bf16 ? MT_FLAG_BF16 : 0) |
                  (unaligned ? MT_FLAG_UNALIGNED : 0);
      },
      [&](const MTBatch& batch, int n_blocks) {
        if (grad_is_bf16) {
          hipLaunchKernelGGL((mt_adamw_kernel<true>), dim3(n_blocks),
                             dim3(MT_THREADS), 0, stream, batch, beta1, beta2,
                             eps, grad_scale, norm_sq, max_norm,
                             skip_nonfinite);
        } else {
          hipLaunchKernelGGL((mt_adamw_kernel<false>), dim3(n_blocks),
                             dim3(MT_THREADS), 0, stream, batch, beta1, beta2,
                             eps, grad_scale, norm_sq, max_norm,
                             skip_nonfinite);
        }
      });
}
