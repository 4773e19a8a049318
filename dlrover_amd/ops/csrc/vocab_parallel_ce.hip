// Vocab-parallel fused cross-entropy: each tensor-parallel rank holds a
// [N, Vs] column shard of the bf16 logits (Vs = V / tp) and no rank ever sees
// a whole row, so the softmax is split around ONE collective:
//
//   ce_shard_stats   one read of the shard  -> stats[N,3] = (m, s, t)
//                    m = shard max, s = sum exp(x - m), t = target logit or 0
//   (all-gather of the tiny [N,3] stats over the TP group, done by the caller)
//   ce_shard_finish  combines stats_all[tp,N,3] in rank order r = 0..tp-1:
//                    M = max m_r, S = sum s_r exp(m_r - M), lse = M + log S,
//                    loss = lse - sum t_r; then one read + one write of the
//                    shard: dlogit = (exp(x - lse) - onehot) * grad_scale,
//                    in place.
//
// Two reads and one write of V/tp columns per rank, against three reads and
// one write of V in cross_entropy.hip. No atomics and a fixed combine order:
// every rank derives bitwise the same loss from the same gathered buffer.
// Targets are GLOBAL vocabulary ids; a shard owns a target iff
// 0 <= target - vocab_start < Vs, and only then is it used as a column index.
// Finite logits are assumed, as in cross_entropy.hip.
#include "kern_common.h"

extern "C" {

__global__ void ce_shard_stats_kernel(
    const short* __restrict__ logits, const int* __restrict__ targets,
    float* __restrict__ stats, long long n_rows, int vs, int vocab_start,
    int ignore_index) {
  __shared__ float scratch[16];
  const int vecs = vs >> 3;  // vs % 8 == 0 is checked by the binding
  for (long long row = blockIdx.x; row < n_rows; row += gridDim.x) {
    const short* r = logits + row * vs;
    // online max/sum: one pass over the shard, rescaling the running sum
    // whenever a vector raises the running max
    float m = -INFINITY, s = 0.f;
    for (int v = threadIdx.x; v < vecs; v += blockDim.x) {
      float xv[8];
      load8(r + v * 8, xv);
      float vm = xv[0];
#pragma unroll
      for (int j = 1; j < 8; ++j) vm = fmaxf(vm, xv[j]);
      if (vm > m) {
        s = (m == -INFINITY) ? 0.f : s * __expf(m - vm);
        m = vm;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) s += __expf(xv[j] - m);
    }
    const float bm = block_reduce_max(m, scratch);
    // threads that saw no vector (vecs < blockDim.x) carry m == -inf, s == 0
    const float part = (m == -INFINITY) ? 0.f : s * __expf(m - bm);
    const float bs = block_reduce_sum(part, scratch);
    if (threadIdx.x == 0) {
      const int tgt = targets[row];
      const int local = tgt - vocab_start;
      const bool owns = tgt != ignore_index && local >= 0 && local < vs;
      float* o = stats + row * 3;
      o[0] = bm;
      o[1] = bs;
      o[2] = owns ? bf2f(r[local]) : 0.f;
    }
  }
}

__global__ void ce_shard_finish_kernel(
    short* __restrict__ logits, const int* __restrict__ targets,
    const float* __restrict__ stats_all, float* __restrict__ losses,
    long long n_rows, int vs, int vocab_start, int tp, int ignore_index,
    float grad_scale, int compute_grad) {
  const int vecs = vs >> 3;
  for (long long row = blockIdx.x; row < n_rows; row += gridDim.x) {
    short* r = logits + row * vs;
    const int tgt = targets[row];
    if (tgt == ignore_index) {
      if (compute_grad) {
        for (int v = threadIdx.x; v < vecs; v += blockDim.x) {
          float z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
          store8(r + v * 8, z);
        }
      }
      if (threadIdx.x == 0) losses[row] = 0.f;
      continue;
    }
    // every thread combines the tp stats itself (uniform addresses: one
    // broadcast load each), in rank order, so no block reduction is needed
    float gm = -INFINITY;
    for (int k = 0; k < tp; ++k)
      gm = fmaxf(gm, stats_all[((long long)k * n_rows + row) * 3]);
    float gs = 0.f, gt = 0.f;
    for (int k = 0; k < tp; ++k) {
      const float* st = stats_all + ((long long)k * n_rows + row) * 3;
      gs += st[1] * __expf(st[0] - gm);
      gt += st[2];
    }
    const float lse = gm + logf(gs);
    if (threadIdx.x == 0) losses[row] = lse - gt;
    if (compute_grad) {
      // -1 when another shard owns the target: matches no column below
      const int local = tgt - vocab_start;
      const int hot = (local >= 0 && local < vs) ? local : -1;
      for (int v = threadIdx.x; v < vecs; v += blockDim.x) {
        float xv[8], ov[8];
        load8(r + v * 8, xv);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float p = __expf(xv[j] - lse);
          ov[j] = (p - (v * 8 + j == hot ? 1.f : 0.f)) * grad_scale;
        }
        store8(r + v * 8, ov);
      }
    }
  }
}

static int ce_shard_grid(long long n_rows) {
  int grid = n_rows < 2048 ? (int)n_rows : 2048;
  return grid < 1 ? 1 : grid;
}

void ce_shard_stats_launch(const void* logits, const void* targets,
                           void* stats, long long n_rows, int vs,
                           int vocab_start, int ignore_index,
                           hipStream_t stream) {
  hipLaunchKernelGGL(ce_shard_stats_kernel, dim3(ce_shard_grid(n_rows)),
                     dim3(512), 0, stream, (const short*)logits,
                     (const int*)targets, (float*)stats, n_rows, vs,
                     vocab_start, ignore_index);
}

void ce_shard_finish_launch(void* logits, const void* targets,
                            const void* stats_all, void* losses,
                            long long n_rows, int vs, int vocab_start, int tp,
                            int ignore_index, float grad_scale,
                            int compute_grad, hipStream_t stream) {
  hipLaunchKernelGGL(ce_shard_finish_kernel, dim3(ce_shard_grid(n_rows)),
                     dim3(512), 0, stream, (short*)logits,
                     (const int*)targets, (const float*)stats_all,
                     (float*)losses, n_rows, vs, vocab_start, tp,
                     ignore_index, grad_scale, compute_grad);
}

}  // extern "C"
