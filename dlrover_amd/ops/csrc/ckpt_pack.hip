// Flash-checkpoint pack kernel: a batched HBM->HBM copy that also produces a
// per-tensor checksum from the words it already holds in registers.
//
// Checksum of one tensor's nbytes (zero-extended to a multiple of 4, read as
// little-endian u32 words w_0..w_{W-1}), both sums mod 2^64:
//     A = sum w_i            B = sum (2i+1) * w_i
// It is plain modular integer arithmetic, so any partition of the words over
// blocks and launches gives the same bits; no atomics are needed and none are
// used: every block plain-stores the pair of its span into its own slot and
// a finalize kernel adds each tensor's run of slots.
//
// One kernel serves three uses, chosen by the pointers alone:
//     pack    src = tensor,           dst = staging + offset
//     unpack  src = staging + offset, dst = tensor
//     verify  dst = nullptr (read and sum only)
//
// The batch descriptor is passed by value and cut into launches by
// mt_cut_launches, exactly like MTBatch in multi_tensor.hip.
#include "kern_common.h"
#include "mt_launch.h"

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
// the same 16 bytes without an alignment promise: gfx950 serves misaligned
// global accesses in hardware, and given this type the compiler still emits
// one 16-byte load or store per access instead of assuming alignment
typedef unsigned int u32x4_u __attribute__((ext_vector_type(4), aligned(1)));
typedef unsigned long long u64;

#define CK_MAX_TENSORS 32
#define CK_MAX_BLOCKS 1024
#define CK_THREADS 512
// one trip of a block: every lane moves 16 bytes
#define CK_QUANTUM (CK_THREADS * 16)
// src or dst is not 16-byte aligned: 16-byte accesses go through u32x4_u
#define CK_FLAG_UNALIGNED 1

struct CkTensor {
  const void* src;
  void* dst;  // nullptr: checksum only
  long long nbytes;
  int span_bias;  // span index within the tensor = blockIdx.x + span_bias
  int flags;
};

struct CkBatch {
  CkTensor t[CK_MAX_TENSORS];
  unsigned int block_tensor[CK_MAX_BLOCKS / 4];  // u8 entry index per block
  long long span;                                // bytes per span
  int partial_base;  // global block index of this launch's block 0
  int pad_;
};

// kernel-argument limit; leave room for the other (and hidden) arguments
static_assert(sizeof(CkBatch) <= 4096 - 512, "CkBatch must fit kernel args");

// tensors per finalize launch
#define CK_FIN_MAX 256

struct CkFinBatch {
  int first_slot[CK_FIN_MAX];
  int n_slots[CK_FIN_MAX];
  int tensor_base;  // row of sums[] that block 0 writes
  int pad_;
};

static_assert(sizeof(CkFinBatch) <= 4096 - 512,
              "CkFinBatch must fit kernel args");

// Adds (a, b) over the block; the totals are valid in thread 0. `scratch`
// holds 2 * (blockDim.x / 64) words.
__device__ __forceinline__ void ck_block_reduce(u64& a, u64& b, u64* scratch) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_xor(a, off, WAVE_SIZE);
    b += __shfl_xor(b, off, WAVE_SIZE);
  }
  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  const int wid = threadIdx.x >> 6;
  const int nwaves = (blockDim.x + WAVE_SIZE - 1) >> 6;
  if (lane == 0) {
    scratch[2 * wid] = a;
    scratch[2 * wid + 1] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    a = 0;
    b = 0;
    for (int i = 0; i < nwaves; ++i) {
      a += scratch[2 * i];
      b += scratch[2 * i + 1];
    }
  }
}

// The four words of 16-byte vector `vi` of the span: s0 += sum w,
// s1 += sum j * w with the span-local word index j = 4 * vi + k. One
// 32x32->64 multiply-add and one add per word.
__device__ __forceinline__ void ck_acc(const u32x4 v, unsigned vi, u64& s0,
                                       u64& s1) {
  const unsigned j = vi * 4u;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    s0 += (u64)v[k];
    s1 += (u64)(j + (unsigned)k) * (u64)v[k];
  }
}

// The whole 16-byte vectors of a span, through V = u32x4 (both pointers
// 16-byte aligned) or u32x4_u (any alignment). Four independent trips: the
// loads of one iteration do not wait for each other's sums (as
// mt_sqnorm_kernel).
template <class V>
__device__ __forceinline__ void ck_vec_body(const unsigned char* src,
                                            unsigned char* dst, unsigned vecs,
                                            u64 s0[4], u64 s1[4]) {
  const V* vsrc = reinterpret_cast<const V*>(src);
  V* vdst = reinterpret_cast<V*>(dst);
  unsigned i = threadIdx.x;
  for (; i + 3 * CK_THREADS < vecs; i += 4 * CK_THREADS) {
    u32x4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = vsrc[i + u * CK_THREADS];
    if (dst) {
#pragma unroll
      for (int u = 0; u < 4; ++u) vdst[i + u * CK_THREADS] = v[u];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) ck_acc(v[u], i + u * CK_THREADS, s0[u], s1[u]);
  }
  for (; i < vecs; i += CK_THREADS) {
    const u32x4 v = vsrc[i];
    if (dst) vdst[i] = v;
    ck_acc(v, i, s0[0], s1[0]);
  }
}

__global__ __launch_bounds__(CK_THREADS) void ckpt_copy_sum_kernel(
    const CkBatch b, u64* __restrict__ partials) {
  __shared__ u64 scratch[2 * (CK_THREADS / WAVE_SIZE)];
  const CkTensor& e = b.t[mt_block_entry(b.block_tensor)];
  const long long start = ((long long)blockIdx.x + e.span_bias) * b.span;
  long long n = e.nbytes - start;  // bytes of this span, > 0
  if (n > b.span) n = b.span;
  const unsigned char* __restrict__ src = (const unsigned char*)e.src + start;
  unsigned char* __restrict__ dst =
      e.dst ? (unsigned char*)e.dst + start : nullptr;

  // the span is below 2^31 bytes (checked by the host), so span-local vector
  // and word indices fit 32 bits
  const unsigned vecs = (unsigned)(n >> 4);
  u64 s0[4] = {0, 0, 0, 0}, s1[4] = {0, 0, 0, 0};
  if (e.flags & CK_FLAG_UNALIGNED)
    ck_vec_body<u32x4_u>(src, dst, vecs, s0, s1);
  else
    ck_vec_body<u32x4>(src, dst, vecs, s0, s1);

  // Word-wise path for the at most 15 bytes after the last whole vector.
  // Words are assembled from the widest loads that both pointers allow;
  // bytes at and past `n` are taken as zero and never read (staging padding
  // is uninitialised).
  const unsigned nwords = (unsigned)((n + 3) >> 2);
  const unsigned align =
      (unsigned)(((uintptr_t)src | (uintptr_t)dst) & 3u);  // nullptr adds 0
  for (unsigned j = vecs * 4u + threadIdx.x; j < nwords; j += CK_THREADS) {
    const long long off = (long long)j * 4;
    const long long left = n - off;  // >= 1
    unsigned w = 0;
    if (left >= 4 && align == 0) {
      w = *reinterpret_cast<const unsigned*>(src + off);
      if (dst) *reinterpret_cast<unsigned*>(dst + off) = w;
    } else if (left >= 4 && (align & 1u) == 0) {
      const unsigned short lo =
          *reinterpret_cast<const unsigned short*>(src + off);
      const unsigned short hi =
          *reinterpret_cast<const unsigned short*>(src + off + 2);
      if (dst) {
        *reinterpret_cast<unsigned short*>(dst + off) = lo;
        *reinterpret_cast<unsigned short*>(dst + off + 2) = hi;
      }
      w = (unsigned)lo | ((unsigned)hi << 16);
    } else {
      const int nb = left >= 4 ? 4 : (int)left;
      for (int k = 0; k < nb; ++k) {
        const unsigned char c = src[off + k];
        if (dst) dst[off + k] = c;
        w |= (unsigned)c << (8 * k);
      }
    }
    s0[0] += (u64)w;
    s1[0] += (u64)j * (u64)w;
  }

  u64 a = (s0[0] + s0[1]) + (s0[2] + s0[3]);
  u64 s = (s1[0] + s1[1]) + (s1[2] + s1[3]);
  ck_block_reduce(a, s, scratch);
  if (threadIdx.x == 0) {
    // fold the span's first word index in once: sum (2 (base + j) + 1) w
    const u64 base = (u64)start >> 2;
    const long long slot = (long long)b.partial_base + blockIdx.x;
    partials[2 * slot] = a;
    partials[2 * slot + 1] = (2ull * base + 1ull) * a + 2ull * s;
  }
}

// One block per tensor: adds the tensor's contiguous run of slots. A tensor
// without slots (zero bytes) gets (0, 0), so every row of sums is written.
__global__ __launch_bounds__(256) void ckpt_sum_finalize_kernel(
    const CkFinBatch f, const u64* __restrict__ partials,
    u64* __restrict__ sums) {
  __shared__ u64 scratch[2 * (256 / WAVE_SIZE)];
  const long long first = f.first_slot[blockIdx.x];
  const int count = f.n_slots[blockIdx.x];
  u64 a = 0, b = 0;
  for (int k = threadIdx.x; k < count; k += 256) {
    a += partials[2 * (first + k)];
    b += partials[2 * (first + k) + 1];
  }
  ck_block_reduce(a, b, scratch);
  if (threadIdx.x == 0) {
    const long long row = (long long)f.tensor_base + blockIdx.x;
    sums[2 * row] = a;
    sums[2 * row + 1] = b;
  }
}

// ---------------------------------------------------------------------------
// host side. Nothing here allocates, copies to the host or synchronises, so
// callers may capture these launches into a graph.
// ---------------------------------------------------------------------------

namespace {

inline bool ck_misaligned16(const void* p) {
  return p != nullptr && ((uintptr_t)p & 15u) != 0;
}

}  // namespace

extern "C" int ckpt_span_quantum() { return CK_QUANTUM; }
extern "C" int ckpt_max_blocks() { return CK_MAX_BLOCKS; }

// Span for a whole list: about 2048 blocks in total (the grid_capped rule), a
// multiple of the block's 8 KiB trip, at most CK_SPAN_CAP so that a large
// state still fills every launch with CK_MAX_BLOCKS blocks.
#define CK_SPAN_CAP (1ll << 20)
extern "C" long long ckpt_auto_span(long long total_bytes) {
  long long span = (total_bytes + 2047) / 2048;
  span = (span + CK_QUANTUM - 1) / CK_QUANTUM * CK_QUANTUM;
  if (span < CK_QUANTUM) span = CK_QUANTUM;
  return span > CK_SPAN_CAP ? CK_SPAN_CAP : span;
}

extern "C" long long ckpt_num_slots(int n, const long long* nbytes,
                                    long long span) {
  long long total = 0;
  for (int i = 0; i < n; ++i)
    if (nbytes[i] > 0) total += mt_spans_of(nbytes[i], span);
  return total;
}

// partials: [slots, 2] words, slots = ckpt_num_slots(...); sums: [n, 2].
extern "C" void ckpt_copy_sum_launch(int n, const void* const* src,
                                     void* const* dst, const long long* nbytes,
                                     long long span, long long* partials,
                                     long long* sums, hipStream_t stream) {
  mt_cut_launches<CkBatch, CK_MAX_TENSORS, CK_MAX_BLOCKS>(
      n, nbytes, span,
      [&](int i, CkTensor& e) {
        e.src = src[i];
        e.dst = dst ? dst[i] : nullptr;
        e.nbytes = nbytes[i];
        e.flags = (ck_misaligned16(e.src) || ck_misaligned16(e.dst))
                      ? CK_FLAG_UNALIGNED
                      : 0;
      },
      [&](const CkBatch& batch, int n_blocks) {
        hipLaunchKernelGGL(ckpt_copy_sum_kernel, dim3(n_blocks),
                           dim3(CK_THREADS), 0, stream, batch, (u64*)partials);
      });
  long long slot = 0;
  for (int t0 = 0; t0 < n; t0 += CK_FIN_MAX) {
    CkFinBatch f;
    memset(&f, 0, sizeof(f));
    f.tensor_base = t0;
    const int m = n - t0 < CK_FIN_MAX ? n - t0 : CK_FIN_MAX;
    for (int k = 0; k < m; ++k) {
      const long long nb = nbytes[t0 + k];
      const long long spans = nb > 0 ? mt_spans_of(nb, span) : 0;
      f.first_slot[k] = (int)slot;
      f.n_slots[k] = (int)spans;
      slot += spans;
    }
    hipLaunchKernelGGL(ckpt_sum_finalize_kernel, dim3(m), dim3(256), 0, stream,
                       f, (const u64*)partials, (u64*)sums);
  }
}
