// Host-side launch cutting shared by the batched ("multi-tensor") kernels.
//
// A batch descriptor is a POD passed BY VALUE as the kernel argument. It
// holds up to MAX_T entries `t[]`, a packed u8 block -> entry map
// `block_tensor[]` for up to MAX_B blocks, the span size `span` and
// `partial_base`, the global index of the launch's block 0. A "span" is a
// contiguous run of one tensor handled by one block; every entry carries the
// `span_bias` that turns a block index into its span index, so one tensor
// may continue across launches.
#pragma once

#include <string.h>

// u8 entry index of this block, read from a packed block -> entry map
__device__ __forceinline__ int mt_block_entry(const unsigned int* block_tensor) {
  const unsigned blk = blockIdx.x;
  return (int)((block_tensor[blk >> 2] >> ((blk & 3u) * 8u)) & 0xffu);
}

inline long long mt_spans_of(long long size, long long span) {
  return (size + span - 1) / span;
}

// Cuts a list of `n` tensors of `size[i]` units (elements or bytes) into
// launches of at most MAX_B spans over at most MAX_T entries.
// fill(i, entry) sets everything but span_bias; launch(batch, n_blocks) fires
// one kernel. Zero-size tensors are skipped. Nothing here allocates, copies
// or synchronises.
template <class Batch, int MAX_T, int MAX_B, class Fill, class Launch>
void mt_cut_launches(int n, const long long* size, long long span, Fill fill,
                     Launch launch) {
  static_assert(MAX_T <= 256, "block->entry map is u8");
  Batch batch;
  memset(&batch, 0, sizeof(batch));
  batch.span = span;
  int nt = 0, nb = 0;
  long long global_block = 0;
  auto flush = [&]() {
    if (nb == 0) return;
    batch.partial_base = (int)global_block;
    launch(batch, nb);
    global_block += nb;
    memset(&batch, 0, sizeof(batch));
    batch.span = span;
    nt = nb = 0;
  };
  for (int i = 0; i < n; ++i) {
    if (size[i] <= 0) continue;
    const long long spans = mt_spans_of(size[i], span);
    long long s = 0;
    while (s < spans) {
      if (nt == MAX_T || nb == MAX_B) flush();
      long long take = spans - s;
      if (take > MAX_B - nb) take = MAX_B - nb;
      auto& e = batch.t[nt];
      fill(i, e);
      e.span_bias = (int)(s - nb);
      for (long long k = 0; k < take; ++k) {
        const unsigned blk = (unsigned)(nb + k);
        batch.block_tensor[blk >> 2] |= (unsigned)nt << ((blk & 3u) * 8u);
      }
      nb += (int)take;
      nt += 1;
      s += take;
    }
  }
  flush();
}
