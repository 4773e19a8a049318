// Building blocks shared by the flash-attention kernels: vector typedefs, the
// LDS swizzle, and the register-fragment helpers of the 32x32x16 MFMA kernels
// (attention_v3.hip, attention_bwd_v3.hip). Fragment layouts and the tr_b16
// gather semantics are hardware-verified (tests/test_mfma_gpu.py,
// profiles/r02a_fa_v3.txt).
#pragma once

#include "kern_common.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2_t;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;

// XOR swizzle on a byte offset within an LDS row (guide G4): the 16 B chunk
// index is XORed with the low three row bits, so a column of b128 reads
// spreads over the banks.
__device__ __forceinline__ int swz(int row, int byte_col) {
  return byte_col ^ ((row & 7) << 4);
}

// pack two fp32 into one u32 of two bf16 (compiler emits v_cvt_pk_bf16_f32)
__device__ __forceinline__ unsigned pack_bf16(float lo, float hi) {
  bf16x2 v = {(__bf16)lo, (__bf16)hi};
  return *reinterpret_cast<unsigned*>(&v);
}

// A-operand fragment X^T[d = n*32 + (l&31)][row = rb + half*8 + i] read from
// a ROW-major swz-swizzled [rows][128] bf16 LDS tile via two cooperative
// ds_read_b64_tr_b16 gathers. Semantics probe-pinned (profiles/r02a): the
// 16-lane group's addresses form a gather table — lane l supplies the word
// address for (row rb + ((l&15)>>2), d-quad base+(l&3)) and receives, as
// element j, its OWN d column of row rb + j (slots 4j + ((l>>2)&3)).
// Because a lane's data comes from addresses its NEIGHBOURS supply (only
// address bits 1-2 act per lane), a layout in which each lane points at a
// 4x4 tile of its own returns wrong columns for every lane but the first
// four of a group: the 16 lanes have to lay out one shared table, as here.
__device__ __forceinline__ bf16x8 tr_colT_frag(const char* lds, int rb,
                                               int n, int lane, int half) {
  const int j = (lane & 15) >> 2;
  const int dq = n * 8 + ((lane & 16) >> 2) + (lane & 3);
  const int r0 = rb + half * 8 + j;
  const int r1 = r0 + 4;
  const unsigned base = (unsigned)(uintptr_t)lds;
  const unsigned a0 = base + r0 * 256 + ((dq * 8) ^ ((r0 & 7) << 4));
  const unsigned a1 = base + r1 * 256 + ((dq * 8) ^ ((r1 & 7) << 4));
  u32x2_t w0, w1;
  asm volatile(
      "ds_read_b64_tr_b16 %0, %2\n\t"
      "ds_read_b64_tr_b16 %1, %3\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=v"(w0), "=v"(w1)
      : "v"(a0), "v"(a1));
  u32x4_t frag = u32x4_t{w0.x, w0.y, w1.x, w1.y};
  return *reinterpret_cast<bf16x8*>(&frag);
}

// B-operand fragments [16 rows, 32 cols] assembled IN REGISTERS from C-form
// per-lane values v16 (16 f32, C rows (r&3)+8*(r>>2)+4*half, col = lane-own):
// two k-slices of 16 rows each, pairs packed to bf16 and ONE permlane32_swap
// per register pair. Slice ks2 uses own regs r0 = ks2*8 .. +8: regs r0+0..3
// are rows base+(0..3), r0+4..7 rows base+(8..11), base = ks2*16 + 4*half;
// the partner lane (l^32) holds the rows 4 further on.
// swap(vdst, vsrc) exchanges vdst's lanes 32-63 with vsrc's 0-31:
//   .x (new w0): h0 lanes own rows(+0,1); h1 lanes partner rows(+8,9)
//   .y (new w2): h0 lanes partner rows(+4,5); h1 lanes own rows(+12,13)
// so [x0, x1, y0, y1] is, for BOTH halves, the lane's 8 rows
// (half*8 .. half*8+8) of the 16-row slice — exactly the B fragment.
__device__ __forceinline__ void pairswap_frags(const float v16[16],
                                               bf16x8 out[2]) {
#pragma unroll
  for (int ks2 = 0; ks2 < 2; ++ks2) {
    const int r0 = ks2 * 8;
    unsigned w0 = pack_bf16(v16[r0 + 0], v16[r0 + 1]);
    unsigned w1 = pack_bf16(v16[r0 + 2], v16[r0 + 3]);
    unsigned w2 = pack_bf16(v16[r0 + 4], v16[r0 + 5]);
    unsigned w3 = pack_bf16(v16[r0 + 6], v16[r0 + 7]);
    u32x2_t s0 = __builtin_amdgcn_permlane32_swap(w0, w2, false, false);
    u32x2_t s1 = __builtin_amdgcn_permlane32_swap(w1, w3, false, false);
    u32x4_t frag = u32x4_t{s0.x, s1.x, s0.y, s1.y};
    out[ks2] = *reinterpret_cast<bf16x8*>(&frag);
  }
}
