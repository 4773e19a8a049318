// Device and host helpers shared by the batched AdamW kernels
// (multi_tensor.hip, adamw_fp8.hip, adamw_sr.hip): the clip coefficient, the
// FP8 block format of the moments, and the alignment rule of the launchers.
#pragma once

#include <stdint.h>

#include "kern_common.h"

typedef __attribute__((ext_vector_type(4))) float f32x4;

// Gradient scale of one batched update: grad_scale times torch's
// clip_grad_norm_ coefficient min(1, max_norm / (sqrt(norm_sq) + 1e-6)) when
// norm_sq is given. Returns false when the update must not store anything:
// an inf or NaN norm with skip_nonfinite set.
__device__ __forceinline__ bool adamw_grad_scale(const float* norm_sq,
                                                 float max_norm,
                                                 int skip_nonfinite,
                                                 float grad_scale, float& gs) {
  float coef = 1.f;
  if (norm_sq) {
    const float nsq = norm_sq[0];
    if (skip_nonfinite && !(fabsf(nsq) <= 3.402823466e+38f)) return false;
    const float c = max_norm / (sqrtf(nsq) + 1e-6f);
    coef = (c > 1.f) ? 1.f : c;  // a NaN propagates, like torch.clamp
  }
  gs = grad_scale * coef;
  return true;
}

inline bool misaligned16(const void* p) {
  return p != nullptr && ((uintptr_t)p & 15u) != 0;
}

// ---------------------------------------------------------------------------
// FP8 block-scaled moments (the format is defined in adamw_fp8.hip)
// ---------------------------------------------------------------------------

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

// e4m3fn <-> fp32, four at a time (one dword of codes)
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
  return __builtin_bit_cast(unsigned int, x) & 0x7fffffffu;
}

// v of lane (this lane ^ off): __shfl_xor over the whole wave, as a builtin
// so that it inlines into callers of any target features
__device__ __forceinline__ unsigned int wave_xor_u32(unsigned int v, int off) {
  const int lane =
      (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  return (unsigned int)__builtin_amdgcn_ds_bpermute((lane ^ off) << 2, (int)v);
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
    bits = umax(bits, wave_xor_u32(bits, off));
  scale = __builtin_bit_cast(float, bits) / F8_E4M3_MAX;
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
