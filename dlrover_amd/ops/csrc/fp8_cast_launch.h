// Host launchers of the FP8 tensor-wise cast kernels (fp8_cast.hip). Included
// by the .hip file that defines them and by bindings.cpp, so a signature
// mismatch is a compile error. The stream type is forward-declared exactly as
// the HIP runtime does, which keeps this header free of HIP includes.
//
// x is [R, C] contiguous, 16-byte aligned, bf16 (is_bf16) or fp32, with
// R % 16 == 0 and C % 16 == 0. fmt: 0 = OCP e4m3fn (max 448), 1 = OCP e5m2
// (max 57344). Nothing here allocates, copies or synchronises.
#pragma once

struct ihipStream_t;
typedef struct ihipStream_t* hipStream_t;

#define FP8_FMT_E4M3 0
#define FP8_FMT_E5M2 1

extern "C" {

// u32 partial slots fp8_amax_scale_launch needs for `numel` elements
long long fp8_amax_num_partials(long long numel, int is_bf16);

// scale[0] = absmax(x) / FMAX (0 when below FLT_MIN; NaN/inf propagate).
// Two kernels over `partials` (fp8_amax_num_partials u32 slots), no atomics.
void fp8_amax_scale_launch(const void* x, long long numel, int is_bf16,
                           int fmt, unsigned int* partials, float* scale,
                           hipStream_t stream);

// codes[R, C] and/or codes_t[C, R] (either may be nullptr) = RNE(x / scale[0])
// in `fmt`; all zero when scale[0] == 0. Both outputs 16-byte aligned.
void fp8_cast_transpose_launch(const void* x, const float* scale, void* codes,
                               void* codes_t, long long R, long long C,
                               int is_bf16, int fmt, hipStream_t stream);

}  // extern "C"
