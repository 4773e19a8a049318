// Host launchers of the flash-attention kernels. Included by the .hip files
// that define them and by bindings.cpp, so a signature mismatch is a compile
// error. The stream type is forward-declared exactly as the HIP runtime does,
// which keeps this header free of HIP includes.
//
// All tensors are logically [B,H,S,D] bf16 with D == 128 contiguous.
// `strides` holds 4 x (batch, head, seq) element strides: q, k, v, then out
// (forward) or dout (backward); the backward kernels store dq with q's.
// The 16x16 launchers need S % 64 == 0, the v3 (32x32) ones S % 256 == 0.
// doc_start / doc_end: int32 [B,S] contiguous, or nullptr for the causal
// kernels (see attention_v3.hip for the mask).
#pragma once

struct ihipStream_t;
typedef struct ihipStream_t* hipStream_t;

extern "C" {

void flash_attn_fwd_launch(const void* q, const void* k, const void* v,
                           void* out, void* lse, int B, int H, int HKV, int S,
                           float scale, const long long* strides,
                           hipStream_t stream);
void flash_attn_fwd_v3_launch(const void* q, const void* k, const void* v,
                              void* out, void* lse, int B, int H, int HKV,
                              int S, float scale, const long long* strides,
                              const int* doc_start, hipStream_t stream);

// Dvec[b,h,s] = rowsum(dO * O); ost / dst: (batch, head, seq) strides
void fa_bwd_pre_launch(const void* dout, const void* out, void* dvec, int B,
                       int H, int S, const long long* ost,
                       const long long* dst, hipStream_t stream);
void fa_bwd_dq_launch(const void* q, const void* k, const void* v,
                      const void* dout, const void* lse, const void* dvec,
                      void* dq, int B, int H, int HKV, int S, float scale,
                      const long long* strides, hipStream_t stream);
void fa_bwd_dq_v3_launch(const void* q, const void* k, const void* v,
                         const void* dout, const void* lse, const void* dvec,
                         void* dq, int B, int H, int HKV, int S, float scale,
                         const long long* strides, const int* doc_start,
                         hipStream_t stream);
// dk32 / dv32: zero-initialised contiguous fp32 [B,HKV,S,D] accumulators
void fa_bwd_dkv_launch(const void* q, const void* k, const void* v,
                       const void* dout, const void* lse, const void* dvec,
                       void* dk32, void* dv32, int B, int H, int HKV, int S,
                       float scale, const long long* strides,
                       hipStream_t stream);
void fa_bwd_dkv_v3_launch(const void* q, const void* k, const void* v,
                          const void* dout, const void* lse, const void* dvec,
                          void* dk32, void* dv32, int B, int H, int HKV, int S,
                          float scale, const long long* strides,
                          const int* doc_end, hipStream_t stream);
void f32_to_bf16_launch(const void* src, void* dst, long long n,
                        hipStream_t stream);

}  // extern "C"
