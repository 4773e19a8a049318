// Host launchers of the grouped GEMMs of the MoE experts (moe_gemm.hip).
// Included by the .hip file that defines them and by bindings.cpp, so a
// signature mismatch is a compile error.
//
// R rows in expert order, E experts (2..256), offs [E] int32 the inclusive
// cumulative row counts of moe_sort, w [E, K, N] bf16, K % 32 == 0 and
// N % 32 == 0, R < 2^31, every bf16 pointer 16-byte aligned. a(r) is row r of
// `a` [R, K], or with a gather (slot_of_row != nullptr) row
// slot_of_row[r] / k of `a` [T, K], T * k == R. The rules of moe_launch.h
// hold: nothing here allocates, copies, synchronises, reads on the host or
// uses an atomic on global memory, and grids are a function of the shapes
// alone, so every launch can be captured into a graph. R == 0 is the
// caller's case: the launchers need R >= 1.
#pragma once

struct ihipStream_t;
typedef struct ihipStream_t* hipStream_t;

#define MOE_GEMM_MAX_EXPERTS 256

extern "C" {

// y[r, :] = a(r) @ w[e(r)], y [R, N]
void moe_gemm_fwd_launch(const void* a, const void* w, const int* offs,
                         const int* slot_of_row, void* y, long long R,
                         long long T, int k, int E, int K, int N,
                         hipStream_t stream);

// da[r, :] = dy[r, :] @ w[e(r)]^T, da [R, K]; reads the same w
void moe_gemm_dgrad_launch(const void* dy, const void* w, const int* offs,
                           void* da, long long R, int E, int K, int N,
                           hipStream_t stream);

// dw[e] = sum over the rows r of e of a(r)^T dy[r, :], dw [E, K, N] bf16;
// every element is written, zeros for an expert without rows
void moe_gemm_wgrad_launch(const void* a, const void* dy, const int* offs,
                           const int* slot_of_row, void* dw, long long R,
                           long long T, int k, int E, int K, int N,
                           hipStream_t stream);

}  // extern "C"
