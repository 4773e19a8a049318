// Host launchers of the mixture-of-experts kernels (moe.hip). Included by the
// .hip file that defines them and by bindings.cpp, so a signature mismatch is
// a compile error. The stream type is forward-declared exactly as the HIP
// runtime does, which keeps this header free of HIP includes.
//
// T tokens, E experts (2..256), k experts per token (1..min(8, E)), H hidden
// (a multiple of 8), n_slots = T * k < 2^31. Slot s = t * k + j is token t's
// j-th choice. Activations are bf16 rows, 16-byte aligned; weights,
// probabilities and their gradients are fp32; every index array is int32.
// Nothing here allocates, copies, synchronises or uses an atomic on global
// memory: grids are a function of the shapes alone and the workspaces come
// from the caller, so every launch can be captured into a graph.
#pragma once

struct ihipStream_t;
typedef struct ihipStream_t* hipStream_t;

#define MOE_MAX_EXPERTS 256
#define MOE_MAX_TOPK 8

extern "C" {

// [E]-wide fp32 slices of `partials` that moe_router_fwd_launch needs
int moe_router_num_partials(long long T);

// logits [T, E] bf16 -> topk_idx [T, k], topk_w [T, k], probs_mean [E].
// The k largest logits win, equal logits go to the lower expert, slots come
// in descending logit order; topk_w is softmax(logits)[idx], divided by its
// sum over the k slots when norm_topk.
void moe_router_fwd_launch(const void* logits, int* topk_idx, float* topk_w,
                           float* probs_mean, float* partials, long long T,
                           int E, int k, int norm_topk, hipStream_t stream);

// dlogits [T, E] bf16 from d_topk_w [T, k] and d_probs_mean [E]
void moe_router_bwd_launch(const void* logits, const int* topk_idx,
                           const float* d_topk_w, const float* d_probs_mean,
                           void* dlogits, long long T, int E, int k,
                           int norm_topk, hipStream_t stream);

// blocks of the counting sort; `hist` holds E * blocks ints
int moe_sort_num_blocks(long long n_slots);

// Stable counting sort of the slots by expert. offs [E]: inclusive cumulative
// counts; row_of_slot / slot_of_row [n_slots]: the permutation and its
// inverse. An expert id outside [0, E) is counted as expert E - 1.
void moe_sort_launch(const int* topk_idx, int* hist, int* offs,
                     int* row_of_slot, int* slot_of_row, long long n_slots,
                     int E, hipStream_t stream);

// xp[r, :] = x[slot_of_row[r] / k, :]
void moe_dispatch_launch(const void* x, const int* slot_of_row, void* xp,
                         long long T, int k, int H, hipStream_t stream);

// y[t, :] = sum_j w[t, j] * yp[row_of_slot[t * k + j], :]; w == nullptr means
// unit weights (the backward of the dispatch)
void moe_combine_fwd_launch(const void* yp, const float* w,
                            const int* row_of_slot, void* y, long long T,
                            int k, int H, hipStream_t stream);

// dyp[row, :] = w[t, j] * dy[t, :] and dw[t, j] = <dy[t, :], yp[row, :]>
void moe_combine_bwd_launch(const void* dy, const void* yp, const float* w,
                            const int* row_of_slot, void* dyp, float* dw,
                            long long T, int k, int H, hipStream_t stream);

}  // extern "C"
