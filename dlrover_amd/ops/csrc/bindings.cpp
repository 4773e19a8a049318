// Python bindings for the dlrover_amd HIP kernels.
//
// Host-only translation layer: validates tensors, allocates outputs through
// the torch caching allocator, and forwards raw pointers + the current HIP
// stream to the extern "C" launchers in the .hip translation units.
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <tuple>
#include <vector>

#include "attention_launch.h"
#include "fp8_cast_launch.h"
#include "moe_gemm_launch.h"
#include "moe_launch.h"

extern "C" {
void rmsnorm_fwd_launch(const void*, const void*, void*, void*, int, int,
                        float, void*);
void rmsnorm_add_fwd_launch(const void*, const void*, const void*, void*,
                            void*, void*, int, int, float, void*);
void rmsnorm_bwd_launch(const void*, const void*, const void*, const void*,
                        const void*, void*, void*, void*, void*, int, int,
                        int, void*);
void rope_launch(void*, const void*, const void*, const void*, long long,
                 long long, int, int, int, void*);
void rope_oop_launch(const void*, void*, const void*, const void*,
                     const void*, long long, long long, int, int, long long,
                     int, void*);
int qk_norm_rope_bwd_slices(long long, int);
void qk_norm_rope_fwd_launch(const void*, const void*, long long, long long,
                             const void*, const void*, const void*,
                             const void*, const void*, void*, void*, void*,
                             int, int, int, int, int, float, void*);
void qk_norm_rope_bwd_launch(const void*, const void*, long long, long long,
                             const void*, const void*, long long, long long,
                             const void*, const void*, const void*,
                             const void*, const void*, const void*, void*,
                             void*, void*, void*, void*, int, int, int, int,
                             int, void*);
void swiglu_fwd_launch(const void*, void*, long long, int, void*);
void swiglu_bwd_launch(const void*, const void*, void*, long long, int, void*);
void adamw_launch(void*, const void*, void*, void*, void*, long long, float,
                  float, float, float, float, int, int, float, void*);
void causal_softmax_fwd_launch(void*, long long, int, int, int, float, void*);
void causal_softmax_bwd_launch(void*, const void*, long long, int, float,
                               void*);
void cross_entropy_launch(void*, const void*, void*, long long, int, int,
                          float, int, void*);
void ce_shard_stats_launch(const void*, const void*, void*, long long, int,
                           int, int, void*);
void ce_shard_finish_launch(void*, const void*, const void*, void*, long long,
                            int, int, int, int, float, int, void*);
void mfma16_probe_launch(const void*, const void*, void*, void*);
void mfma32_probe_launch(const void*, const void*, void*, void*);
void tr_b16_probe3_launch(void*, void*);
void tr_b16_probe_launch(void*, void*);
int mt_max_tensors();
long long mt_auto_span(long long);
long long mt_num_blocks(int, const long long*, long long);
void mt_sqnorm_launch(int, const void* const*, const long long*, const int*,
                      long long, float*, float*, void*);
void mt_adamw_launch(int, void* const*, const void* const*, void* const*,
                     void* const*, void* const*, const long long*,
                     const float*, const float*, const int*, int, float,
                     float, float, float, const float*, float, int, long long,
                     void*);
int f8_max_tensors();
int f8_block_elems();
long long f8_auto_span(long long);
void f8_quantize_launch(const float*, void*, float*, long long, void*);
void f8_dequantize_launch(const void*, const float*, float*, long long, void*);
void f8_adamw_launch(int, void* const*, const void* const*, void* const*,
                     void* const*, void* const*, void* const*, void* const*,
                     const long long*, const float*, const float*, const int*,
                     int, float, float, float, float, const float*, float,
                     int, long long, void*);
int sr_max_tensors();
void sr_round_launch(const float*, void*, long long, unsigned long long,
                     unsigned int, unsigned int, void*);
void sr_adamw_launch(int, void* const*, const void* const*, void* const*,
                     void* const*, const long long*, const float*,
                     const float*, const int*, const int*, int, float, float,
                     float, float, const float*, float, int,
                     unsigned long long, long long, void*);
void sr_f8_adamw_launch(int, void* const*, const void* const*, void* const*,
                        void* const*, void* const*, void* const*,
                        const long long*, const float*, const float*,
                        const int*, const int*, int, float, float, float,
                        float, const float*, float, int, unsigned long long,
                        long long, void*);
int ckpt_span_quantum();
int ckpt_max_blocks();
long long ckpt_auto_span(long long);
long long ckpt_num_slots(int, const long long*, long long);
void ckpt_copy_sum_launch(int, const void* const*, void* const*,
                          const long long*, long long, long long*, long long*,
                          void*);
}

namespace {

void* cur_stream() {
  return (void*)at::cuda::getCurrentCUDAStream().stream();
}

void check_bf16(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.scalar_type() == at::kBFloat16, name, " must be bf16");
}

std::tuple<at::Tensor, at::Tensor> rmsnorm_fwd(const at::Tensor& x,
                                               const at::Tensor& w,
                                               double eps) {
  check_bf16(x, "x");
  check_bf16(w, "w");
  const int hidden = (int)x.size(-1);
  TORCH_CHECK(hidden % 8 == 0, "hidden must be a multiple of 8");
  const long long n_rows = x.numel() / hidden;
  auto y = at::empty_like(x);
  auto invrms = at::empty({n_rows}, x.options().dtype(at::kFloat));
  rmsnorm_fwd_launch(x.data_ptr(), w.data_ptr(), y.data_ptr(),
                     invrms.data_ptr(), (int)n_rows, hidden, (float)eps,
                     cur_stream());
  return {y, invrms};
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> rmsnorm_add_fwd(
    const at::Tensor& x, const at::Tensor& resid, const at::Tensor& w,
    double eps) {
  check_bf16(x, "x");
  check_bf16(resid, "resid");
  const int hidden = (int)x.size(-1);
  const long long n_rows = x.numel() / hidden;
  auto h = at::empty_like(x);
  auto y = at::empty_like(x);
  auto invrms = at::empty({n_rows}, x.options().dtype(at::kFloat));
  rmsnorm_add_fwd_launch(x.data_ptr(), resid.data_ptr(), w.data_ptr(),
                         h.data_ptr(), y.data_ptr(), invrms.data_ptr(),
                         (int)n_rows, hidden, (float)eps, cur_stream());
  return {h, y, invrms};
}

std::tuple<at::Tensor, at::Tensor> rmsnorm_bwd(
    const at::Tensor& dy, const at::Tensor& x, const at::Tensor& w,
    const at::Tensor& invrms, c10::optional<at::Tensor> dh_extra) {
  check_bf16(dy, "dy");
  check_bf16(x, "x");
  const int hidden = (int)x.size(-1);
  TORCH_CHECK(hidden <= 16384, "rmsnorm_bwd: hidden > 16384 unsupported "
              "(register dw accumulator: RMSN_MAX_VPT)");
  const long long n_rows = x.numel() / hidden;
  // one private slice per block (plain stores, no atomics): n_partials must
  // match the kernel grid = min(n_rows, 2048)
  const int n_partials = (int)(n_rows < 2048 ? (n_rows > 0 ? n_rows : 1) : 2048);
  auto dx = at::empty_like(x);
  auto dw = at::empty_like(w);
  auto partial =
      at::empty({n_partials, hidden}, x.options().dtype(at::kFloat));
  auto dw_f32 = at::zeros({hidden}, x.options().dtype(at::kFloat));
  const void* dh_ptr = nullptr;
  if (dh_extra.has_value()) {
    check_bf16(*dh_extra, "dh_extra");
    dh_ptr = dh_extra->data_ptr();
  }
  rmsnorm_bwd_launch(dy.data_ptr(), x.data_ptr(), w.data_ptr(),
                     invrms.data_ptr(), dh_ptr, dx.data_ptr(),
                     partial.data_ptr(), dw_f32.data_ptr(), dw.data_ptr(),
                     (int)n_rows, hidden, n_partials, cur_stream());
  return {dx, dw};
}

void rope_apply(at::Tensor& x, const at::Tensor& pos, const at::Tensor& cos,
                const at::Tensor& sin, bool backward) {
  check_bf16(x, "x");
  TORCH_CHECK(pos.scalar_type() == at::kInt && pos.is_cuda(),
              "pos must be int32 on GPU");
  TORCH_CHECK(cos.scalar_type() == at::kFloat && cos.is_contiguous(),
              "cos table must be contiguous fp32");
  const int head_dim = (int)x.size(-1);
  const int n_heads = (int)x.size(-2);
  TORCH_CHECK(head_dim % 8 == 0, "head_dim must be a multiple of 8");
  const long long n_tokens = x.numel() / ((long long)n_heads * head_dim);
  TORCH_CHECK(pos.numel() > 0 && n_tokens % pos.numel() == 0,
              "pos length must divide the token count (one entry per "
              "sequence position)");
  rope_launch(x.data_ptr(), pos.data_ptr(), cos.data_ptr(), sin.data_ptr(),
              n_tokens, (long long)pos.numel(), n_heads, head_dim,
              backward ? 1 : 0, cur_stream());
}

at::Tensor rope_rotate_oop(const at::Tensor& x, const at::Tensor& pos,
                           const at::Tensor& cos, const at::Tensor& sin,
                           bool backward) {
  // x: [..., n_tokens?, n_heads, head_dim] with heads*head_dim contiguous
  // per token row; the token stride may exceed n_heads*head_dim (a view out
  // of the fused QKV projection). Returns a fresh CONTIGUOUS tensor.
  TORCH_CHECK(x.is_cuda(), "x must be on GPU");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, "x must be bf16");
  TORCH_CHECK(pos.scalar_type() == at::kInt && pos.is_cuda(),
              "pos must be int32 on GPU");
  const int head_dim = (int)x.size(-1);
  const int n_heads = (int)x.size(-2);
  TORCH_CHECK(head_dim % 8 == 0, "head_dim must be a multiple of 8");
  TORCH_CHECK(x.stride(-1) == 1 && x.stride(-2) == head_dim,
              "rope: head_dim/heads must be contiguous within a token row");
  const long long n_tokens = x.numel() / ((long long)n_heads * head_dim);
  // flatten every leading dim into tokens: requires uniform token stride
  long long tok_stride = n_heads * (long long)head_dim;
  if (x.dim() >= 3) {
    tok_stride = x.stride(-3);
    long long rows = x.size(-3);
    for (int d = (int)x.dim() - 4; d >= 0; --d) {
      TORCH_CHECK(x.stride(d) == rows * tok_stride,
                  "rope: leading dims must be uniformly strided");
      rows *= x.size(d);
    }
  }
  TORCH_CHECK(pos.numel() > 0 && n_tokens % pos.numel() == 0,
              "pos length must divide the token count");
  auto out = at::empty(x.sizes(), x.options());
  rope_oop_launch(x.data_ptr(), out.data_ptr(), pos.data_ptr(),
                  cos.data_ptr(), sin.data_ptr(), n_tokens,
                  (long long)pos.numel(), n_heads, head_dim, tok_stride,
                  backward ? 1 : 0, cur_stream());
  return out;
}

// Token stride of a [..., tokens, heads, D] bf16 view that the QK-norm
// kernels can address in place: heads*D contiguous inside a token and every
// leading dim uniformly strided (rope_rotate_oop's rule).
long long qknr_tok_stride(const at::Tensor& x, const char* name) {
  TORCH_CHECK(x.is_cuda(), "qk_norm_rope: ", name, " must be on GPU");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, "qk_norm_rope: ", name,
              " must be bf16");
  TORCH_CHECK(x.dim() >= 3, "qk_norm_rope: ", name,
              " must be [..., tokens, heads, head_dim]");
  // the stride of a size-1 dim is never used and may hold anything
  TORCH_CHECK(x.stride(-1) == 1 &&
                  (x.size(-2) == 1 || x.stride(-2) == x.size(-1)),
              "qk_norm_rope: ", name,
              " needs head_dim/heads contiguous within a token row");
  const long long tok_stride = x.stride(-3);
  long long rows = x.size(-3);
  for (int d = (int)x.dim() - 4; d >= 0; --d) {
    TORCH_CHECK(x.size(d) == 1 || x.stride(d) == rows * tok_stride,
                "qk_norm_rope: ", name,
                " leading dims must be uniformly strided");
    rows *= x.size(d);
  }
  TORCH_CHECK(tok_stride % 8 == 0 &&
                  reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0,
              "qk_norm_rope: ", name, " must be 16-byte aligned per token");
  return tok_stride;
}

// Checks shared by forward and backward; returns the token count.
long long qknr_check(const at::Tensor& q, const at::Tensor& k,
                     const at::Tensor& wq, const at::Tensor& wk,
                     const at::Tensor& pos, const at::Tensor& cos,
                     const at::Tensor& sin) {
  const long long hd = q.size(-1);
  TORCH_CHECK(hd == 64 || hd == 128,
              "qk_norm_rope: head_dim must be 64 or 128, got ", hd);
  TORCH_CHECK(k.size(-1) == hd && q.dim() == k.dim(),
              "qk_norm_rope: q and k must share head_dim and rank");
  const long long n_tokens = q.numel() / (q.size(-2) * hd);
  TORCH_CHECK(k.numel() / (k.size(-2) * hd) == n_tokens,
              "qk_norm_rope: q and k must have the same token count");
  TORCH_CHECK(n_tokens * (q.size(-2) + k.size(-2)) < (1LL << 31),
              "qk_norm_rope: more than 2^31 head rows");
  check_bf16(wq, "wq");
  check_bf16(wk, "wk");
  TORCH_CHECK(wq.numel() == hd && wk.numel() == hd,
              "qk_norm_rope: wq and wk must have head_dim elements");
  TORCH_CHECK(pos.scalar_type() == at::kInt && pos.is_cuda() &&
                  pos.is_contiguous(),
              "qk_norm_rope: pos must be contiguous int32 on GPU");
  TORCH_CHECK(pos.numel() > 0 && n_tokens % pos.numel() == 0,
              "qk_norm_rope: pos length must equal or divide the token "
              "count");
  for (const at::Tensor* tab : {&cos, &sin})
    TORCH_CHECK(tab->is_cuda() && tab->scalar_type() == at::kFloat &&
                    tab->is_contiguous() && tab->dim() == 2 &&
                    tab->size(1) == hd / 2,
                "qk_norm_rope: cos/sin must be contiguous fp32 "
                "[max_pos, head_dim/2] on GPU");
  TORCH_CHECK(cos.size(0) == sin.size(0),
              "qk_norm_rope: cos and sin must have the same length");
  return n_tokens;
}

// q [..., T, nh, D], k [..., T, nkv, D] (strided views are read in place)
// -> contiguous q_out, k_out and inv [T_total, nh+nkv] fp32 for backward.
std::tuple<at::Tensor, at::Tensor, at::Tensor> qk_norm_rope_fwd(
    const at::Tensor& q, const at::Tensor& k, const at::Tensor& wq,
    const at::Tensor& wk, const at::Tensor& pos, const at::Tensor& cos,
    const at::Tensor& sin, double eps) {
  const long long q_stride = qknr_tok_stride(q, "q");
  const long long k_stride = qknr_tok_stride(k, "k");
  const long long n_tokens = qknr_check(q, k, wq, wk, pos, cos, sin);
  const int nh = (int)q.size(-2), nkv = (int)k.size(-2);
  auto q_out = at::empty(q.sizes(), q.options());
  auto k_out = at::empty(k.sizes(), k.options());
  auto inv = at::empty({n_tokens, nh + nkv}, q.options().dtype(at::kFloat));
  if (n_tokens > 0)
    qk_norm_rope_fwd_launch(
        q.data_ptr(), k.data_ptr(), q_stride, k_stride, wq.data_ptr(),
        wk.data_ptr(), pos.data_ptr(), cos.data_ptr(), sin.data_ptr(),
        q_out.data_ptr(), k_out.data_ptr(), inv.data_ptr(), (int)n_tokens,
        (int)pos.numel(), nh, nkv, (int)q.size(-1), (float)eps, cur_stream());
  return {q_out, k_out, inv};
}

// -> contiguous dx_q, dx_k and bf16 dwq, dwk
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> qk_norm_rope_bwd(
    const at::Tensor& dyq, const at::Tensor& dyk, const at::Tensor& q,
    const at::Tensor& k, const at::Tensor& inv, const at::Tensor& wq,
    const at::Tensor& wk, const at::Tensor& pos, const at::Tensor& cos,
    const at::Tensor& sin) {
  const long long dyq_stride = qknr_tok_stride(dyq, "dy_q");
  const long long dyk_stride = qknr_tok_stride(dyk, "dy_k");
  const long long q_stride = qknr_tok_stride(q, "q");
  const long long k_stride = qknr_tok_stride(k, "k");
  const long long n_tokens = qknr_check(q, k, wq, wk, pos, cos, sin);
  TORCH_CHECK(dyq.sizes() == q.sizes() && dyk.sizes() == k.sizes(),
              "qk_norm_rope_bwd: dy shapes must match q and k");
  const int nh = (int)q.size(-2), nkv = (int)k.size(-2);
  const int hd = (int)q.size(-1);
  TORCH_CHECK(inv.is_cuda() && inv.scalar_type() == at::kFloat &&
                  inv.is_contiguous() &&
                  inv.numel() == n_tokens * (nh + nkv),
              "qk_norm_rope_bwd: inv must be contiguous fp32 "
              "[tokens, nh+nkv]");
  auto dxq = at::empty(q.sizes(), q.options());
  auto dxk = at::empty(k.sizes(), k.options());
  auto dwq = at::empty_like(wq);
  auto dwk = at::empty_like(wk);
  if (n_tokens == 0) return {dxq, dxk, dwq.zero_(), dwk.zero_()};
  const int n_slices =
      qk_norm_rope_bwd_slices(n_tokens * (long long)(nh + nkv), hd);
  auto partial =
      at::empty({n_slices, 2, hd}, q.options().dtype(at::kFloat));
  qk_norm_rope_bwd_launch(
      dyq.data_ptr(), dyk.data_ptr(), dyq_stride, dyk_stride, q.data_ptr(),
      k.data_ptr(), q_stride, k_stride, inv.data_ptr(), wq.data_ptr(),
      wk.data_ptr(), pos.data_ptr(), cos.data_ptr(), sin.data_ptr(),
      dxq.data_ptr(), dxk.data_ptr(), partial.data_ptr(), dwq.data_ptr(),
      dwk.data_ptr(), (int)n_tokens, (int)pos.numel(), nh, nkv, hd,
      cur_stream());
  return {dxq, dxk, dwq, dwk};
}

at::Tensor swiglu_fwd(const at::Tensor& gate_up) {
  check_bf16(gate_up, "gate_up");
  const int two_inner = (int)gate_up.size(-1);
  TORCH_CHECK(two_inner % 16 == 0, "inner dim must be a multiple of 8");
  const int inner = two_inner / 2;
  const long long n_rows = gate_up.numel() / two_inner;
  auto sizes = gate_up.sizes().vec();
  sizes.back() = inner;
  auto out = at::empty(sizes, gate_up.options());
  swiglu_fwd_launch(gate_up.data_ptr(), out.data_ptr(), n_rows, inner,
                    cur_stream());
  return out;
}

at::Tensor swiglu_bwd(const at::Tensor& dy, const at::Tensor& gate_up) {
  check_bf16(dy, "dy");
  check_bf16(gate_up, "gate_up");
  const int inner = (int)gate_up.size(-1) / 2;
  const long long n_rows = gate_up.numel() / (2LL * inner);
  auto d_gate_up = at::empty_like(gate_up);
  swiglu_bwd_launch(dy.data_ptr(), gate_up.data_ptr(), d_gate_up.data_ptr(),
                    n_rows, inner, cur_stream());
  return d_gate_up;
}

void adamw_step(at::Tensor& param, const at::Tensor& grad, at::Tensor& m,
                at::Tensor& v, c10::optional<at::Tensor> param_bf16,
                double lr, double beta1, double beta2, double eps,
                double weight_decay, int64_t step, double grad_scale) {
  TORCH_CHECK(param.scalar_type() == at::kFloat && param.is_contiguous(),
              "master param must be contiguous fp32");
  TORCH_CHECK(grad.is_cuda() && grad.is_contiguous(), "grad must be GPU");
  TORCH_CHECK(grad.numel() == param.numel(), "grad/param numel mismatch");
  const bool gbf16 = grad.scalar_type() == at::kBFloat16;
  TORCH_CHECK(gbf16 || grad.scalar_type() == at::kFloat,
              "grad must be bf16 or fp32");
  void* pb = nullptr;
  if (param_bf16.has_value()) {
    check_bf16(*param_bf16, "param_bf16");
    pb = param_bf16->data_ptr();
  }
  adamw_launch(param.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(),
               pb, param.numel(), (float)lr, (float)beta1, (float)beta2,
               (float)eps, (float)weight_decay, (int)step, gbf16 ? 1 : 0,
               (float)grad_scale, cur_stream());
}

void causal_softmax_fwd(at::Tensor& scores, int64_t q_len, int64_t q_offset,
                        double scale) {
  check_bf16(scores, "scores");
  const int row_len = (int)scores.size(-1);
  TORCH_CHECK(row_len % 8 == 0, "row_len must be a multiple of 8");
  const long long n_rows = scores.numel() / row_len;
  causal_softmax_fwd_launch(scores.data_ptr(), n_rows, row_len, (int)q_len,
                            (int)q_offset, (float)scale, cur_stream());
}

void causal_softmax_bwd(at::Tensor& dscores, const at::Tensor& probs,
                        double scale) {
  check_bf16(dscores, "dscores");
  check_bf16(probs, "probs");
  const int row_len = (int)dscores.size(-1);
  const long long n_rows = dscores.numel() / row_len;
  causal_softmax_bwd_launch(dscores.data_ptr(), probs.data_ptr(), n_rows,
                            row_len, (float)scale, cur_stream());
}

// ---- flash attention ------------------------------------------------------
// q/k/v/out are LOGICALLY [B,H,S,D]; strided permuted views are fine as long
// as the last (D) dim is contiguous — no transpose copies needed.
void check_attn_view(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kBFloat16, name,
              " must be bf16 GPU");
  TORCH_CHECK(t.dim() == 4 && t.stride(3) == 1, name,
              " must be [B,H,S,D] with contiguous D");
}

void pack_strides(long long* st, const at::Tensor& t, int at) {
  st[at + 0] = (long long)t.stride(0);
  st[at + 1] = (long long)t.stride(1);
  st[at + 2] = (long long)t.stride(2);
}

hipStream_t attn_stream() {
  return at::cuda::getCurrentCUDAStream().stream();
}

struct AttnShape {
  int B, H, HKV, S, D;
};

// everything the kernels assume about q/k/v, forward and backward alike
AttnShape check_attn_qkv(const at::Tensor& q, const at::Tensor& k,
                         const at::Tensor& v) {
  check_attn_view(q, "q");
  check_attn_view(k, "k");
  check_attn_view(v, "v");
  TORCH_CHECK(k.device() == q.device() && v.device() == q.device(),
              "flash_attn: q, k and v must be on one device");
  TORCH_CHECK(k.sizes() == v.sizes(),
              "flash_attn: k and v must have the same shape");
  TORCH_CHECK(k.size(0) == q.size(0) && k.size(2) == q.size(2) &&
                  k.size(3) == q.size(3),
              "flash_attn: k/v must have q's B, S and D");
  const AttnShape s = {(int)q.size(0), (int)q.size(1), (int)k.size(1),
                       (int)q.size(2), (int)q.size(3)};
  TORCH_CHECK(s.D == 128, "flash_attn: head_dim must be 128");
  TORCH_CHECK(s.S % 64 == 0, "flash_attn: seq len must be a multiple of 64");
  TORCH_CHECK(s.HKV > 0 && s.H % s.HKV == 0, "flash_attn: H % HKV != 0");
  return s;
}

// The 32x32-MFMA kernels (attention_v3.hip, attention_bwd_v3.hip) own 256-row
// blocks; every other S (a multiple of 64) runs the 16x16 kernels. Forward
// and backward use the same rule.
bool attn_use_v3(int S) { return S % 256 == 0; }

// document-mask arguments: int32 [B, S], contiguous, on q's device; only the
// v3 kernels have the DOC variant
void check_doc_arg(const at::Tensor& d, const at::Tensor& q,
                   const char* name) {
  TORCH_CHECK(d.scalar_type() == at::kInt, name, " must be int32");
  TORCH_CHECK(d.device() == q.device(), name, " must be on q's device");
  TORCH_CHECK(d.dim() == 2 && d.size(0) == q.size(0) &&
                  d.size(1) == q.size(2) && d.is_contiguous(),
              name, " must be contiguous [B, S]");
  TORCH_CHECK(attn_use_v3((int)q.size(2)),
              "flash_attn_doc: seq len must be a multiple of 256");
}

const int* doc_ptr(const at::Tensor* d) {
  return d != nullptr ? (const int*)d->data_ptr() : nullptr;
}

// doc_start null: the causal path
std::tuple<at::Tensor, at::Tensor> flash_attn_fwd_impl(
    const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
    double scale, const at::Tensor* doc_start) {
  const AttnShape s = check_attn_qkv(q, k, v);
  if (doc_start != nullptr) check_doc_arg(*doc_start, q, "doc_start");
  // output in [B,S,H,D] storage (what the model consumes — avoids the
  // transpose-back copy); returned as a [B,H,S,D] view
  auto out_bshd = at::empty({s.B, s.S, s.H, s.D}, q.options());
  auto out = out_bshd.permute({0, 2, 1, 3});
  auto lse = at::empty({s.B, s.H, s.S}, q.options().dtype(at::kFloat));
  long long st[12];
  pack_strides(st, q, 0);
  pack_strides(st, k, 3);
  pack_strides(st, v, 6);
  pack_strides(st, out, 9);
  if (attn_use_v3(s.S)) {
    flash_attn_fwd_v3_launch(q.data_ptr(), k.data_ptr(), v.data_ptr(),
                             out_bshd.data_ptr(), lse.data_ptr(), s.B, s.H,
                             s.HKV, s.S, (float)scale, st, doc_ptr(doc_start),
                             attn_stream());
  } else {
    flash_attn_fwd_launch(q.data_ptr(), k.data_ptr(), v.data_ptr(),
                          out_bshd.data_ptr(), lse.data_ptr(), s.B, s.H,
                          s.HKV, s.S, (float)scale, st, attn_stream());
  }
  return {out, lse};
}

std::tuple<at::Tensor, at::Tensor> flash_attn_fwd(const at::Tensor& q,
                                                  const at::Tensor& k,
                                                  const at::Tensor& v,
                                                  double scale) {
  return flash_attn_fwd_impl(q, k, v, scale, nullptr);
}

std::tuple<at::Tensor, at::Tensor> flash_attn_doc_fwd(
    const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
    double scale, const at::Tensor& doc_start) {
  return flash_attn_fwd_impl(q, k, v, scale, &doc_start);
}

// out / dout: bf16 on q's device with q's logical shape
void check_attn_like_q(const at::Tensor& t, const at::Tensor& q,
                       const char* name) {
  TORCH_CHECK(t.is_cuda() && t.device() == q.device() &&
                  t.scalar_type() == at::kBFloat16,
              name, " must be bf16 on q's device");
  TORCH_CHECK(t.sizes() == q.sizes(), name, " must have q's shape");
}

// doc_start / doc_end both null: the causal path
std::tuple<at::Tensor, at::Tensor, at::Tensor> flash_attn_bwd_impl(
    const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
    const at::Tensor& out, const at::Tensor& dout_in, const at::Tensor& lse,
    double scale, const at::Tensor* doc_start, const at::Tensor* doc_end) {
  const AttnShape s = check_attn_qkv(q, k, v);
  check_attn_like_q(out, q, "out");
  TORCH_CHECK(out.stride(3) == 1, "out needs contiguous D");
  check_attn_like_q(dout_in, q, "dout");
  TORCH_CHECK(lse.is_cuda() && lse.device() == q.device() &&
                  lse.scalar_type() == at::kFloat,
              "lse must be fp32 on q's device");
  TORCH_CHECK(lse.is_contiguous() &&
                  lse.sizes() == at::IntArrayRef({s.B, s.H, s.S}),
              "lse must be contiguous [B, H, S]");
  if (doc_start != nullptr) {
    check_doc_arg(*doc_start, q, "doc_start");
    check_doc_arg(*doc_end, q, "doc_end");
  }
  // the preprocess + dkv stage read dO/O with [B,S,H,D]-style strides; accept
  // any incoming grad layout by normalizing dO into out's layout
  at::Tensor dout = dout_in;
  if (dout.strides() != out.strides()) {
    dout = at::empty({s.B, s.S, s.H, s.D}, out.options())
               .permute({0, 2, 1, 3});
    dout.copy_(dout_in);
  }
  TORCH_CHECK(dout.stride(3) == 1, "dout needs contiguous D");
  auto dvec = at::empty({s.B, s.H, s.S}, q.options().dtype(at::kFloat));
  long long ost[3], dstr[3];
  pack_strides(ost, out, 0);
  pack_strides(dstr, dout, 0);
  fa_bwd_pre_launch(dout.data_ptr(), out.data_ptr(), dvec.data_ptr(), s.B,
                    s.H, s.S, ost, dstr, attn_stream());
  // dq mirrors q's layout: allocate [B,S,H,D] storage, return as view
  auto dq_bshd = at::empty({s.B, s.S, s.H, s.D}, q.options());
  auto dq = dq_bshd.permute({0, 2, 1, 3});
  // the kernels use ONE strides triple for both q loads and dq stores, so
  // stage q into dq's layout if they differ
  at::Tensor quse = q;
  if (q.strides() != dq.strides()) {
    quse = at::empty({s.B, s.S, s.H, s.D}, q.options()).permute({0, 2, 1, 3});
    quse.copy_(q);
  }
  long long st[12];
  pack_strides(st, quse, 0);
  pack_strides(st, k, 3);
  pack_strides(st, v, 6);
  pack_strides(st, dout, 9);
  auto dk32 =
      at::zeros({s.B, s.HKV, s.S, s.D}, k.options().dtype(at::kFloat));
  auto dv32 =
      at::zeros({s.B, s.HKV, s.S, s.D}, v.options().dtype(at::kFloat));
  if (attn_use_v3(s.S)) {
    fa_bwd_dq_v3_launch(quse.data_ptr(), k.data_ptr(), v.data_ptr(),
                        dout.data_ptr(), lse.data_ptr(), dvec.data_ptr(),
                        dq_bshd.data_ptr(), s.B, s.H, s.HKV, s.S,
                        (float)scale, st, doc_ptr(doc_start), attn_stream());
    fa_bwd_dkv_v3_launch(quse.data_ptr(), k.data_ptr(), v.data_ptr(),
                         dout.data_ptr(), lse.data_ptr(), dvec.data_ptr(),
                         dk32.data_ptr(), dv32.data_ptr(), s.B, s.H, s.HKV,
                         s.S, (float)scale, st, doc_ptr(doc_end),
                         attn_stream());
  } else {
    fa_bwd_dq_launch(quse.data_ptr(), k.data_ptr(), v.data_ptr(),
                     dout.data_ptr(), lse.data_ptr(), dvec.data_ptr(),
                     dq_bshd.data_ptr(), s.B, s.H, s.HKV, s.S, (float)scale,
                     st, attn_stream());
    fa_bwd_dkv_launch(quse.data_ptr(), k.data_ptr(), v.data_ptr(),
                      dout.data_ptr(), lse.data_ptr(), dvec.data_ptr(),
                      dk32.data_ptr(), dv32.data_ptr(), s.B, s.H, s.HKV, s.S,
                      (float)scale, st, attn_stream());
  }
  auto dk = at::empty({s.B, s.HKV, s.S, s.D}, k.options());
  auto dv = at::empty({s.B, s.HKV, s.S, s.D}, v.options());
  f32_to_bf16_launch(dk32.data_ptr(), dk.data_ptr(), dk32.numel(),
                     attn_stream());
  f32_to_bf16_launch(dv32.data_ptr(), dv.data_ptr(), dv32.numel(),
                     attn_stream());
  return {dq, dk, dv};
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> flash_attn_bwd(
    const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
    const at::Tensor& out, const at::Tensor& dout, const at::Tensor& lse,
    double scale) {
  return flash_attn_bwd_impl(q, k, v, out, dout, lse, scale, nullptr,
                             nullptr);
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> flash_attn_doc_bwd(
    const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
    const at::Tensor& out, const at::Tensor& dout, const at::Tensor& lse,
    double scale, const at::Tensor& doc_start, const at::Tensor& doc_end) {
  return flash_attn_bwd_impl(q, k, v, out, dout, lse, scale, &doc_start,
                             &doc_end);
}

at::Tensor mfma16_probe(const at::Tensor& A, const at::Tensor& B) {
  check_bf16(A, "A");
  check_bf16(B, "B");
  TORCH_CHECK(A.sizes() == at::IntArrayRef({16, 32}) &&
              B.sizes() == at::IntArrayRef({32, 16}),
              "probe wants A[16,32], B[32,16]");
  auto C = at::empty({16, 16}, A.options().dtype(at::kFloat));
  mfma16_probe_launch(A.data_ptr(), B.data_ptr(), C.data_ptr(), cur_stream());
  return C;
}

// Direct async copies between device tensors and FOREIGN host memory
// (hipHostRegister'ed shm mappings). torch's copy_ cannot be trusted here:
// it may not recognize the registered pointer as pinned and fall back to a
// synchronous null-stream hipMemcpy, which serializes with ALL compute on
// the default stream (measured: each 104-GB ckpt drain added its full ~2 s
// to the training wall instead of overlapping). These run on the CURRENT
// torch stream — call inside `with torch.cuda.stream(side)`.
void memcpy_d2h_async(int64_t dst_addr, const at::Tensor& src) {
  TORCH_CHECK(src.is_cuda() && src.is_contiguous(), "src must be cuda+contig");
  auto err = hipMemcpyAsync((void*)dst_addr, src.data_ptr(), src.nbytes(),
                            hipMemcpyDeviceToHost,
                            (hipStream_t)cur_stream());
  TORCH_CHECK(err == hipSuccess, "hipMemcpyAsync D2H: ", hipGetErrorString(err));
}

void memcpy_h2d_async(at::Tensor& dst, int64_t src_addr, int64_t nbytes) {
  TORCH_CHECK(dst.is_cuda() && dst.is_contiguous(), "dst must be cuda+contig");
  TORCH_CHECK(nbytes <= (int64_t)dst.nbytes(), "overflow");
  auto err = hipMemcpyAsync(dst.data_ptr(), (const void*)src_addr, nbytes,
                            hipMemcpyHostToDevice,
                            (hipStream_t)cur_stream());
  TORCH_CHECK(err == hipSuccess, "hipMemcpyAsync H2D: ", hipGetErrorString(err));
}

at::Tensor mfma32_probe(const at::Tensor& A, const at::Tensor& B) {
  check_bf16(A, "A");
  check_bf16(B, "B");
  TORCH_CHECK(A.sizes() == at::IntArrayRef({32, 16}) &&
              B.sizes() == at::IntArrayRef({16, 32}),
              "probe wants A[32,16], B[16,32]");
  auto C = at::empty({32, 32}, A.options().dtype(at::kFloat));
  mfma32_probe_launch(A.data_ptr(), B.data_ptr(), C.data_ptr(), cur_stream());
  return C;
}

at::Tensor cross_entropy_fwd_bwd(at::Tensor& logits, const at::Tensor& targets,
                                 int64_t ignore_index, double grad_scale,
                                 bool compute_grad) {
  check_bf16(logits, "logits");
  TORCH_CHECK(targets.scalar_type() == at::kInt && targets.is_cuda(),
              "targets must be int32 on GPU");
  const int vocab = (int)logits.size(-1);
  const long long n_rows = logits.numel() / vocab;
  TORCH_CHECK(targets.numel() == n_rows, "one target per row");
  auto losses = at::empty({n_rows}, logits.options().dtype(at::kFloat));
  cross_entropy_launch(logits.data_ptr(), targets.data_ptr(),
                       losses.data_ptr(), n_rows, vocab, (int)ignore_index,
                       (float)grad_scale, compute_grad ? 1 : 0, cur_stream());
  return losses;
}

// ---- vocab-parallel cross-entropy (vocab_parallel_ce.hip) ----------------
// Validates one [N, Vs] logits shard and its N global-id targets; returns N.
long long check_ce_shard(const at::Tensor& logits_shard,
                         const at::Tensor& targets, int64_t vocab_start) {
  check_bf16(logits_shard, "logits_shard");
  TORCH_CHECK(logits_shard.dim() >= 1, "logits_shard must be [N, Vs]");
  const int64_t vs = logits_shard.size(-1);
  TORCH_CHECK(vs > 0 && vs % 8 == 0 && vs < (1LL << 31),
              "shard width Vs must be a positive multiple of 8, got ", vs);
  TORCH_CHECK(vocab_start >= 0 && vocab_start + vs < (1LL << 31),
              "vocab_start out of int32 range");
  TORCH_CHECK(targets.scalar_type() == at::kInt && targets.is_cuda() &&
                  targets.is_contiguous(),
              "targets must be contiguous int32 on GPU");
  const long long n_rows = logits_shard.numel() / vs;
  TORCH_CHECK(targets.numel() == n_rows, "one target per row");
  return n_rows;
}

at::Tensor ce_shard_stats(const at::Tensor& logits_shard,
                          const at::Tensor& targets, int64_t vocab_start,
                          int64_t ignore_index) {
  const long long n_rows = check_ce_shard(logits_shard, targets, vocab_start);
  auto stats =
      at::empty({n_rows, 3}, logits_shard.options().dtype(at::kFloat));
  ce_shard_stats_launch(logits_shard.data_ptr(), targets.data_ptr(),
                        stats.data_ptr(), n_rows, (int)logits_shard.size(-1),
                        (int)vocab_start, (int)ignore_index, cur_stream());
  return stats;
}

at::Tensor ce_shard_finish(at::Tensor& logits_shard, const at::Tensor& targets,
                           int64_t vocab_start, const at::Tensor& stats_all,
                           double grad_scale, int64_t ignore_index,
                           bool compute_grad) {
  const long long n_rows = check_ce_shard(logits_shard, targets, vocab_start);
  TORCH_CHECK(stats_all.is_cuda() && stats_all.is_contiguous() &&
                  stats_all.scalar_type() == at::kFloat,
              "stats_all must be contiguous fp32 on GPU");
  TORCH_CHECK(stats_all.dim() == 3 && stats_all.size(0) >= 1 &&
                  stats_all.size(0) < (1LL << 31),
              "stats_all must be [tp, N, 3]");
  const long long tp = stats_all.size(0);
  TORCH_CHECK(stats_all.numel() == tp * n_rows * 3,
              "stats_all must hold tp*N*3 = ", tp * n_rows * 3,
              " elements, got ", stats_all.numel());
  auto losses = at::empty({n_rows}, logits_shard.options().dtype(at::kFloat));
  ce_shard_finish_launch(logits_shard.data_ptr(), targets.data_ptr(),
                         stats_all.data_ptr(), losses.data_ptr(), n_rows,
                         (int)logits_shard.size(-1), (int)vocab_start, (int)tp,
                         (int)ignore_index, (float)grad_scale,
                         compute_grad ? 1 : 0, cur_stream());
  return losses;
}

// ---- multi-tensor ops (multi_tensor.hip) ---------------------------------
// span_elems == 0 picks the span from the list's total size; any other value
// must be a multiple of 8 and is used as given.
long long mt_span(const std::vector<long long>& numel, int64_t span_elems) {
  TORCH_CHECK(span_elems >= 0 && span_elems % 8 == 0,
              "span_elems must be 0 (automatic) or a positive multiple of 8");
  if (span_elems > 0) return span_elems;
  long long total = 0;
  for (long long n : numel) total += n;
  return mt_auto_span(total);
}

std::vector<long long> mt_numels(const std::vector<at::Tensor>& ts) {
  std::vector<long long> numel;
  numel.reserve(ts.size());
  for (const auto& t : ts) numel.push_back((long long)t.numel());
  return numel;
}

int64_t multi_tensor_num_partials(const std::vector<at::Tensor>& tensors,
                                  int64_t span_elems) {
  const auto numel = mt_numels(tensors);
  return mt_num_blocks((int)numel.size(), numel.data(),
                       mt_span(numel, span_elems));
}

void multi_tensor_sq_norm(const std::vector<at::Tensor>& tensors,
                          at::Tensor& partials, at::Tensor& out,
                          int64_t span_elems) {
  const auto numel = mt_numels(tensors);
  const long long span = mt_span(numel, span_elems);
  const int n = (int)tensors.size();
  std::vector<const void*> ptrs(n);
  std::vector<int> is_bf16(n);
  for (int i = 0; i < n; ++i) {
    const auto& t = tensors[i];
    TORCH_CHECK(t.is_cuda(), "sq_norm: tensors must be on GPU");
    TORCH_CHECK(t.numel() == 0 || t.is_contiguous(),
                "sq_norm: tensors must be contiguous");
    is_bf16[i] = t.scalar_type() == at::kBFloat16;
    TORCH_CHECK(is_bf16[i] || t.scalar_type() == at::kFloat,
                "sq_norm: tensors must be bf16 or fp32");
    ptrs[i] = t.numel() ? t.data_ptr() : nullptr;
  }
  const long long need = mt_num_blocks(n, numel.data(), span);
  TORCH_CHECK(need < (1LL << 31), "sq_norm: too many spans");
  TORCH_CHECK(partials.is_cuda() && partials.is_contiguous() &&
                  partials.scalar_type() == at::kFloat &&
                  partials.numel() >= need,
              "sq_norm: partials must be contiguous fp32 on GPU with at "
              "least ", need, " elements");
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == at::kFloat &&
                  out.numel() >= 1,
              "sq_norm: out must be fp32 on GPU");
  mt_sqnorm_launch(n, ptrs.data(), numel.data(), is_bf16.data(), span,
                   (float*)partials.data_ptr(), (float*)out.data_ptr(),
                   cur_stream());
}

void multi_tensor_adamw(
    const std::vector<at::Tensor>& masters,
    const std::vector<at::Tensor>& grads,
    const std::vector<at::Tensor>& exp_avgs,
    const std::vector<at::Tensor>& exp_avg_sqs,
    c10::optional<std::vector<c10::optional<at::Tensor>>> params_bf16,
    const std::vector<double>& lrs, const std::vector<double>& weight_decays,
    const std::vector<int64_t>& steps, double beta1, double beta2, double eps,
    double grad_scale, c10::optional<at::Tensor> norm_sq, double max_norm,
    bool skip_nonfinite, int64_t span_elems) {
  const size_t n = masters.size();
  TORCH_CHECK(grads.size() == n && exp_avgs.size() == n &&
                  exp_avg_sqs.size() == n && lrs.size() == n &&
                  weight_decays.size() == n && steps.size() == n &&
                  (!params_bf16.has_value() || params_bf16->size() == n),
              "multi_tensor_adamw: list lengths differ");
  if (n == 0) return;
  const auto numel = mt_numels(masters);
  const long long span = mt_span(numel, span_elems);
  const bool gbf16 = grads[0].scalar_type() == at::kBFloat16;
  std::vector<void*> pm(n), pe(n), pv(n), pb(n, nullptr);
  std::vector<const void*> pg(n);
  std::vector<float> lr(n), wd(n);
  std::vector<int> st(n);
  for (size_t i = 0; i < n; ++i) {
    const auto& p = masters[i];
    const auto& g = grads[i];
    auto check_f32 = [&](const at::Tensor& t, const char* name) {
      TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat &&
                      t.is_contiguous() && t.numel() == p.numel(),
                  name, " must be contiguous fp32 on GPU, numel matching");
    };
    check_f32(p, "master param");
    check_f32(exp_avgs[i], "exp_avg");
    check_f32(exp_avg_sqs[i], "exp_avg_sq");
    TORCH_CHECK(g.is_cuda() && g.is_contiguous(), "grad must be GPU");
    TORCH_CHECK(g.numel() == p.numel(), "grad/param numel mismatch");
    TORCH_CHECK(g.scalar_type() == (gbf16 ? at::kBFloat16 : at::kFloat),
                "grads of one call must all be bf16 or all be fp32");
    pm[i] = p.data_ptr();
    pg[i] = g.data_ptr();
    pe[i] = exp_avgs[i].data_ptr();
    pv[i] = exp_avg_sqs[i].data_ptr();
    if (params_bf16.has_value() && (*params_bf16)[i].has_value()) {
      const auto& b = *(*params_bf16)[i];
      check_bf16(b, "param_bf16");
      TORCH_CHECK(b.numel() == p.numel(), "param_bf16 numel mismatch");
      pb[i] = b.data_ptr();
    }
    lr[i] = (float)lrs[i];
    wd[i] = (float)weight_decays[i];
    st[i] = (int)steps[i];
  }
  const float* nsq = nullptr;
  if (norm_sq.has_value()) {
    TORCH_CHECK(norm_sq->is_cuda() && norm_sq->scalar_type() == at::kFloat &&
                    norm_sq->numel() >= 1,
                "norm_sq must be fp32 on GPU");
    nsq = (const float*)norm_sq->data_ptr();
  }
  TORCH_CHECK(mt_num_blocks((int)n, numel.data(), span) < (1LL << 31),
              "multi_tensor_adamw: too many spans");
  mt_adamw_launch((int)n, pm.data(), pg.data(), pe.data(), pv.data(),
                  pb.data(), numel.data(), lr.data(), wd.data(), st.data(),
                  gbf16 ? 1 : 0, (float)beta1, (float)beta2, (float)eps,
                  (float)grad_scale, nsq, (float)max_norm,
                  skip_nonfinite ? 1 : 0, span, cur_stream());
}

// ---- FP8 block-scaled moments (adamw_fp8.hip) -----------------------------
// Scales of a [..., C] tensor (C a multiple of the block) are [..., C / block].
std::vector<int64_t> f8_scale_sizes(const at::Tensor& t) {
  const int64_t block = f8_block_elems();
  TORCH_CHECK(t.dim() >= 1 && t.size(-1) % block == 0,
              "fp8 blocks: the last dim must be a multiple of ", block);
  auto sizes = t.sizes().vec();
  sizes.back() /= block;
  return sizes;
}

bool aligned16(const at::Tensor& t) {
  return t.numel() == 0 || ((uintptr_t)t.data_ptr() & 15u) == 0;
}

// codes (uint8, x's shape) and scales (fp32) of one state tensor
void check_f8_pair(const at::Tensor& codes, const at::Tensor& scales,
                   const char* name) {
  TORCH_CHECK(codes.is_cuda() && codes.scalar_type() == at::kByte &&
                  codes.is_contiguous() && aligned16(codes),
              name, " codes must be contiguous, 16-byte aligned uint8 on GPU");
  TORCH_CHECK(scales.is_cuda() && scales.scalar_type() == at::kFloat &&
                  scales.is_contiguous() &&
                  scales.sizes().vec() == f8_scale_sizes(codes),
              name, " scales must be contiguous fp32 on GPU, one per block");
}

std::tuple<at::Tensor, at::Tensor> fp8_block_quantize(const at::Tensor& x) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kFloat &&
                  x.is_contiguous() && aligned16(x),
              "fp8_block_quantize: x must be contiguous, 16-byte aligned fp32 "
              "on GPU");
  auto codes = at::empty(x.sizes(), x.options().dtype(at::kByte));
  auto scales = at::empty(f8_scale_sizes(x), x.options());
  f8_quantize_launch((const float*)x.data_ptr(), codes.data_ptr(),
                     (float*)scales.data_ptr(), scales.numel(), cur_stream());
  return {codes, scales};
}

at::Tensor fp8_block_dequantize(const at::Tensor& codes,
                                const at::Tensor& scales) {
  check_f8_pair(codes, scales, "fp8_block_dequantize:");
  auto out = at::empty(codes.sizes(), scales.options());
  f8_dequantize_launch(codes.data_ptr(), (const float*)scales.data_ptr(),
                       (float*)out.data_ptr(), scales.numel(), cur_stream());
  return out;
}

void multi_tensor_adamw_fp8(
    const std::vector<at::Tensor>& masters,
    const std::vector<at::Tensor>& grads,
    const std::vector<at::Tensor>& exp_avgs,
    const std::vector<at::Tensor>& exp_avg_scales,
    const std::vector<at::Tensor>& exp_avg_sq_roots,
    const std::vector<at::Tensor>& exp_avg_sq_root_scales,
    c10::optional<std::vector<c10::optional<at::Tensor>>> params_bf16,
    const std::vector<double>& lrs, const std::vector<double>& weight_decays,
    const std::vector<int64_t>& steps, double beta1, double beta2, double eps,
    double grad_scale, c10::optional<at::Tensor> norm_sq, double max_norm,
    bool skip_nonfinite, int64_t span_elems) {
  const size_t n = masters.size();
  TORCH_CHECK(grads.size() == n && exp_avgs.size() == n &&
                  exp_avg_scales.size() == n && exp_avg_sq_roots.size() == n &&
                  exp_avg_sq_root_scales.size() == n && lrs.size() == n &&
                  weight_decays.size() == n && steps.size() == n &&
                  (!params_bf16.has_value() || params_bf16->size() == n),
              "multi_tensor_adamw_fp8: list lengths differ");
  if (n == 0) return;
  const int64_t block = f8_block_elems();
  TORCH_CHECK(span_elems >= 0 && span_elems % block == 0 &&
                  span_elems < (1LL << 31),
              "span_elems must be 0 (automatic) or a positive multiple of ",
              block, " below 2^31");
  const auto numel = mt_numels(masters);
  long long span = span_elems;
  if (span == 0) {
    long long total = 0;
    for (long long k : numel) total += k;
    span = f8_auto_span(total);
  }
  const bool gbf16 = grads[0].scalar_type() == at::kBFloat16;
  std::vector<void*> pm(n), pe(n), pes(n), pr(n), prs(n), pb(n, nullptr);
  std::vector<const void*> pg(n);
  std::vector<float> lr(n), wd(n);
  std::vector<int> st(n);
  for (size_t i = 0; i < n; ++i) {
    const auto& p = masters[i];
    const auto& g = grads[i];
    TORCH_CHECK(p.is_cuda() && p.scalar_type() == at::kFloat &&
                    p.is_contiguous() && aligned16(p),
                "master param must be contiguous, 16-byte aligned fp32 on GPU");
    check_f8_pair(exp_avgs[i], exp_avg_scales[i], "exp_avg");
    check_f8_pair(exp_avg_sq_roots[i], exp_avg_sq_root_scales[i],
                  "exp_avg_sq_root");
    TORCH_CHECK(exp_avgs[i].sizes() == p.sizes() &&
                    exp_avg_sq_roots[i].sizes() == p.sizes(),
                "moment codes must have the master param's shape");
    TORCH_CHECK(g.is_cuda() && g.is_contiguous(), "grad must be GPU");
    TORCH_CHECK(g.numel() == p.numel(), "grad/param numel mismatch");
    TORCH_CHECK(g.scalar_type() == (gbf16 ? at::kBFloat16 : at::kFloat),
                "grads of one call must all be bf16 or all be fp32");
    pm[i] = p.data_ptr();
    pg[i] = g.data_ptr();
    pe[i] = exp_avgs[i].data_ptr();
    pes[i] = exp_avg_scales[i].data_ptr();
    pr[i] = exp_avg_sq_roots[i].data_ptr();
    prs[i] = exp_avg_sq_root_scales[i].data_ptr();
    if (params_bf16.has_value() && (*params_bf16)[i].has_value()) {
      const auto& b = *(*params_bf16)[i];
      check_bf16(b, "param_bf16");
      TORCH_CHECK(b.numel() == p.numel(), "param_bf16 numel mismatch");
      pb[i] = b.data_ptr();
    }
    lr[i] = (float)lrs[i];
    wd[i] = (float)weight_decays[i];
    st[i] = (int)steps[i];
  }
  const float* nsq = nullptr;
  if (norm_sq.has_value()) {
    TORCH_CHECK(norm_sq->is_cuda() && norm_sq->scalar_type() == at::kFloat &&
                    norm_sq->numel() >= 1,
                "norm_sq must be fp32 on GPU");
    nsq = (const float*)norm_sq->data_ptr();
  }
  TORCH_CHECK(mt_num_blocks((int)n, numel.data(), span) < (1LL << 31),
              "multi_tensor_adamw_fp8: too many spans");
  f8_adamw_launch((int)n, pm.data(), pg.data(), pe.data(), pes.data(),
                  pr.data(), prs.data(), pb.data(), numel.data(), lr.data(),
                  wd.data(), st.data(), gbf16 ? 1 : 0, (float)beta1,
                  (float)beta2, (float)eps, (float)grad_scale, nsq,
                  (float)max_norm, skip_nonfinite ? 1 : 0, span, cur_stream());
}

// ---- master-free AdamW with stochastic rounding (adamw_sr.hip) ------------
void sr_round(const at::Tensor& x, at::Tensor& out, uint64_t seed,
              int64_t stream, int64_t step) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kFloat &&
                  x.is_contiguous(),
              "sr_round: x must be contiguous fp32 on GPU");
  TORCH_CHECK(out.is_cuda() && out.device() == x.device() &&
                  out.scalar_type() == at::kBFloat16 && out.is_contiguous() &&
                  out.numel() == x.numel(),
              "sr_round: out must be contiguous bf16 on x's device, numel "
              "matching");
  TORCH_CHECK(stream >= 0 && stream < (1LL << 32) && step >= 0 &&
                  step < (1LL << 32),
              "sr_round: stream and step must fit 32 bits");
  if (x.numel() == 0) return;
  sr_round_launch((const float*)x.data_ptr(), out.data_ptr(),
                  (long long)x.numel(), seed, (unsigned int)stream,
                  (unsigned int)step, cur_stream());
}

// per-tensor scalars and the clip norm, shared by the two updates below
struct SrArgs {
  std::vector<float> lr, wd;
  std::vector<int> step, stream;
  const float* nsq = nullptr;
};

SrArgs sr_args(size_t n, const std::vector<double>& lrs,
               const std::vector<double>& weight_decays,
               const std::vector<int64_t>& steps,
               const std::vector<int64_t>& streams,
               const c10::optional<at::Tensor>& norm_sq) {
  TORCH_CHECK(lrs.size() == n && weight_decays.size() == n &&
                  steps.size() == n && streams.size() == n,
              "adamw_sr: list lengths differ");
  SrArgs a;
  a.lr.resize(n);
  a.wd.resize(n);
  a.step.resize(n);
  a.stream.resize(n);
  for (size_t i = 0; i < n; ++i) {
    TORCH_CHECK(steps[i] >= 1 && steps[i] < (1LL << 31) && streams[i] >= 0 &&
                    streams[i] < (1LL << 31),
                "adamw_sr: steps must be >= 1, streams >= 0, both below 2^31");
    a.lr[i] = (float)lrs[i];
    a.wd[i] = (float)weight_decays[i];
    a.step[i] = (int)steps[i];
    a.stream[i] = (int)streams[i];
  }
  if (norm_sq.has_value()) {
    TORCH_CHECK(norm_sq->is_cuda() && norm_sq->scalar_type() == at::kFloat &&
                    norm_sq->numel() >= 1,
                "norm_sq must be fp32 on GPU");
    a.nsq = (const float*)norm_sq->data_ptr();
  }
  return a;
}

// one bf16 weight and its gradient
void check_sr_pair(const at::Tensor& p, const at::Tensor& g, bool gbf16) {
  check_bf16(p, "param");
  TORCH_CHECK(g.is_cuda() && g.is_contiguous(), "grad must be GPU");
  TORCH_CHECK(g.numel() == p.numel(), "grad/param numel mismatch");
  TORCH_CHECK(g.scalar_type() == (gbf16 ? at::kBFloat16 : at::kFloat),
              "grads of one call must all be bf16 or all be fp32");
}

void multi_tensor_adamw_sr(
    const std::vector<at::Tensor>& params, const std::vector<at::Tensor>& grads,
    const std::vector<at::Tensor>& exp_avgs,
    const std::vector<at::Tensor>& exp_avg_sqs, const std::vector<double>& lrs,
    const std::vector<double>& weight_decays, const std::vector<int64_t>& steps,
    const std::vector<int64_t>& streams, double beta1, double beta2, double eps,
    double grad_scale, c10::optional<at::Tensor> norm_sq, double max_norm,
    bool skip_nonfinite, uint64_t seed, int64_t span_elems) {
  const size_t n = params.size();
  TORCH_CHECK(grads.size() == n && exp_avgs.size() == n &&
                  exp_avg_sqs.size() == n,
              "multi_tensor_adamw_sr: list lengths differ");
  if (n == 0) return;
  const SrArgs a = sr_args(n, lrs, weight_decays, steps, streams, norm_sq);
  const auto numel = mt_numels(params);
  const long long span = mt_span(numel, span_elems);
  const bool gbf16 = grads[0].scalar_type() == at::kBFloat16;
  std::vector<void*> pp(n), pe(n), pv(n);
  std::vector<const void*> pg(n);
  for (size_t i = 0; i < n; ++i) {
    const auto& p = params[i];
    check_sr_pair(p, grads[i], gbf16);
    for (const at::Tensor* t : {&exp_avgs[i], &exp_avg_sqs[i]})
      TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kFloat &&
                      t->is_contiguous() && t->numel() == p.numel(),
                  "moments must be contiguous fp32 on GPU, numel matching");
    pp[i] = p.data_ptr();
    pg[i] = grads[i].data_ptr();
    pe[i] = exp_avgs[i].data_ptr();
    pv[i] = exp_avg_sqs[i].data_ptr();
  }
  TORCH_CHECK(mt_num_blocks((int)n, numel.data(), span) < (1LL << 31),
              "multi_tensor_adamw_sr: too many spans");
  sr_adamw_launch((int)n, pp.data(), pg.data(), pe.data(), pv.data(),
                  numel.data(), a.lr.data(), a.wd.data(), a.step.data(),
                  a.stream.data(), gbf16 ? 1 : 0, (float)beta1, (float)beta2,
                  (float)eps, (float)grad_scale, a.nsq, (float)max_norm,
                  skip_nonfinite ? 1 : 0, seed, span, cur_stream());
}

void multi_tensor_adamw_fp8_sr(
    const std::vector<at::Tensor>& params, const std::vector<at::Tensor>& grads,
    const std::vector<at::Tensor>& exp_avgs,
    const std::vector<at::Tensor>& exp_avg_scales,
    const std::vector<at::Tensor>& exp_avg_sq_roots,
    const std::vector<at::Tensor>& exp_avg_sq_root_scales,
    const std::vector<double>& lrs, const std::vector<double>& weight_decays,
    const std::vector<int64_t>& steps, const std::vector<int64_t>& streams,
    double beta1, double beta2, double eps, double grad_scale,
    c10::optional<at::Tensor> norm_sq, double max_norm, bool skip_nonfinite,
    uint64_t seed, int64_t span_elems) {
  const size_t n = params.size();
  TORCH_CHECK(grads.size() == n && exp_avgs.size() == n &&
                  exp_avg_scales.size() == n && exp_avg_sq_roots.size() == n &&
                  exp_avg_sq_root_scales.size() == n,
              "multi_tensor_adamw_fp8_sr: list lengths differ");
  if (n == 0) return;
  const SrArgs a = sr_args(n, lrs, weight_decays, steps, streams, norm_sq);
  const int64_t block = f8_block_elems();
  TORCH_CHECK(span_elems >= 0 && span_elems % block == 0 &&
                  span_elems < (1LL << 31),
              "span_elems must be 0 (automatic) or a positive multiple of ",
              block, " below 2^31");
  const auto numel = mt_numels(params);
  long long span = span_elems;
  if (span == 0) {
    long long total = 0;
    for (long long k : numel) total += k;
    span = f8_auto_span(total);
  }
  const bool gbf16 = grads[0].scalar_type() == at::kBFloat16;
  std::vector<void*> pp(n), pe(n), pes(n), pr(n), prs(n);
  std::vector<const void*> pg(n);
  for (size_t i = 0; i < n; ++i) {
    const auto& p = params[i];
    check_sr_pair(p, grads[i], gbf16);
    check_f8_pair(exp_avgs[i], exp_avg_scales[i], "exp_avg");
    check_f8_pair(exp_avg_sq_roots[i], exp_avg_sq_root_scales[i],
                  "exp_avg_sq_root");
    TORCH_CHECK(exp_avgs[i].sizes() == p.sizes() &&
                    exp_avg_sq_roots[i].sizes() == p.sizes(),
                "moment codes must have the param's shape");
    pp[i] = p.data_ptr();
    pg[i] = grads[i].data_ptr();
    pe[i] = exp_avgs[i].data_ptr();
    pes[i] = exp_avg_scales[i].data_ptr();
    pr[i] = exp_avg_sq_roots[i].data_ptr();
    prs[i] = exp_avg_sq_root_scales[i].data_ptr();
  }
  TORCH_CHECK(mt_num_blocks((int)n, numel.data(), span) < (1LL << 31),
              "multi_tensor_adamw_fp8_sr: too many spans");
  sr_f8_adamw_launch((int)n, pp.data(), pg.data(), pe.data(), pes.data(),
                     pr.data(), prs.data(), numel.data(), a.lr.data(),
                     a.wd.data(), a.step.data(), a.stream.data(),
                     gbf16 ? 1 : 0, (float)beta1, (float)beta2, (float)eps,
                     (float)grad_scale, a.nsq, (float)max_norm,
                     skip_nonfinite ? 1 : 0, seed, span, cur_stream());
}

// ---- FP8 tensor-wise cast for the linear layers (fp8_cast.hip) -----------
// x: [R, C] bf16 or fp32, contiguous, 16-byte aligned, R and C multiples of 16
bool check_fp8_cast_input(const at::Tensor& x, const char* op) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.is_contiguous() && aligned16(x),
              op, ": x must be a contiguous, 16-byte aligned 2-D GPU tensor");
  TORCH_CHECK(x.size(0) % 16 == 0 && x.size(1) % 16 == 0 && x.numel() > 0,
              op, ": both dimensions must be positive multiples of 16");
  const bool bf16 = x.scalar_type() == at::kBFloat16;
  TORCH_CHECK(bf16 || x.scalar_type() == at::kFloat, op,
              ": x must be bf16 or fp32");
  return bf16;
}

int fp8_fmt_code(const std::string& fmt) {
  TORCH_CHECK(fmt == "e4m3" || fmt == "e5m2", "fp8 format must be 'e4m3' or "
              "'e5m2', got '", fmt, "'");
  return fmt == "e5m2" ? FP8_FMT_E5M2 : FP8_FMT_E4M3;
}

void check_fp8_scale(const at::Tensor& scale, const at::Tensor& x) {
  TORCH_CHECK(scale.is_cuda() && scale.scalar_type() == at::kFloat &&
                  scale.numel() == 1 && scale.device() == x.device(),
              "fp8 scale must be a 1-element fp32 tensor on x's device");
}

int64_t fp8_amax_slots(const at::Tensor& x) {
  return fp8_amax_num_partials((long long)x.numel(),
                               x.scalar_type() == at::kBFloat16);
}

// scale[0] = absmax(x) / FMAX; partials: int32 workspace of fp8_amax_slots(x)
void fp8_amax_scale(const at::Tensor& x, const std::string& fmt,
                    at::Tensor& partials, at::Tensor& scale) {
  const bool bf16 = check_fp8_cast_input(x, "fp8_amax_scale");
  check_fp8_scale(scale, x);
  const long long need = fp8_amax_num_partials((long long)x.numel(), bf16);
  TORCH_CHECK(partials.is_cuda() && partials.is_contiguous() &&
                  partials.scalar_type() == at::kInt &&
                  partials.numel() >= need,
              "fp8_amax_scale: partials must be contiguous int32 on GPU with "
              "at least ", need, " elements");
  fp8_amax_scale_launch(x.data_ptr(), (long long)x.numel(), bf16,
                        fp8_fmt_code(fmt), (unsigned int*)partials.data_ptr(),
                        (float*)scale.data_ptr(), (hipStream_t)cur_stream());
}

// (codes [R, C] | None, codes_t [C, R] | None) as uint8
std::tuple<c10::optional<at::Tensor>, c10::optional<at::Tensor>>
fp8_cast_transpose(const at::Tensor& x, const at::Tensor& scale,
                   const std::string& fmt, bool rowwise, bool colwise) {
  const bool bf16 = check_fp8_cast_input(x, "fp8_cast_transpose");
  check_fp8_scale(scale, x);
  c10::optional<at::Tensor> codes, codes_t;
  const int64_t R = x.size(0), C = x.size(1);
  if (rowwise) codes = at::empty({R, C}, x.options().dtype(at::kByte));
  if (colwise) codes_t = at::empty({C, R}, x.options().dtype(at::kByte));
  fp8_cast_transpose_launch(
      x.data_ptr(), (const float*)scale.data_ptr(),
      rowwise ? codes->data_ptr() : nullptr,
      colwise ? codes_t->data_ptr() : nullptr, R, C, bf16, fp8_fmt_code(fmt),
      (hipStream_t)cur_stream());
  return {codes, codes_t};
}

// ---- checkpoint pack / unpack / checksum (ckpt_pack.hip) ------------------
// span_bytes == 0 picks the span from the list's total size; any other value
// must be a multiple of the block's trip (threads x 16 bytes).
long long ckpt_span(const std::vector<long long>& nbytes, int64_t span_bytes) {
  const long long q = ckpt_span_quantum();
  TORCH_CHECK(span_bytes >= 0 && span_bytes % q == 0 &&
                  span_bytes < (1LL << 31),
              "span_bytes must be 0 (automatic) or a positive multiple of ", q,
              " below 2^31");
  if (span_bytes > 0) return span_bytes;
  long long total = 0;
  for (long long n : nbytes) total += n;
  return ckpt_auto_span(total);
}

int64_t ckpt_sum_slots(const std::vector<int64_t>& nbytes_list,
                       int64_t span_bytes) {
  std::vector<long long> nbytes(nbytes_list.begin(), nbytes_list.end());
  for (long long n : nbytes) TORCH_CHECK(n >= 0, "negative nbytes");
  return ckpt_num_slots((int)nbytes.size(), nbytes.data(),
                        ckpt_span(nbytes, span_bytes));
}

// mode 0 (pack):   tensors[i] -> staging[offsets[i] ...)
// mode 1 (unpack): staging[offsets[i] ...) -> tensors[i]
// mode 2 (sum):    read tensors[i] only; staging and offsets unused
// Every mode writes the checksum of tensor i's bytes to sums[i].
void ckpt_copy_sum(int64_t mode, const std::vector<at::Tensor>& tensors,
                   c10::optional<at::Tensor> staging,
                   const std::vector<int64_t>& offsets, at::Tensor& partials,
                   at::Tensor& sums, int64_t span_bytes) {
  TORCH_CHECK(mode >= 0 && mode <= 2, "ckpt_copy_sum: mode must be 0, 1 or 2");
  const int n = (int)tensors.size();
  if (n == 0) return;
  unsigned char* stage = nullptr;
  long long stage_bytes = 0;
  if (mode != 2) {
    TORCH_CHECK(staging.has_value() && staging->is_cuda() &&
                    staging->is_contiguous() &&
                    staging->scalar_type() == at::kByte,
                "ckpt: staging must be a contiguous uint8 tensor on GPU");
    TORCH_CHECK((int)offsets.size() == n, "ckpt: one offset per tensor");
    stage = (unsigned char*)staging->data_ptr();
    stage_bytes = (long long)staging->numel();
  }
  std::vector<long long> nbytes(n);
  std::vector<const void*> src(n);
  std::vector<void*> dst(n, nullptr);
  for (int i = 0; i < n; ++i) {
    const auto& t = tensors[i];
    TORCH_CHECK(t.is_cuda(), "ckpt: tensors must be on GPU");
    TORCH_CHECK(t.numel() == 0 || t.is_contiguous(),
                "ckpt: tensors must be contiguous");
    nbytes[i] = (long long)t.numel() * (long long)t.element_size();
    void* tp = nbytes[i] ? t.data_ptr() : nullptr;
    void* sp = nullptr;
    if (mode != 2) {
      TORCH_CHECK(offsets[i] >= 0 && offsets[i] + nbytes[i] <= stage_bytes,
                  "ckpt: tensor ", i, " at offset ", offsets[i], " with ",
                  nbytes[i], " bytes does not fit the staging buffer of ",
                  stage_bytes, " bytes");
      sp = stage + offsets[i];
    }
    if (mode == 1) {
      src[i] = sp;
      dst[i] = tp;
    } else {
      src[i] = tp;
      dst[i] = sp;
    }
  }
  const long long span = ckpt_span(nbytes, span_bytes);
  const long long need = ckpt_num_slots(n, nbytes.data(), span);
  TORCH_CHECK(need < (1LL << 31), "ckpt: too many spans");
  TORCH_CHECK(partials.is_cuda() && partials.is_contiguous() &&
                  partials.scalar_type() == at::kLong &&
                  partials.numel() >= 2 * need,
              "ckpt: partials must be contiguous int64 on GPU with at least ",
              need, " x 2 elements");
  TORCH_CHECK(sums.is_cuda() && sums.is_contiguous() &&
                  sums.scalar_type() == at::kLong && sums.numel() >= 2LL * n,
              "ckpt: sums must be contiguous int64 on GPU with at least ", n,
              " x 2 elements");
  ckpt_copy_sum_launch(n, src.data(), mode == 2 ? nullptr : dst.data(),
                       nbytes.data(), span, (long long*)partials.data_ptr(),
                       (long long*)sums.data_ptr(), cur_stream());
}

// ---- mixture of experts (moe.hip) ------------------------------------------
void check_moe_tensor(const at::Tensor& t, at::ScalarType dtype,
                      const char* name) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.scalar_type() == dtype,
              "moe: ", name, " must be a contiguous ", dtype, " GPU tensor");
}

// bf16 [rows, H] with H % 8 == 0 and 16-byte aligned rows
void check_moe_rows(const at::Tensor& t, const char* name) {
  check_moe_tensor(t, at::kBFloat16, name);
  TORCH_CHECK(t.dim() == 2 && t.size(1) > 0 && t.size(1) % 8 == 0 &&
                  t.size(1) < (1LL << 31) &&
                  reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
              "moe: ", name, " must be 16-byte aligned [rows, H], H % 8 == 0");
}

// Validates [T, k] against the supported range; returns T.
long long check_moe_tk(const at::Tensor& t, int64_t E, const char* name) {
  TORCH_CHECK(t.dim() == 2, "moe: ", name, " must be [T, k]");
  const int64_t T = t.size(0), k = t.size(1);
  TORCH_CHECK(E >= 2 && E <= MOE_MAX_EXPERTS, "moe: 2 <= E <= ",
              MOE_MAX_EXPERTS, " experts, got ", E);
  TORCH_CHECK(k >= 1 && k <= MOE_MAX_TOPK && k <= E,
              "moe: 1 <= k <= min(", MOE_MAX_TOPK, ", E), got ", k);
  TORCH_CHECK(T * k < (1LL << 31), "moe: T * k must stay below 2^31");
  return T;
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> moe_router_fwd(
    const at::Tensor& logits, int64_t k, bool norm_topk) {
  check_moe_tensor(logits, at::kBFloat16, "logits");
  TORCH_CHECK(logits.dim() == 2, "moe: logits must be [T, E]");
  const int64_t T = logits.size(0), E = logits.size(1);
  TORCH_CHECK(k >= 1 && k <= MOE_MAX_TOPK, "moe: 1 <= k <= ", MOE_MAX_TOPK);
  auto topk_idx = at::empty({T, k}, logits.options().dtype(at::kInt));
  auto topk_w = at::empty({T, k}, logits.options().dtype(at::kFloat));
  check_moe_tk(topk_idx, E, "topk_idx");
  auto probs_mean = at::zeros({E}, logits.options().dtype(at::kFloat));
  if (T == 0) return {topk_idx, topk_w, probs_mean};
  auto partials = at::empty({moe_router_num_partials(T), E},
                            logits.options().dtype(at::kFloat));
  moe_router_fwd_launch(logits.data_ptr(), (int*)topk_idx.data_ptr(),
                        (float*)topk_w.data_ptr(),
                        (float*)probs_mean.data_ptr(),
                        (float*)partials.data_ptr(), T, (int)E, (int)k,
                        norm_topk ? 1 : 0, attn_stream());
  return {topk_idx, topk_w, probs_mean};
}

at::Tensor moe_router_bwd(const at::Tensor& logits, const at::Tensor& topk_idx,
                          const at::Tensor& d_topk_w,
                          const at::Tensor& d_probs_mean, bool norm_topk) {
  check_moe_tensor(logits, at::kBFloat16, "logits");
  check_moe_tensor(topk_idx, at::kInt, "topk_idx");
  check_moe_tensor(d_topk_w, at::kFloat, "d_topk_w");
  check_moe_tensor(d_probs_mean, at::kFloat, "d_probs_mean");
  TORCH_CHECK(logits.dim() == 2, "moe: logits must be [T, E]");
  const int64_t E = logits.size(1);
  const long long T = check_moe_tk(topk_idx, E, "topk_idx");
  TORCH_CHECK(logits.size(0) == T && d_topk_w.sizes() == topk_idx.sizes() &&
                  d_probs_mean.numel() == E,
              "moe_router_bwd: shapes must be logits [T, E], topk_idx and "
              "d_topk_w [T, k], d_probs_mean [E]");
  auto dlogits = at::empty_like(logits);
  if (T > 0)
    moe_router_bwd_launch(logits.data_ptr(), (const int*)topk_idx.data_ptr(),
                          (const float*)d_topk_w.data_ptr(),
                          (const float*)d_probs_mean.data_ptr(),
                          dlogits.data_ptr(), T, (int)E,
                          (int)topk_idx.size(1), norm_topk ? 1 : 0,
                          attn_stream());
  return dlogits;
}

// -> offs [E], row_of_slot [T*k], slot_of_row [T*k], all int32
std::tuple<at::Tensor, at::Tensor, at::Tensor> moe_sort(
    const at::Tensor& topk_idx, int64_t num_experts) {
  check_moe_tensor(topk_idx, at::kInt, "topk_idx");
  const long long n_slots =
      check_moe_tk(topk_idx, num_experts, "topk_idx") * topk_idx.size(1);
  auto offs = at::zeros({num_experts}, topk_idx.options());
  auto row_of_slot = at::empty({n_slots}, topk_idx.options());
  auto slot_of_row = at::empty({n_slots}, topk_idx.options());
  if (n_slots == 0) return {offs, row_of_slot, slot_of_row};
  auto hist = at::empty({num_experts, moe_sort_num_blocks(n_slots)},
                        topk_idx.options());
  moe_sort_launch((const int*)topk_idx.data_ptr(), (int*)hist.data_ptr(),
                  (int*)offs.data_ptr(), (int*)row_of_slot.data_ptr(),
                  (int*)slot_of_row.data_ptr(), n_slots, (int)num_experts,
                  attn_stream());
  return {offs, row_of_slot, slot_of_row};
}

// An index array of T * k slots.
void check_moe_slots(const at::Tensor& idx, int64_t T, int64_t k,
                     const char* name) {
  check_moe_tensor(idx, at::kInt, name);
  TORCH_CHECK(k >= 1 && k <= MOE_MAX_TOPK, "moe: 1 <= k <= ", MOE_MAX_TOPK);
  TORCH_CHECK(T * k < (1LL << 31) && idx.numel() == T * k, "moe: ", name,
              " must hold T * k = ", T * k, " slots (< 2^31), got ",
              idx.numel());
}

at::Tensor moe_dispatch(const at::Tensor& x, const at::Tensor& slot_of_row,
                        int64_t k) {
  check_moe_rows(x, "x");
  const int64_t T = x.size(0), H = x.size(1);
  check_moe_slots(slot_of_row, T, k, "slot_of_row");
  auto xp = at::empty({T * k, H}, x.options());
  if (T > 0)
    moe_dispatch_launch(x.data_ptr(), (const int*)slot_of_row.data_ptr(),
                        xp.data_ptr(), T, (int)k, (int)H, attn_stream());
  return xp;
}

// topk_w absent: unit weights, k given (the dispatch backward)
at::Tensor moe_combine_fwd(const at::Tensor& yp,
                           c10::optional<at::Tensor> topk_w,
                           const at::Tensor& row_of_slot, int64_t k) {
  check_moe_rows(yp, "yp");
  const float* w = nullptr;
  if (topk_w.has_value()) {
    check_moe_tensor(*topk_w, at::kFloat, "topk_w");
    TORCH_CHECK(topk_w->dim() == 2 && topk_w->size(1) == k,
                "moe: topk_w must be [T, k]");
    w = (const float*)topk_w->data_ptr();
  }
  TORCH_CHECK(k >= 1 && yp.size(0) % k == 0, "moe: yp must have T * k rows");
  const int64_t T = yp.size(0) / k, H = yp.size(1);
  TORCH_CHECK(!topk_w.has_value() || topk_w->size(0) == T,
              "moe: topk_w must be [T, k]");
  check_moe_slots(row_of_slot, T, k, "row_of_slot");
  auto y = at::empty({T, H}, yp.options());
  if (T > 0)
    moe_combine_fwd_launch(yp.data_ptr(), w,
                           (const int*)row_of_slot.data_ptr(), y.data_ptr(),
                           T, (int)k, (int)H, attn_stream());
  return y;
}

// -> dyp [T*k, H] bf16, d_topk_w [T, k] fp32
std::tuple<at::Tensor, at::Tensor> moe_combine_bwd(
    const at::Tensor& dy, const at::Tensor& yp, const at::Tensor& topk_w,
    const at::Tensor& row_of_slot) {
  check_moe_rows(dy, "dy");
  check_moe_rows(yp, "yp");
  check_moe_tensor(topk_w, at::kFloat, "topk_w");
  TORCH_CHECK(topk_w.dim() == 2, "moe: topk_w must be [T, k]");
  const int64_t T = topk_w.size(0), k = topk_w.size(1), H = yp.size(1);
  check_moe_slots(row_of_slot, T, k, "row_of_slot");
  TORCH_CHECK(dy.size(0) == T && dy.size(1) == H && yp.size(0) == T * k,
              "moe_combine_bwd: shapes must be dy [T, H], yp [T*k, H]");
  auto dyp = at::empty_like(yp);
  auto dw = at::empty_like(topk_w);
  if (T > 0)
    moe_combine_bwd_launch(dy.data_ptr(), yp.data_ptr(),
                           (const float*)topk_w.data_ptr(),
                           (const int*)row_of_slot.data_ptr(), dyp.data_ptr(),
                           (float*)dw.data_ptr(), T, (int)k, (int)H,
                           attn_stream());
  return {dyp, dw};
}

// ---- grouped GEMMs of the experts (moe_gemm.hip) ---------------------------
// bf16 [rows, C] with C % 32 == 0 and 16-byte aligned rows
void check_moe_gemm_rows(const at::Tensor& t, const char* name) {
  check_moe_tensor(t, at::kBFloat16, name);
  TORCH_CHECK(t.dim() == 2 && t.size(1) > 0 && t.size(1) % 32 == 0 &&
                  t.size(1) < (1LL << 23) && t.size(0) < (1LL << 31) &&
                  reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
              "moe_gemm: ", name,
              " must be 16-byte aligned [rows < 2^31, C < 2^23], C % 32 == 0");
}

// offs [E] with 2 <= E <= 256; returns E
int check_moe_gemm_offs(const at::Tensor& offs) {
  check_moe_tensor(offs, at::kInt, "offs");
  TORCH_CHECK(offs.dim() == 1 && offs.numel() >= 2 &&
                  offs.numel() <= MOE_GEMM_MAX_EXPERTS,
              "moe_gemm: offs must be [E], 2 <= E <= ", MOE_GEMM_MAX_EXPERTS);
  return (int)offs.numel();
}

// w [E, K, N] against the [rows, K] and [rows, N] operands
void check_moe_gemm_w(const at::Tensor& w, int E, int64_t K, int64_t N) {
  check_moe_tensor(w, at::kBFloat16, "w");
  TORCH_CHECK(w.dim() == 3 && w.size(0) == E && w.size(1) == K &&
                  w.size(2) == N &&
                  reinterpret_cast<uintptr_t>(w.data_ptr()) % 16 == 0,
              "moe_gemm: w must be 16-byte aligned [E, K, N] = [", E, ", ", K,
              ", ", N, "]");
}

// The gather of the fused dispatch: slot_of_row [R] over a [T, K], R = T * k.
// Returns R; without a gather R is a's row count.
int64_t check_moe_gemm_gather(const at::Tensor& a,
                              const c10::optional<at::Tensor>& slot_of_row,
                              int64_t k) {
  if (!slot_of_row.has_value()) return a.size(0);
  check_moe_slots(*slot_of_row, a.size(0), k, "slot_of_row");
  return slot_of_row->numel();
}

at::Tensor moe_gemm_fwd(const at::Tensor& a, const at::Tensor& w,
                        const at::Tensor& offs,
                        c10::optional<at::Tensor> slot_of_row, int64_t k) {
  check_moe_gemm_rows(a, "a");
  const int E = check_moe_gemm_offs(offs);
  TORCH_CHECK(w.dim() == 3, "moe_gemm: w must be [E, K, N]");
  const int64_t K = a.size(1), N = w.size(2);
  check_moe_gemm_w(w, E, K, N);
  TORCH_CHECK(N % 32 == 0 && N < (1LL << 23), "moe_gemm: N % 32 == 0");
  const int64_t R = check_moe_gemm_gather(a, slot_of_row, k);
  auto y = at::empty({R, N}, a.options());
  if (R > 0)
    moe_gemm_fwd_launch(
        a.data_ptr(), w.data_ptr(), (const int*)offs.data_ptr(),
        slot_of_row.has_value() ? (const int*)slot_of_row->data_ptr() : nullptr,
        y.data_ptr(), R, a.size(0), (int)k, E, (int)K, (int)N, attn_stream());
  return y;
}

at::Tensor moe_gemm_dgrad(const at::Tensor& dy, const at::Tensor& w,
                          const at::Tensor& offs) {
  check_moe_gemm_rows(dy, "dy");
  const int E = check_moe_gemm_offs(offs);
  TORCH_CHECK(w.dim() == 3, "moe_gemm: w must be [E, K, N]");
  const int64_t K = w.size(1), N = dy.size(1), R = dy.size(0);
  check_moe_gemm_w(w, E, K, N);
  TORCH_CHECK(K % 32 == 0 && K < (1LL << 23), "moe_gemm: K % 32 == 0");
  auto da = at::empty({R, K}, dy.options());
  if (R > 0)
    moe_gemm_dgrad_launch(dy.data_ptr(), w.data_ptr(),
                          (const int*)offs.data_ptr(), da.data_ptr(), R, E,
                          (int)K, (int)N, attn_stream());
  return da;
}

at::Tensor moe_gemm_wgrad(const at::Tensor& a, const at::Tensor& dy,
                          const at::Tensor& offs,
                          c10::optional<at::Tensor> slot_of_row, int64_t k) {
  check_moe_gemm_rows(a, "a");
  check_moe_gemm_rows(dy, "dy");
  const int E = check_moe_gemm_offs(offs);
  const int64_t K = a.size(1), N = dy.size(1);
  const int64_t R = check_moe_gemm_gather(a, slot_of_row, k);
  TORCH_CHECK(dy.size(0) == R, "moe_gemm: dy must have ", R, " rows");
  if (R == 0) return at::zeros({E, K, N}, a.options());
  auto dw = at::empty({E, K, N}, a.options());
  moe_gemm_wgrad_launch(
      a.data_ptr(), dy.data_ptr(), (const int*)offs.data_ptr(),
      slot_of_row.has_value() ? (const int*)slot_of_row->data_ptr() : nullptr,
      dw.data_ptr(), R, a.size(0), (int)k, E, (int)K, (int)N, attn_stream());
  return dw;
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "dlrover_amd CDNA4 (gfx950) kernels";
  m.def("rmsnorm_fwd", &rmsnorm_fwd, "fused RMSNorm forward (bf16)");
  m.def("rmsnorm_bwd", &rmsnorm_bwd, "fused RMSNorm backward (bf16)");
  m.def("rmsnorm_add_fwd", &rmsnorm_add_fwd,
        "fused residual-add + RMSNorm forward -> (h, y, invrms)");
  m.def("rope_apply", &rope_apply, "in-place RoPE rotate-half (bf16)");
  m.def("rope_rotate_oop", &rope_rotate_oop,
        "out-of-place RoPE: strided source -> contiguous output");
  m.def("qk_norm_rope_fwd", &qk_norm_rope_fwd,
        "fused per-head RMSNorm + RoPE of q and k, forward (bf16)");
  m.def("qk_norm_rope_bwd", &qk_norm_rope_bwd,
        "fused per-head RMSNorm + RoPE of q and k, backward (bf16)");
  m.def("moe_router_fwd", &moe_router_fwd,
        "MoE router: logits [T, E] bf16 -> (topk_idx int32 [T, k], topk_w "
        "fp32 [T, k], probs_mean fp32 [E]); top-k on the logits, ties to the "
        "lower expert",
        py::arg("logits"), py::arg("k"), py::arg("norm_topk"));
  m.def("moe_router_bwd", &moe_router_bwd, "MoE router backward -> dlogits",
        py::arg("logits"), py::arg("topk_idx"), py::arg("d_topk_w"),
        py::arg("d_probs_mean"), py::arg("norm_topk"));
  m.def("moe_sort", &moe_sort,
        "stable counting sort of the T*k slots by expert -> (offs [E], "
        "row_of_slot, slot_of_row), int32, counts stay on the device",
        py::arg("topk_idx"), py::arg("num_experts"));
  m.def("moe_dispatch", &moe_dispatch,
        "xp[r] = x[slot_of_row[r] / k] (bf16 row gather)", py::arg("x"),
        py::arg("slot_of_row"), py::arg("k"));
  m.def("moe_combine_fwd", &moe_combine_fwd,
        "y[t] = sum_j topk_w[t, j] * yp[row_of_slot[t*k+j]]; unit weights "
        "when topk_w is None",
        py::arg("yp"), py::arg("topk_w"), py::arg("row_of_slot"),
        py::arg("k"));
  m.def("moe_combine_bwd", &moe_combine_bwd,
        "MoE combine backward -> (dyp bf16 [T*k, H], d_topk_w fp32 [T, k])",
        py::arg("dy"), py::arg("yp"), py::arg("topk_w"),
        py::arg("row_of_slot"));
  m.def("moe_gemm_fwd", &moe_gemm_fwd,
        "grouped GEMM y[r] = a(r) @ w[e(r)] (bf16, MFMA); a(r) = a[r], or "
        "a[slot_of_row[r] / k] with the dispatch fused in",
        py::arg("a"), py::arg("w"), py::arg("offs"), py::arg("slot_of_row"),
        py::arg("k"));
  m.def("moe_gemm_dgrad", &moe_gemm_dgrad,
        "grouped GEMM da[r] = dy[r] @ w[e(r)]^T from the same w", py::arg("dy"),
        py::arg("w"), py::arg("offs"));
  m.def("moe_gemm_wgrad", &moe_gemm_wgrad,
        "grouped GEMM dw[e] = sum over e's rows of a(r)^T dy[r] -> [E, K, N] "
        "bf16, zeros for an empty expert",
        py::arg("a"), py::arg("dy"), py::arg("offs"), py::arg("slot_of_row"),
        py::arg("k"));
  m.def("swiglu_fwd", &swiglu_fwd, "fused SwiGLU forward (bf16)");
  m.def("swiglu_bwd", &swiglu_bwd, "fused SwiGLU backward (bf16)");
  m.def("adamw_step", &adamw_step, "fused AdamW with fp32 master weights");
  m.def("causal_softmax_fwd", &causal_softmax_fwd,
        "in-place fused scale+causal-mask+softmax (bf16)");
  m.def("causal_softmax_bwd", &causal_softmax_bwd,
        "in-place softmax backward (bf16)");
  m.def("cross_entropy_fwd_bwd", &cross_entropy_fwd_bwd,
        "fused CE loss + in-place dlogits (bf16)");
  m.def("ce_shard_stats", &ce_shard_stats,
        "vocab-parallel CE, stage 1: per-row (max, sumexp, target logit) of "
        "one vocab shard -> fp32 [N,3]",
        py::arg("logits_shard"), py::arg("targets"), py::arg("vocab_start"),
        py::arg("ignore_index"));
  m.def("ce_shard_finish", &ce_shard_finish,
        "vocab-parallel CE, stage 2: combine stats_all [tp,N,3] -> losses, "
        "in-place dlogits of the shard",
        py::arg("logits_shard"), py::arg("targets"), py::arg("vocab_start"),
        py::arg("stats_all"), py::arg("grad_scale"), py::arg("ignore_index"),
        py::arg("compute_grad"));
  m.def("tr_b16_probe", []() {
    auto out = at::empty({64, 12}, at::TensorOptions()
                                      .dtype(at::kBFloat16)
                                      .device(at::kCUDA));
    tr_b16_probe_launch(out.data_ptr(), cur_stream());
    return out;
  }, "ds_read_b64_tr_b16 semantics probe");
  m.def("mfma16_probe", &mfma16_probe, "MFMA 16x16x32 bf16 layout self-test");
  m.def("mfma32_probe", &mfma32_probe, "MFMA 32x32x16 bf16 layout self-test");
  m.def("memcpy_d2h_async", &memcpy_d2h_async,
        "hipMemcpyAsync device tensor -> registered host address");
  m.def("memcpy_h2d_async", &memcpy_h2d_async,
        "hipMemcpyAsync registered host address -> device tensor");
  m.def("tr_b16_probe3", []() {
    auto out = at::empty({64, 12}, at::TensorOptions()
                                      .dtype(at::kShort)
                                      .device(at::kCUDA));
    tr_b16_probe3_launch(out.data_ptr(), cur_stream());
    return out;
  }, "tr_b16 cooperative tile-sourcing probe (raw index bits)");
  m.def("flash_attn_fwd", &flash_attn_fwd,
        "flash attention forward (bf16, causal, GQA, D=128) -> (out, lse)");
  m.def("flash_attn_bwd", &flash_attn_bwd,
        "flash attention backward -> (dq, dk, dv)");
  m.def("flash_attn_doc_fwd", &flash_attn_doc_fwd,
        "document-masked flash attention forward: query i sees key j iff "
        "doc_start[b,i] <= j <= i (int32 [B,S]; D=128, S%256==0) -> (out, lse)");
  m.def("flash_attn_doc_bwd", &flash_attn_doc_bwd,
        "document-masked flash attention backward (doc_end[b,j] = exclusive "
        "end of j's document) -> (dq, dk, dv)");
  m.attr("MT_MAX_TENSORS") = mt_max_tensors();
  m.def("multi_tensor_num_partials", &multi_tensor_num_partials,
        "partial slots multi_tensor_sq_norm needs for a tensor list",
        py::arg("tensors"), py::arg("span_elems") = 0);
  m.def("multi_tensor_sq_norm", &multi_tensor_sq_norm,
        "sum of squares over a tensor list -> out[0] (fp32, no atomics)",
        py::arg("tensors"), py::arg("partials"), py::arg("out"),
        py::arg("span_elems") = 0);
  m.def("multi_tensor_adamw", &multi_tensor_adamw,
        "batched fused AdamW with an optional device-side clip coefficient",
        py::arg("masters"), py::arg("grads"), py::arg("exp_avgs"),
        py::arg("exp_avg_sqs"), py::arg("params_bf16"), py::arg("lrs"),
        py::arg("weight_decays"), py::arg("steps"), py::arg("beta1"),
        py::arg("beta2"), py::arg("eps"), py::arg("grad_scale"),
        py::arg("norm_sq"), py::arg("max_norm"), py::arg("skip_nonfinite"),
        py::arg("span_elems") = 0);
  m.attr("F8_MAX_TENSORS") = f8_max_tensors();
  m.attr("F8_BLOCK") = f8_block_elems();
  m.def("fp8_block_quantize", &fp8_block_quantize,
        "fp32 [..., C] -> (e4m3fn codes as uint8 [..., C], fp32 scales "
        "[..., C/256]); scale = absmax/448 per 256-block",
        py::arg("x"));
  m.def("fp8_block_dequantize", &fp8_block_dequantize,
        "(codes, scales) of fp8_block_quantize -> fp32", py::arg("codes"),
        py::arg("scales"));
  m.def("multi_tensor_adamw_fp8", &multi_tensor_adamw_fp8,
        "batched fused AdamW on FP8 block-scaled moments (exp_avg and "
        "sqrt(exp_avg_sq)) with an optional device-side clip coefficient",
        py::arg("masters"), py::arg("grads"), py::arg("exp_avgs"),
        py::arg("exp_avg_scales"), py::arg("exp_avg_sq_roots"),
        py::arg("exp_avg_sq_root_scales"), py::arg("params_bf16"),
        py::arg("lrs"), py::arg("weight_decays"), py::arg("steps"),
        py::arg("beta1"), py::arg("beta2"), py::arg("eps"),
        py::arg("grad_scale"), py::arg("norm_sq"), py::arg("max_norm"),
        py::arg("skip_nonfinite"), py::arg("span_elems") = 0);
  m.attr("SR_MAX_TENSORS") = sr_max_tensors();
  m.def("sr_round", &sr_round,
        "out = stochastic rounding of fp32 x to bf16, Philox4x32-10 noise "
        "keyed on (seed, stream, step, element index)",
        py::arg("x"), py::arg("out"), py::arg("seed"), py::arg("stream"),
        py::arg("step"));
  m.def("multi_tensor_adamw_sr", &multi_tensor_adamw_sr,
        "batched fused AdamW on bf16 weights without an fp32 master: the "
        "update is computed in fp32 and rounded stochastically",
        py::arg("params"), py::arg("grads"), py::arg("exp_avgs"),
        py::arg("exp_avg_sqs"), py::arg("lrs"), py::arg("weight_decays"),
        py::arg("steps"), py::arg("streams"), py::arg("beta1"),
        py::arg("beta2"), py::arg("eps"), py::arg("grad_scale"),
        py::arg("norm_sq"), py::arg("max_norm"), py::arg("skip_nonfinite"),
        py::arg("seed"), py::arg("span_elems") = 0);
  m.def("multi_tensor_adamw_fp8_sr", &multi_tensor_adamw_fp8_sr,
        "multi_tensor_adamw_sr on FP8 block-scaled moments",
        py::arg("params"), py::arg("grads"), py::arg("exp_avgs"),
        py::arg("exp_avg_scales"), py::arg("exp_avg_sq_roots"),
        py::arg("exp_avg_sq_root_scales"), py::arg("lrs"),
        py::arg("weight_decays"), py::arg("steps"), py::arg("streams"),
        py::arg("beta1"), py::arg("beta2"), py::arg("eps"),
        py::arg("grad_scale"), py::arg("norm_sq"), py::arg("max_norm"),
        py::arg("skip_nonfinite"), py::arg("seed"),
        py::arg("span_elems") = 0);
  m.attr("CKPT_SPAN_QUANTUM") = ckpt_span_quantum();
  m.attr("CKPT_MAX_BLOCKS") = ckpt_max_blocks();
  m.def("fp8_amax_slots", &fp8_amax_slots,
        "int32 partial slots fp8_amax_scale needs for this tensor",
        py::arg("x"));
  m.def("fp8_amax_scale", &fp8_amax_scale,
        "scale[0] = absmax(x) / FMAX of the format (0 below FLT_MIN, NaN and "
        "inf propagate): two kernels over the partials workspace, no atomics",
        py::arg("x"), py::arg("fmt"), py::arg("partials"), py::arg("scale"));
  m.def("fp8_cast_transpose", &fp8_cast_transpose,
        "RNE(x / scale) as OCP fp8 codes, row-major and/or transposed, from "
        "one read of x",
        py::arg("x"), py::arg("scale"), py::arg("fmt"), py::arg("rowwise"),
        py::arg("colwise"));
  m.def("ckpt_auto_span", [](int64_t total) {
    return (int64_t)ckpt_auto_span((long long)total);
  }, "span in bytes that ckpt_copy_sum picks for a list of this total size");
  m.def("ckpt_sum_slots", &ckpt_sum_slots,
        "[slots, 2] int64 partial slots ckpt_copy_sum needs for these sizes",
        py::arg("nbytes_list"), py::arg("span_bytes") = 0);
  m.def("ckpt_copy_sum", &ckpt_copy_sum,
        "batched copy (0 pack, 1 unpack, 2 none) with per-tensor checksums "
        "-> sums[N,2] (int64, no atomics)",
        py::arg("mode"), py::arg("tensors"), py::arg("staging"),
        py::arg("offsets"), py::arg("partials"), py::arg("sums"),
        py::arg("span_bytes") = 0);
}
