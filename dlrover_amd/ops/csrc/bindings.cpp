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
