"""HIP/CDNA4 kernel wrappers.

Loading policy (the framework's hot path must actually run native code):
  - On a GPU box, every op REQUIRES the in-tree ``_hip_ops`` extension and
    raises ExtensionMissingError if it isn't built — no silent eager
    fallback on ROCm.
  - On CPU (this dev container, CPU tests), ops run a pure-torch fp32
    reference implementation. GPU numerics tests compare the HIP kernels
    against these same references.
"""

# Importing the submodule binds the name ``fp8_linear`` in this package to the
# module; the import from ``api`` below rebinds it to the function, which is
# what ``dlrover_amd.ops.fp8_linear`` means to callers. Keep this order.
from dlrover_amd.ops.fp8_linear import Fp8Linear  # noqa: F401
from dlrover_amd.ops.api import (  # noqa: F401
    ExtensionMissingError,
    causal_softmax,
    ce_shard_finish,
    ce_shard_stats,
    flash_attention,
    flash_attention_ref,
    flash_attention_supports_doc_mask,
    cross_entropy_loss,
    doc_end_from_start,
    doc_positions,
    doc_start_from_eos,
    doc_start_from_ids,
    fp8_block_dequantize,
    fp8_block_quantize,
    fp8_linear,
    fp8_linear_supported,
    fp8_quantize,
    fused_adamw_fp8_multi_step,
    fused_adamw_multi_step,
    fused_adamw_step,
    grad_sq_norm,
    hip_ops,
    hip_ops_available,
    rmsnorm,
    rmsnorm_add,
    rope_ref,
    rope_rotate,
    swiglu,
    validate_doc_start,
    vocab_parallel_cross_entropy,
)
from dlrover_amd.ops.adamw import FusedAdamW  # noqa: F401
