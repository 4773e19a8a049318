"""``nn.Linear`` whose three GEMMs take FP8 operands (``ops.fp8_linear``)."""

import torch
import torch.nn as nn

from dlrover_amd.ops.api import fp8_linear


class Fp8Linear(nn.Linear):
    """Drop-in ``nn.Linear``: the same parameters under the same names
    (``weight``, ``bias``) in the same dtype, so state dicts, flash
    checkpoints, FSDP sharding and the optimizer's fp32 masters are those of
    the bf16 model. Only the GEMM operands are 8-bit: input and weight as
    e4m3, the output gradient as ``grad_format``, each with one current
    absmax scale. The saved input is its transposed e4m3 codes, 1 byte per
    element instead of 2."""

    def __init__(self, in_features: int, out_features: int, bias: bool = True,
                 device=None, dtype=None, grad_format: str = "e5m2"):
        super().__init__(in_features, out_features, bias=bias, device=device,
                         dtype=dtype)
        self.grad_format = grad_format

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return fp8_linear(x, self.weight, self.bias, self.grad_format)

    def extra_repr(self) -> str:
        return f"{super().extra_repr()}, grad_format={self.grad_format}"
