"""FusedAdamW: bf16 training with fp32 master weights, one HIP kernel per
param, optionally replayed as a single hipGraph.

MI355X-native replacement for the fused Adam the reference delegates to
Megatron/Apex (BASELINE.json north star). Design:
  - model params stay bf16 (what forward/backward/collectives touch);
  - this optimizer owns fp32 master params + fp32 moments;
  - each step launches adamw_kernel once per param; the kernel updates
    master/m/v AND writes the bf16 param in the same pass;
  - with ``capture_graph=True`` the per-param launch sequence is captured
    into a hipGraph after the first step and replayed thereafter (launch
    overhead of ~300 small kernels -> 1 graph launch). Requires stable grad
    pointers (true under DDP bucket views and our Llama trainer).

State-dict format is torch-optimizer-compatible (state[param] has step /
exp_avg / exp_avg_sq / master_param) so flash checkpoint handles it like any
optimizer.

Opt-in batched path (``multi_tensor=True`` and/or ``max_grad_norm=...``):
  - the update runs as a few multi-tensor launches instead of one launch per
    parameter (ops/csrc/multi_tensor.hip);
  - with ``max_grad_norm`` the global gradient norm is computed on the device
    from all local gradients (two kernels, no atomics), optionally
    all-reduced, and the clip coefficient
    ``min(1, max_norm / (norm + 1e-6))`` — the definition of
    ``torch.nn.utils.clip_grad_norm_`` — is applied inside the update
    kernel. Gradients are read, never rewritten; there is no host sync
    anywhere in the step. ``opt.last_grad_norm`` is a 0-dim fp32 device
    tensor with the pre-clip global norm; reading it is the caller's sync;
  - a non-finite norm (inf/NaN gradient) with ``skip_nonfinite=True`` makes
    the update kernel return without storing: master weights, both moments
    and the bf16 weights stay bit-identical. The host cannot see that
    without a sync, so ``state["step"]`` still advances on a skipped step and
    bias correction drifts by one step per skip — the same approximation the
    graph path already makes. Skipping needs the norm, so it is only active
    together with ``max_grad_norm``.

Which ranks the norm is summed over: an explicit ``grad_norm_group`` always
wins. Without one, DTensor parameters (FSDP2) are reduced over their mesh's
group — all parameters must share one 1-D mesh and be ``Shard``-placed,
anything else raises NotImplementedError; plain tensors (single process, DDP
replicas) are not reduced. The TP/PP stack in ``dlrover_amd/parallel`` is out
of scope: it must pass ``grad_norm_group`` itself, and parameters replicated
across that group would be counted once per rank.

The new arguments live on the optimizer object, not in ``param_groups``, so
checkpoints keep their format.

Opt-in FP8 moments (``moments="fp8"``, implies the batched path): a parameter
with ``ndim >= 2`` and a last dim that is a multiple of 256 — decided from
the global shape, so every FSDP2 rank decides alike — keeps both moments as
OCP e4m3fn codes with one fp32 scale per 256 consecutive elements
(ops/csrc/adamw_fp8.hip). Its state is ``master_param`` (fp32), ``exp_avg``
(uint8 codes, the local parameter's shape), ``exp_avg_scale`` (fp32
``[rows..., cols/256]``), ``exp_avg_sq_root`` / ``exp_avg_sq_root_scale``
(the same for the SQUARE ROOT of the second moment) and ``step``: 6.03 bytes
per parameter instead of 12. Every tensor keeps the parameter's dim 0, so the
state reshards like any other. All other parameters keep fp32 moments on the
multi-tensor path. ``load_state_dict`` converts between the two formats, so
either kind of checkpoint loads into either kind of optimizer. A non-finite
gradient that is not caught by ``max_grad_norm`` poisons its whole 256-block
(through the block scale) instead of one element.
"""

import logging
from typing import Iterable, Optional

import torch

from dlrover_amd.ops.api import (
    FP8_BLOCK,
    fp8_block_dequantize,
    fp8_block_quantize,
    fused_adamw_fp8_multi_step,
    fused_adamw_multi_step,
    fused_adamw_step,
    grad_sq_norm,
    grad_sq_norm_slots,
)

logger = logging.getLogger(__name__)

try:
    from torch.distributed.tensor import DTensor
except ImportError:  # pragma: no cover
    DTensor = ()


def _local(t: torch.Tensor) -> torch.Tensor:
    """FSDP2 params/grads are DTensors; the kernel operates on the local
    shard (each rank owns its shard's optimizer state — ZeRO-3 style)."""
    if DTensor and isinstance(t, DTensor):
        return t.to_local()
    return t


class FusedAdamW(torch.optim.Optimizer):
    def __init__(
        self,
        params: Iterable[torch.nn.Parameter],
        lr: float = 1e-4,
        betas=(0.9, 0.95),
        eps: float = 1e-8,
        weight_decay: float = 0.1,
        capture_graph: bool = False,
        max_grad_norm: Optional[float] = None,
        multi_tensor: bool = False,
        skip_nonfinite: bool = True,
        grad_norm_group=None,
        moments: str = "fp32",
    ):
        if moments not in ("fp32", "fp8"):
            raise ValueError(f'moments must be "fp32" or "fp8", got {moments!r}')
        if max_grad_norm is not None and not max_grad_norm > 0:
            raise ValueError(f"max_grad_norm must be > 0, got {max_grad_norm}")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        self._capture_graph = capture_graph and torch.cuda.is_available()
        self._graph: Optional[torch.cuda.CUDAGraph] = None
        self._graph_ptrs = None
        self._lr_at_capture = None
        self.max_grad_norm = max_grad_norm
        self.skip_nonfinite = skip_nonfinite
        self.grad_norm_group = grad_norm_group
        self.moments = moments
        self._batched = (
            multi_tensor or max_grad_norm is not None or moments == "fp8"
        )
        # 0-dim fp32 tensor on the params' device: global pre-clip norm of
        # the last step (None until a clipped step has run)
        self.last_grad_norm: Optional[torch.Tensor] = None
        self._ws_key = None
        self._ws_partials = None
        self._ws_norm_sq = None
        self._span_elems = 0  # 0 = automatic
        self._span_elems_fp8 = 0  # same, a multiple of 256
        self._reduce_group_cache = None
        self._warned_no_capture = False

    def _init_state(self, p: torch.Tensor):
        state = self.state[p]
        state["step"] = 0
        master = _local(p.detach()).float().clone()
        state["master_param"] = master
        if self._fp8_eligible(p):
            scale_shape = (*master.shape[:-1], master.shape[-1] // FP8_BLOCK)
            for k in ("exp_avg", "exp_avg_sq_root"):
                state[k] = torch.zeros_like(master, dtype=torch.uint8)
                state[k + "_scale"] = master.new_zeros(scale_shape)
            return
        state["exp_avg"] = torch.zeros_like(master)
        state["exp_avg_sq"] = torch.zeros_like(master)

    def _fp8_eligible(self, p: torch.Tensor) -> bool:
        """FP8 moments for this parameter? From the GLOBAL shape only (a
        DTensor's ``shape``), so every rank of a Shard(0) placement decides
        alike, one that holds 0 rows included."""
        return (
            self.moments == "fp8"
            and p.ndim >= 2
            and p.shape[-1] % FP8_BLOCK == 0
        )

    def state_nbytes(self) -> int:
        """Bytes of all optimizer state tensors (the local shards)."""
        return sum(
            v.numel() * v.element_size()
            for st in self.state.values()
            for v in st.values()
            if torch.is_tensor(v)
        )

    def _one_step(self):
        for group in self.param_groups:
            beta1, beta2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                state = self.state[p]
                if "master_param" not in state:
                    self._init_state(p)
                state["step"] += 1
                is_bf16 = p.dtype == torch.bfloat16
                p_data = _local(p.data)
                fused_adamw_step(
                    state["master_param"],
                    _local(p.grad).contiguous(),
                    state["exp_avg"],
                    state["exp_avg_sq"],
                    p_data if is_bf16 else None,
                    group["lr"],
                    beta1,
                    beta2,
                    group["eps"],
                    group["weight_decay"],
                    state["step"],
                )
                if not is_bf16:
                    # fp32 params: master IS the param storage
                    p_data.copy_(state["master_param"])

    def _norm_reduce_group(self, params):
        """Process group the squared norm is summed over, or None."""
        if self.grad_norm_group is not None:
            return self.grad_norm_group
        if self._reduce_group_cache is not None:
            return self._reduce_group_cache[0]
        dts = [p for p in params if DTensor and isinstance(p, DTensor)]
        group = None
        if dts:
            mesh = dts[0].device_mesh
            ok = len(dts) == len(params) and mesh.ndim == 1
            for p in dts:
                ok = ok and p.device_mesh == mesh
                ok = ok and all(pl.is_shard() for pl in p.placements)
            if not ok:
                raise NotImplementedError(
                    "FusedAdamW(max_grad_norm=...): the global gradient norm "
                    "is only derived automatically when every parameter is a "
                    "DTensor sharded (Shard placement) over one common 1-D "
                    "device mesh, or none is a DTensor. Pass grad_norm_group "
                    "explicitly for any other layout."
                )
            group = mesh.get_group()
        self._reduce_group_cache = (group,)
        return group

    def _global_norm_sq(self, grads, params):
        dev = grads[0].device
        key = (tuple((g.numel(), g.dtype) for g in grads), dev, self._span_elems)
        if key != self._ws_key:
            # persistent workspace: reallocated only when the set of
            # gradient sizes changes
            slots = grad_sq_norm_slots(grads, self._span_elems)
            self._ws_partials = torch.empty(
                max(slots, 1), device=dev, dtype=torch.float32
            )
            self._ws_norm_sq = torch.zeros(1, device=dev, dtype=torch.float32)
            self.last_grad_norm = torch.zeros((), device=dev, dtype=torch.float32)
            self._ws_key = key
        grad_sq_norm(
            grads,
            out=self._ws_norm_sq,
            partials=self._ws_partials,
            span_elems=self._span_elems,
        )
        group = self._norm_reduce_group(params)
        if group is not None:
            torch.distributed.all_reduce(self._ws_norm_sq, group=group)
        torch.sqrt(self._ws_norm_sq[0], out=self.last_grad_norm)
        return self._ws_norm_sq

    def _mt_step(self):
        """Batched path: [global norm ->] one multi-tensor update per
        (param group, gradient dtype, moment format). No host sync."""
        if self.max_grad_norm is not None:
            # refuse an unsupported layout before any state is touched
            self._norm_reduce_group(
                [p for g in self.param_groups for p in g["params"]
                 if p.grad is not None]
            )
        batches, grads, params, fp32_copies = [], [], [], []
        for group in self.param_groups:
            by_dtype = {}
            for p in group["params"]:
                if p.grad is None:
                    continue
                state = self.state[p]
                if "master_param" not in state:
                    self._init_state(p)
                state["step"] += 1
                g = _local(p.grad).contiguous()
                p_data = _local(p.data)
                is_bf16 = p.dtype == torch.bfloat16
                fp8 = "exp_avg_sq_root" in state
                b = by_dtype.setdefault(
                    (g.dtype, fp8), ([], [], [], [], [], [], [], [])
                )
                b[0].append(state["master_param"])
                b[1].append(g)
                b[2].append(state["exp_avg"])
                b[3].append(state["exp_avg_sq_root" if fp8 else "exp_avg_sq"])
                b[4].append(p_data if is_bf16 else None)
                b[5].append(state["step"])
                if fp8:
                    b[6].append(state["exp_avg_scale"])
                    b[7].append(state["exp_avg_sq_root_scale"])
                grads.append(g)
                params.append(p)
                if not is_bf16:
                    fp32_copies.append((p_data, state["master_param"]))
            batches.extend((group, k[1], b) for k, b in by_dtype.items())
        if not grads:
            return
        norm_sq = None
        if self.max_grad_norm is not None:
            norm_sq = self._global_norm_sq(grads, params)
        for group, fp8, b in batches:
            n = len(b[0])
            if fp8:
                fused_adamw_fp8_multi_step(
                    b[0], b[1], b[2], b[6], b[3], b[7], b[4],
                    [group["lr"]] * n,
                    [group["weight_decay"]] * n,
                    b[5],
                    group["betas"][0],
                    group["betas"][1],
                    group["eps"],
                    1.0,
                    norm_sq,
                    self.max_grad_norm if norm_sq is not None else float("inf"),
                    self.skip_nonfinite,
                    self._span_elems_fp8,
                )
                continue
            fused_adamw_multi_step(
                b[0], b[1], b[2], b[3], b[4],
                [group["lr"]] * n,
                [group["weight_decay"]] * n,
                b[5],
                group["betas"][0],
                group["betas"][1],
                group["eps"],
                1.0,
                norm_sq,
                self.max_grad_norm if norm_sq is not None else float("inf"),
                self.skip_nonfinite,
                self._span_elems,
            )
        for p_data, master in fp32_copies:
            # fp32 params: master IS the param storage
            p_data.copy_(master)

    def _can_capture(self):
        if not self._capture_graph:
            return False
        if not self._batched or self.max_grad_norm is None:
            return True
        params = [
            p for g in self.param_groups for p in g["params"] if p.grad is not None
        ]
        if self._norm_reduce_group(params) is None:
            return True
        if not self._warned_no_capture:
            logger.warning(
                "FusedAdamW: capture_graph is ignored while the gradient "
                "norm is all-reduced over a process group; running eagerly"
            )
            self._warned_no_capture = True
        return False

    def _grad_ptrs(self):
        return tuple(
            p.grad.data_ptr()
            for g in self.param_groups
            for p in g["params"]
            if p.grad is not None
        )

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        one_step = self._mt_step if self._batched else self._one_step
        if not self._can_capture():
            one_step()
            return loss

        ptrs = self._grad_ptrs()
        lr = self.param_groups[0]["lr"]
        if self._graph is None or ptrs != self._graph_ptrs or lr != self._lr_at_capture:
            # warm-up step on a side stream, then capture the next one.
            # NOTE: `step` increments inside the graph are host-side, so the
            # kernel's bias correction uses a step snapshot; graphs are only
            # exact when bias correction has converged (step >> 1/(1-beta)).
            # We therefore run eagerly for the first 100 steps.
            min_step = min(
                (self.state[p].get("step", 0))
                for g in self.param_groups
                for p in g["params"]
                if p.grad is not None
            )
            if min_step < 100:
                one_step()
                return loss
            torch.cuda.synchronize()
            self._graph = torch.cuda.CUDAGraph()
            # capture records the kernels WITHOUT executing them — the
            # step counters bumped inside _one_step() then describe work
            # that has not run yet. Replay immediately (capture-then-replay)
            # so the capture iteration's gradients are actually applied.
            # the batched path captures the same way: the clip coefficient
            # is computed on the device, so every replay recomputes it
            with torch.cuda.graph(self._graph):
                one_step()
            self._graph.replay()
            self._graph_ptrs = ptrs
            self._lr_at_capture = lr
            return loss
        # replay path: bump host-side step counters to keep state dict honest
        for g in self.param_groups:
            for p in g["params"]:
                if p.grad is not None:
                    self.state[p]["step"] += 1
        self._graph.replay()
        return loss

    def load_state_dict(self, state_dict):
        """Override: torch's default casts every floating state tensor to the
        PARAM dtype — which would narrow our fp32 master weights to bf16.
        Restore state by position with device moves only."""
        groups = self.param_groups
        saved_groups = state_dict["param_groups"]
        params = [p for g in groups for p in g["params"]]
        saved_ids = [pid for g in saved_groups for pid in g["params"]]
        if len(params) != len(saved_ids):
            raise ValueError(
                f"optimizer param count mismatch: {len(params)} vs {len(saved_ids)}"
            )
        new_state = {}
        for sid, p in zip(saved_ids, params):
            if sid in state_dict["state"]:
                dev = _local(p).device
                cur = self.state.get(p, {})
                entry = {}
                saved = self._convert_moments(p, state_dict["state"][sid], dev)
                for k, v in saved.items():
                    if torch.is_tensor(v):
                        # copy INTO existing state storage when shapes match:
                        # a fresh .to(dev) would double-allocate ~96 GB of
                        # fp32 optimizer state mid-restore (OOM on 8B @ N=1)
                        old = cur.get(k)
                        if (
                            torch.is_tensor(old)
                            and old.shape == v.shape
                            and old.dtype == v.dtype
                            and old.device == dev
                        ):
                            old.copy_(v, non_blocking=True)
                            entry[k] = old
                        else:
                            entry[k] = v.to(dev)
                    else:
                        entry[k] = v
                new_state[p] = entry
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        self.state.clear()
        self.state.update(new_state)
        for g, sg in zip(groups, saved_groups):
            g.update({k: v for k, v in sg.items() if k != "params"})
        self._graph = None  # state tensors moved: any captured graph is stale

    def _convert_moments(self, p, saved: dict, dev) -> dict:
        """A saved state entry in the moment format this optimizer keeps for
        ``p``: fp32 moments are quantised (``exp_avg_sq`` through its square
        root), FP8 moments are dequantised (and the root squared). An entry
        that already has the right format is returned as it is."""
        has_fp8 = "exp_avg_sq_root" in saved
        want_fp8 = self._fp8_eligible(p)
        if has_fp8 == want_fp8 or "exp_avg" not in saved:
            return saved
        out = dict(saved)
        if want_fp8:
            m = out.pop("exp_avg").to(dev).float()
            root = out.pop("exp_avg_sq").to(dev).float().sqrt()
            out["exp_avg"], out["exp_avg_scale"] = fp8_block_quantize(m)
            out["exp_avg_sq_root"], out["exp_avg_sq_root_scale"] = (
                fp8_block_quantize(root)
            )
        else:
            out["exp_avg"] = fp8_block_dequantize(
                out.pop("exp_avg").to(dev), out.pop("exp_avg_scale").to(dev)
            )
            out["exp_avg_sq"] = fp8_block_dequantize(
                out.pop("exp_avg_sq_root").to(dev),
                out.pop("exp_avg_sq_root_scale").to(dev),
            ).square_()
        return out

    def zero_grad(self, set_to_none: bool = True):
        # torch semantics by default: dropping grads lets backward ASSIGN the
        # first accumulation instead of add_-ing into zeroed storage (measured
        # ~2% of an 8B step in fills + fan-in adds). Graph capture is the one
        # case that needs stable grad storage — zero in place there.
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is not None:
                    if set_to_none and not self._capture_graph:
                        p.grad = None
                    else:
                        p.grad.detach_()
                        p.grad.zero_()
