"""Flash-checkpoint engines: coordinate shm snapshots in the TRAINING process
and hand persistence to the agent's AsyncCheckpointSaver.

Parity target: ref dlrover/trainer/torch/flash_checkpoint/engine.py:60-560
(CheckpointEngine, readiness all-reduce, save_state_dict_to_memory,
save_to_storage event queue) and full_ckpt_engine.py / fsdp_engine.py.

Operating modes:
  - agent mode (default under dlrover-run): SharedLock/SharedQueue served by
    the elastic agent's IPCServer coordinate with AsyncCheckpointSaver;
  - standalone mode (no agent socket, e.g. bench.py / notebooks): an
    in-process saver thread provides the same behavior.
"""

import os
import threading
import time
from dataclasses import dataclass
from typing import Any, Optional

import torch
import torch.distributed as dist

from dlrover_amd.common.constants import CheckpointConstant
from dlrover_amd.common.log import logger
from dlrover_amd.common.multi_process import (
    SharedDict,
    SharedLock,
    SharedQueue,
    ipc_socket_path,
)
from dlrover_amd.common.storage import (
    PosixDiskStorage,
    read_tracker_step,
)
from dlrover_amd.trainer.flash_checkpoint.shm_handler import (
    CheckpointCorruptError,
    SharedMemoryHandler,
    DEVICE_COPY_HEADROOM,
    shm_segment_name,
    sums_file_name,
    traverse_state_dict,
)

CKPT_EVENT_QUEUE = "flash_ckpt_events"
CKPT_META_DICT = "flash_ckpt_meta"
CKPT_LOCK_PREFIX = "flash_ckpt_shm_"


@dataclass
class CheckpointEvent:
    SAVE = "SAVE"
    EXIT = "EXIT"
    type: str = SAVE
    step: int = 0
    path: str = ""
    local_rank: int = 0
    global_rank: int = 0
    world_size: int = 1
    expected_shards: int = 1


def checksum_from_env() -> bool:
    """DLROVER_CKPT_CHECKSUM=1 turns checkpoint checksums on for every engine
    that was not told otherwise (default: off)."""
    return os.getenv("DLROVER_CKPT_CHECKSUM", "0").lower() in ("1", "true", "on")


def _local_rank() -> int:
    # LOCAL_RANK when a launcher set it; otherwise fall back to the GLOBAL
    # rank — on a single host without a launcher every process would
    # otherwise claim shm segment _0 and the savers would race (observed:
    # two standalone savers persisting the same segment, one os.replace
    # losing the other's tmp file)
    lr = os.getenv("LOCAL_RANK")
    if lr is not None:
        return int(lr)
    return int(os.getenv("RANK", "0"))


def _global_rank() -> int:
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank()
    return int(os.getenv("RANK", "0"))


def _world_size() -> int:
    if dist.is_available() and dist.is_initialized():
        return dist.get_world_size()
    return int(os.getenv("WORLD_SIZE", "1"))


class CheckpointEngine:
    """Base engine: one shm segment per local rank.

    save_to_memory(step, state_dict)  -> blocking seconds (training stall)
    save_to_storage(step, state_dict, path) -> same + async persist event
    load(path=None) -> state_dict from shm (hit) or storage

    checksum: record a per-tensor checksum with every snapshot and verify it
    on every load (shm, replica, storage). None reads the environment
    variable DLROVER_CKPT_CHECKSUM; the default is off, and off changes
    nothing about the paths, files and formats.
    """

    def __init__(
        self,
        checkpoint_dir: str,
        storage=None,
        comm_backend: str = "",
        save_timeout: int = CheckpointConstant.SAVE_TIMEOUT,
        checksum: Optional[bool] = None,
    ):
        self.checkpoint_dir = checkpoint_dir
        self.storage = storage or PosixDiskStorage()
        self._save_timeout = save_timeout
        self._local_rank = _local_rank()
        self._job = os.getenv("ELASTIC_JOB_NAME", "default")
        self._checksum = checksum_from_env() if checksum is None else bool(checksum)
        self.shm_handler = SharedMemoryHandler(
            shm_segment_name(self._job, self._local_rank),
            checksum=self._checksum,
        )
        self._agent_mode = os.path.exists(ipc_socket_path())
        if self._agent_mode:
            self._shm_lock = SharedLock(f"{CKPT_LOCK_PREFIX}{self._local_rank}")
            self._event_queue = SharedQueue(CKPT_EVENT_QUEUE)
            self._meta_dict = SharedDict(CKPT_META_DICT)
            self._standalone_saver = None
        else:
            self._shm_lock = threading.Lock()
            self._event_queue = None
            self._meta_dict = None
            self._standalone_saver = _StandaloneSaver(self)
        # gloo side group for readiness checks (ref: engine.py:60-75); only
        # when a process group exists
        self._sync_group = None
        if dist.is_available() and dist.is_initialized():
            backend = comm_backend or "gloo"
            try:
                self._sync_group = dist.new_group(backend=backend)
            except (RuntimeError, ValueError):
                self._sync_group = None
        self._last_save_step = -1

    # -- readiness -------------------------------------------------------------

    def _check_all_ranks_ready(self, ready: bool) -> bool:
        """All-reduce a readiness flag so a rank that crashed mid-iteration
        can't leave peers writing inconsistent steps (ref: engine.py:60)."""
        if self._sync_group is None:
            return ready
        t = torch.tensor([0.0 if ready else 1.0])
        dist.all_reduce(t, group=self._sync_group)
        return t.item() == 0.0

    def _check_step_consistent(self, step: int) -> bool:
        if self._sync_group is None:
            return True
        ws = dist.get_world_size(self._sync_group)
        out = [torch.zeros(1, dtype=torch.long) for _ in range(ws)]
        dist.all_gather(out, torch.tensor([step], dtype=torch.long), group=self._sync_group)
        return all(int(o.item()) == step for o in out)

    # -- state-dict hooks (framework engines override) ---------------------------

    def gather_state_dict(self, model, optimizer) -> Any:
        raise NotImplementedError

    def load_into(self, model, optimizer, state_dict):
        raise NotImplementedError

    def rank_saves(self) -> bool:
        """Does THIS rank write a shard? (DDP full: rank0 only; FSDP: all)."""
        return True

    def expected_shards(self) -> int:
        """How many shard files make a COMPLETE checkpoint (commit gate)."""
        return _world_size()

    # -- save ------------------------------------------------------------------

    def save_to_memory(
        self, step: int, state_dict: Any, path: str = "", block: bool = True
    ) -> float:
        """Snapshot into shm. Returns blocking seconds."""
        if not self._check_step_consistent(step):
            raise RuntimeError(f"checkpoint step {step} differs across ranks")
        if not self._check_all_ranks_ready(True):
            logger.warning("skip checkpoint@%s: a peer rank is not ready", step)
            return 0.0
        blocking = 0.0
        if self.rank_saves():
            acquired = self._shm_lock.acquire(timeout=self._save_timeout) if isinstance(
                self._shm_lock, SharedLock
            ) else self._shm_lock.acquire(timeout=self._save_timeout)
            if not acquired:
                logger.warning("shm lock not acquired; skip checkpoint@%s", step)
                return 0.0
            try:
                extra = {
                    "path": path,
                    "global_rank": _global_rank(),
                    "world_size": _world_size(),
                    "shard_name": self._shard_file_name(_global_rank()),
                    # the commit gate for THIS snapshot — the agent's static
                    # max_nodes-derived count can exceed the live world and
                    # would block the failure-path commit forever
                    "expected_shards": self.expected_shards(),
                }
                blocking = self.shm_handler.save_state_dict(
                    step, state_dict, extra=extra, block=block
                )
            finally:
                self._shm_lock.release()
        self._last_save_step = step
        return blocking

    def save_to_storage(self, step: int, state_dict: Any, path: str = "") -> float:
        path = path or os.path.join(self.checkpoint_dir, str(step))
        blocking = self.save_to_memory(step, state_dict, path=path)
        event = CheckpointEvent(
            type=CheckpointEvent.SAVE,
            step=step,
            path=path,
            local_rank=self._local_rank,
            global_rank=_global_rank(),
            world_size=_world_size(),
            expected_shards=self.expected_shards(),
        )
        if self._event_queue is not None:
            if self.rank_saves():
                self._event_queue.put(event)
        elif self._standalone_saver is not None and self.rank_saves():
            self._standalone_saver.submit(event)
        return blocking

    # -- load ------------------------------------------------------------------

    def _load_from_shm(self, handler: SharedMemoryHandler, **kw) -> Optional[Any]:
        """handler.load_state_dict, except that a snapshot that fails its
        checksums counts as a miss: the error is logged with the offending
        tensors and the caller falls through to its next source. Nothing but
        CheckpointCorruptError is caught."""
        try:
            return handler.load_state_dict(**kw)
        except CheckpointCorruptError as e:
            logger.error(
                "shm snapshot %s is corrupt, falling back to storage: %s",
                handler.name, e,
            )
            return None

    def load(self, path: str = "", device: Optional[torch.device] = None) -> Optional[Any]:
        """shm hit first (ref: engine.py load :534), else storage. A shm
        snapshot that fails its checksums is skipped like a miss."""
        sd = self._load_from_shm(self.shm_handler, device=device)
        if sd is not None:
            return sd
        return self.load_from_storage(path, device=device)

    def load_from_storage(
        self, path: str = "", device: Optional[torch.device] = None
    ) -> Optional[Any]:
        if not path:
            step = read_tracker_step(self.checkpoint_dir)
            if step < 0:
                return None
            path = os.path.join(self.checkpoint_dir, str(step))
        shard = os.path.join(path, self._shard_file_name(_global_rank()))
        if not os.path.exists(shard):
            return None
        sd = torch.load(shard, map_location=device or "cpu", weights_only=False)
        self._verify_loaded_shard(sd, shard)
        return sd

    def _verify_loaded_shard(self, state_dict: Any, shard_file: str):
        """Check a state dict loaded from `shard_file` against its checksum
        sidecar. No sidecar (old checkpoints, checksums off at save time) or
        checksums disabled on this engine: no verification. GPU tensors are
        summed by one batched kernel call, CPU tensors by the host reference.
        Raises CheckpointCorruptError(source="storage")."""
        if not self._checksum:
            return
        sidecar = sums_file_name(shard_file)
        if not os.path.exists(sidecar):
            return
        import pickle

        with open(sidecar, "rb") as f:
            recorded = pickle.load(f)
        from dlrover_amd.ops.api import (
            ckpt_checksum,
            ckpt_checksum_ref,
            ckpt_sums_to_ints,
        )

        leaves = {
            tuple(p): v
            for p, v in traverse_state_dict(state_dict)
            if isinstance(v, torch.Tensor)
        }
        bad = [p for p in recorded if tuple(p) not in leaves]
        on_gpu = [(p, leaves[tuple(p)]) for p in recorded
                  if tuple(p) in leaves and leaves[tuple(p)].is_cuda]
        on_cpu = [(p, leaves[tuple(p)]) for p in recorded
                  if tuple(p) in leaves and not leaves[tuple(p)].is_cuda]
        for p, t in on_cpu:
            if ckpt_checksum_ref(t) != tuple(recorded[p]):
                bad.append(p)
        if on_gpu:
            got = ckpt_sums_to_ints(ckpt_checksum([t for _, t in on_gpu]))
            bad += [p for (p, _), have in zip(on_gpu, got)
                    if have != tuple(recorded[p])]
        if bad:
            raise CheckpointCorruptError(bad, source="storage")

    @staticmethod
    def _shard_file_name(global_rank: int) -> str:
        return f"rank_{global_rank:05d}.pt"

    def latest_step(self) -> int:
        """Max of shm step and storage tracker step."""
        return max(self.shm_handler.committed_step(), read_tracker_step(self.checkpoint_dir))

    def wait_saving(self):
        """Block until async persist (if any) finished."""
        self.shm_handler.wait_drained()
        if self._standalone_saver is not None:
            self._standalone_saver.wait_idle()

    def close(self):
        if self._standalone_saver is not None:
            self._standalone_saver.stop()
        self.shm_handler.close()


class _StandaloneSaver:
    """In-process persistence thread for agent-less runs. Mirrors the agent's
    AsyncCheckpointSaver commit protocol (done files + tracker)."""

    def __init__(self, engine: CheckpointEngine):
        self._engine = engine
        self._queue: "list[CheckpointEvent]" = []
        self._cv = threading.Condition()
        self._stop = False
        self._busy = False
        self._thread = threading.Thread(target=self._run, daemon=True)
        self._thread.start()

    def submit(self, event: CheckpointEvent):
        with self._cv:
            self._queue.append(event)
            self._cv.notify()

    def wait_idle(self):
        while True:
            with self._cv:
                if not self._queue and not self._busy:
                    return
            time.sleep(0.02)

    def stop(self):
        with self._cv:
            self._stop = True
            self._cv.notify()
        self._thread.join(timeout=10)

    def _run(self):
        from dlrover_amd.agent.ckpt_saver import persist_shm_to_storage

        while True:
            with self._cv:
                while not self._queue and not self._stop:
                    self._cv.wait(timeout=1.0)
                if self._stop and not self._queue:
                    return
                event = self._queue.pop(0)
                self._busy = True
            try:
                self._engine.shm_handler.wait_drained()
                persist_shm_to_storage(
                    self._engine.shm_handler,
                    event,
                    self._engine.storage,
                    self._engine.checkpoint_dir,
                    expected_shards=getattr(event, "expected_shards", 1) or 1,
                )
            except Exception:  # noqa: BLE001
                logger.exception("standalone checkpoint persist failed")
            finally:
                with self._cv:
                    self._busy = False


class FullCheckpointEngine(CheckpointEngine):
    """DDP-style: the model/optimizer state is replicated, so only global
    rank 0 snapshots and persists (ref: full_ckpt_engine.py:33)."""

    def rank_saves(self) -> bool:
        return _global_rank() == 0

    def expected_shards(self) -> int:
        return 1

    @staticmethod
    def _shard_file_name(global_rank: int) -> str:
        # the full checkpoint is always rank 0's shard — every rank reads it
        return "rank_00000.pt"

    def load(self, path: str = "", device=None):
        """Full-checkpoint load order: own shm, local rank 0's shm (the full
        state lives there on this node), then storage. All ranks MUST resolve
        the same step or DDP ranks would resume divergent and deadlock."""
        sd = self._load_from_shm(self.shm_handler, device=device)
        if sd is None and self._local_rank != 0:
            h0 = SharedMemoryHandler(
                shm_segment_name(self._job, 0), host_pin=False,
                checksum=self._checksum,
            )
            if h0.attach():
                sd = self._load_from_shm(h0, device=device)
                h0.close()
        if sd is None:
            sd = self.load_from_storage(path, device=device)
        return sd

    def gather_state_dict(self, model, optimizer):
        mod = model.module if hasattr(model, "module") else model
        sd = {"model": mod.state_dict(), "step": self._last_save_step}
        if optimizer is not None:
            sd["optimizer"] = optimizer.state_dict()
        return sd

    def load_into(self, model, optimizer, state_dict):
        mod = model.module if hasattr(model, "module") else model
        mod.load_state_dict(state_dict["model"])
        if optimizer is not None and "optimizer" in state_dict:
            optimizer.load_state_dict(state_dict["optimizer"])


class ShardedCheckpointEngine(CheckpointEngine):
    """FSDP-style: every rank snapshots its own local shards
    (ref: fsdp_engine.py:447 — ours iterates params/buffers directly and
    stores DTensor LOCAL shards, instead of DCP StorageWriter plumbing:
    the shm writer then D2H-copies live param storage with zero staging
    surprises, and restore is an in-place copy into the same storage.
    Same-world-size restore only; cross-world resharding is the UCP hook)."""

    def rank_saves(self) -> bool:
        return True

    @staticmethod
    def _named_tensors(model):
        import itertools

        return itertools.chain(model.named_parameters(), model.named_buffers())

    @staticmethod
    def _derived_param_names(model, optimizer) -> dict:
        """bf16 params whose exact value is RE-DERIVABLE from the optimizer's
        fp32 master copy (FusedAdamW writes param = bf16(master) every step):
        storing them in the snapshot is 16 GB of pure redundancy on the 8B
        model — ~15% of checkpoint size, drain time and restore seconds.
        Returns {param_name: flat_param_index}."""
        import os

        if optimizer is None or os.getenv("DLROVER_CKPT_DERIVED", "1") == "0":
            return {}
        state = getattr(optimizer, "state", None)
        if not isinstance(state, dict):
            return {}
        id2name = {id(p): n for n, p in model.named_parameters()}
        out = {}
        idx = 0
        for group in getattr(optimizer, "param_groups", []):
            for p in group["params"]:
                st = state.get(p)
                if (
                    st
                    and "master_param" in st
                    and p.dtype == torch.bfloat16
                    and id(p) in id2name
                ):
                    out[id2name[id(p)]] = idx
                idx += 1
        return out

    def gather_state_dict(self, model, optimizer):
        try:
            from torch.distributed.tensor import DTensor
        except ImportError:  # pragma: no cover
            DTensor = ()
        derived = self._derived_param_names(model, optimizer)
        model_sd = {}
        tags = {}
        for name, t in self._named_tensors(model):
            tags[name] = (
                "shard0" if DTensor and isinstance(t, DTensor) else "replicated"
            )
            if name in derived:
                continue  # re-derived from the fp32 master on restore
            model_sd[name] = _to_local(t.detach())
        opt_sd = _localize(optimizer.state_dict()) if optimizer is not None else {}
        return {
            "model": model_sd,
            "optimizer": opt_sd,
            "_sharding": tags,
            "_derived": derived,
            "world_size": _world_size(),
        }

    def load_into(self, model, optimizer, state_dict):
        live = dict(self._named_tensors(model))
        with torch.no_grad():
            for name, saved in state_dict["model"].items():
                if name not in live:
                    logger.warning("checkpoint key %s not in model — skipped", name)
                    continue
                dst = _to_local(live[name].data)
                # direct copy into live storage; from a page-locked shm view
                # this is one async H2D per tensor at PCIe rate
                dst.copy_(saved, non_blocking=True)
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        if optimizer is not None and state_dict.get("optimizer"):
            optimizer.load_state_dict(state_dict["optimizer"])
        self._rederive_params(model, optimizer, state_dict)

    @staticmethod
    def _rederive_params(model, optimizer, state_dict):
        """Params omitted from the snapshot (gather tagged them _derived)
        are reconstructed on DEVICE from the restored fp32 master — an
        HBM-local cast instead of 16 GB over PCIe."""
        derived = state_dict.get("_derived") or {}
        if not derived or optimizer is None:
            return
        params = [p for g in optimizer.param_groups for p in g["params"]]
        name2p = dict(model.named_parameters())
        with torch.no_grad():
            for name, idx in derived.items():
                if name not in name2p or idx >= len(params):
                    continue
                st = optimizer.state.get(params[idx])
                if not st or "master_param" not in st:
                    logger.warning("derived param %s has no master in the "
                                   "restored optimizer state", name)
                    continue
                dst = _to_local(name2p[name].data)
                dst.copy_(st["master_param"].to(dst.dtype))

    def _verified_device_restore_fits(self) -> bool:
        """Should restore_into take the device-verified path, and can it?"""
        if not (self._checksum and torch.cuda.is_available()):
            return False
        meta = self.shm_handler.read_meta()
        if meta is None or not any(
            getattr(tm, "checksum", None) is not None for tm in meta.tensors
        ):
            return False
        free, _total = torch.cuda.mem_get_info()
        if meta.payload_bytes + DEVICE_COPY_HEADROOM < free:
            return True
        logger.warning(
            "verified restore needs a transient %.1f GB device copy but only "
            "%.1f GB are free: restoring UNVERIFIED from shm",
            meta.payload_bytes / (1 << 30), free / (1 << 30),
        )
        return False

    def restore_into(self, model, optimizer, path: str = ""):
        """Fast-path restore: zero-copy shm views -> async H2D into the live
        param/optimizer storage. Returns the loaded state dict skeleton or
        None when neither shm nor storage has a checkpoint.

        With checksums enabled on a GPU the shm snapshot is instead loaded
        to the device, verified there by the checksum kernel, and copied
        device-to-device into the live storage. That holds a transient
        SECOND copy of the state in HBM; when it would not fit (with the
        stager's 24 GiB headroom) a warning is logged and the restore runs
        unverified through the zero-copy path. A snapshot that fails its
        checksums is skipped and the restore continues from storage."""
        if self._verified_device_restore_fits():
            sd = self._load_from_shm(
                self.shm_handler, device=torch.device("cuda"), verify=True
            )
        else:
            # on a GPU this is the unverified fast path; without one the
            # handler's default applies (host verification when enabled)
            verify = False if torch.cuda.is_available() else None
            sd = self._load_from_shm(
                self.shm_handler, zero_copy=True, verify=verify
            )
        if sd is None:
            sd = self.load_from_storage(path)
        if sd is None:
            return None
        self.load_into(model, optimizer, sd)
        # drop the zero-copy views: live references into shm.buf would make
        # the mapping unclosable (BufferError: exported pointers exist)
        return _map_leaves(sd, lambda v: None if isinstance(v, torch.Tensor) else v)


def _to_local(t):
    try:
        from torch.distributed.tensor import DTensor
    except ImportError:  # pragma: no cover
        return t
    return t.to_local() if isinstance(t, DTensor) else t


def _localize(obj):
    """Replace DTensors with their local shards for shm serialization."""
    return _map_leaves(obj, _to_local)


def _map_leaves(obj, fn):
    if isinstance(obj, dict):
        return {k: _map_leaves(v, fn) for k, v in obj.items()}
    if isinstance(obj, list):
        return [_map_leaves(v, fn) for v in obj]
    if isinstance(obj, tuple):
        return tuple(_map_leaves(v, fn) for v in obj)
    return fn(obj)
