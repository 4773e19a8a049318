"""The fused checkpoint pack / unpack / checksum kernel (ops/csrc/
ckpt_pack.hip) against the host reference, and the shm writer/reader with
device-side checksums. Integer equality everywhere: the checksum is modular
integer arithmetic, so there is no tolerance to speak of."""

import os
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

from dlrover_amd.ops.api import (  # noqa: E402
    ckpt_checksum,
    ckpt_checksum_ref,
    ckpt_pack,
    ckpt_sum_slots,
    ckpt_sums_to_ints,
    ckpt_unpack,
    hip_ops,
)


def _nbytes(t):
    return t.numel() * t.element_size()


def _bytes_of(t):
    """The tensor's bytes as a uint8 CPU tensor."""
    return t.detach().cpu().contiguous().reshape(-1).view(torch.uint8)


def _ref(tensors):
    return [ckpt_checksum_ref(_bytes_of(t)) for t in tensors]


def _u8(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=g)


def _mixed_tensors():
    """Every dtype, the alignment cases and a zero-numel tensor in the
    middle; all small."""
    q = hip_ops().CKPT_SPAN_QUANTUM
    g = torch.Generator(device="cuda").manual_seed(1)

    def rnd(n):
        return torch.randn(n, device="cuda", generator=g)

    bf_base = rnd(2 * q).bfloat16()
    return [
        rnd(1031).bfloat16(),                      # 2062 B: partial last word
        rnd(777),                                  # fp32
        torch.randint(-(1 << 62), 1 << 62, (131,), device="cuda", generator=g),
        _u8(4099, 2),
        rnd(515) > 0,                              # bool, 515 B
        torch.empty(0, device="cuda"),             # zero numel, mid-list
        bf_base[1:1001],                           # 2-byte-aligned source
        bf_base[1001 : 1001 + q // 2 + 3],         # same, more than one span
        torch.tensor(7, dtype=torch.int64, device="cuda"),  # 0-dim
        _u8(5, 3),
    ]


def test_checksum_kernel_bit_exact():
    ext = hip_ops()
    q, max_blocks = ext.CKPT_SPAN_QUANTUM, ext.CKPT_MAX_BLOCKS
    assert q == 512 * 16
    lengths = [1, 2, 3, 4, 15, 16, 17, 4096, q - 1, q, q + 1, q - 2, q + 2,
               2 * q, 3 * q + 7]
    tensors = [_u8(n, 10 + i) for i, n in enumerate(lengths)]
    tensors[7:7] = _mixed_tensors()
    # more than MAX_BLOCKS spans at span = q: continues across launches
    big = _u8(max_blocks * q + 3 * q + 5, 99)
    tensors.insert(3, big)
    # > 2 descriptor batches of 32 entries: 70 tensors and more
    tensors += [_u8(37 + 3 * i, 200 + i) for i in range(70 - len(tensors) + 5)]
    assert len(tensors) >= 70
    assert any(t.numel() == 0 for t in tensors[1:-1])
    assert any(t.data_ptr() % 4 == 2 for t in tensors)
    want = _ref(tensors)

    got = ckpt_sums_to_ints(ckpt_checksum(tensors, span_bytes=q))
    assert got == want
    # other partitions of the same words (automatic span, 2q): the same bits
    got_auto = ckpt_sums_to_ints(ckpt_checksum(tensors))
    assert got_auto == want
    got_2q = ckpt_sums_to_ints(ckpt_checksum(tensors, span_bytes=2 * q))
    assert got_2q == want
    # caller-owned workspaces, larger than needed and pre-filled with junk
    nb = [_nbytes(t) for t in tensors]
    slots = ckpt_sum_slots(nb, q)
    assert slots == sum((n + q - 1) // q for n in nb)
    partials = torch.full((slots + 3, 2), -1, dtype=torch.int64, device="cuda")
    sums = torch.full((len(tensors), 2), -1, dtype=torch.int64, device="cuda")
    out = ckpt_checksum(tensors, sums=sums, partials=partials, span_bytes=q)
    assert out.data_ptr() == sums.data_ptr()
    assert ckpt_sums_to_ints(sums) == want
    assert bool((partials[slots:] == -1).all())  # nothing past the last slot
    # a single flipped bit on the device shows
    big[len(big) // 2] ^= 0x40
    flipped = ckpt_sums_to_ints(ckpt_checksum([big], span_bytes=q))[0]
    assert flipped[0] != want[3][0] and flipped[1] != want[3][1]


def _layout(tensors, misalign=()):
    """64-byte-aligned offsets as plan_layout makes them; indices in
    `misalign` get an odd extra byte so the staging side is unaligned."""
    offsets, off = [], 0
    for i, t in enumerate(tensors):
        if i in misalign:
            off += 1 if _nbytes(t) % 2 else 2
        offsets.append(off)
        off += (_nbytes(t) + 63) // 64 * 64
    return offsets, off + 64


def test_pack_matches_copy():
    tensors = _mixed_tensors()
    offsets, total = _layout(tensors, misalign=(1, 4))
    staging = torch.full((total,), 0xFF, dtype=torch.uint8, device="cuda")
    want = _ref(tensors)
    sums = ckpt_pack(tensors, offsets, staging)
    assert ckpt_sums_to_ints(sums) == want
    host = staging.cpu()
    covered = torch.zeros(total, dtype=torch.bool)
    for t, off in zip(tensors, offsets):
        n = _nbytes(t)
        assert torch.equal(host[off : off + n], _bytes_of(t)), (off, n)
        covered[off : off + n] = True
    # not one byte outside the tensors' ranges was written
    assert bool((host[~covered] == 0xFF).all())
    # summing the staging ranges gives the same: the 0xFF padding next to a
    # partial last word is neither read nor counted
    ranges = [staging[off : off + _nbytes(t)] for t, off in zip(tensors, offsets)]
    assert ckpt_sums_to_ints(ckpt_checksum(ranges)) == want
    # a non-contiguous source is packed as its contiguous bytes
    nc = torch.randn(16, 24, device="cuda").t()
    s2 = ckpt_pack([nc], [0], staging)
    assert torch.equal(staging[: _nbytes(nc)].cpu(), _bytes_of(nc))
    assert ckpt_sums_to_ints(s2) == _ref([nc])
    with pytest.raises(RuntimeError):
        ckpt_pack([tensors[0]], [total - 8], staging)  # would overrun


def test_unpack_roundtrip():
    tensors = _mixed_tensors()
    offsets, total = _layout(tensors, misalign=(0, 3))
    staging = torch.full((total,), 0xFF, dtype=torch.uint8, device="cuda")
    want = _ref(tensors)
    saved = [_bytes_of(t) for t in tensors]
    ckpt_pack(tensors, offsets, staging)
    for t in tensors:
        if t.numel():
            t.reshape(-1).view(torch.uint8).zero_()
    assert all(int(_bytes_of(t).sum()) == 0 for t in tensors)
    sums = ckpt_unpack(staging, offsets, tensors)
    assert ckpt_sums_to_ints(sums) == want
    for t, b in zip(tensors, saved):
        assert torch.equal(_bytes_of(t), b)
    # the neighbours of the 2-byte-aligned destination view are untouched:
    # element 0 of its base lies right in front of it
    assert tensors[6].data_ptr() % 4 == 2


def test_pack_graph_safe():
    q = hip_ops().CKPT_SPAN_QUANTUM
    g = torch.Generator(device="cuda").manual_seed(5)
    tensors = [
        torch.randn(3 * q // 4 + 5, device="cuda", generator=g),
        torch.randn(1001, device="cuda", generator=g).bfloat16(),
        _u8(77, 6),
    ]
    offsets, total = _layout(tensors)
    staging = torch.zeros(total, dtype=torch.uint8, device="cuda")
    sums = torch.zeros((len(tensors), 2), dtype=torch.int64, device="cuda")
    slots = ckpt_sum_slots([_nbytes(t) for t in tensors])
    partials = torch.zeros((slots, 2), dtype=torch.int64, device="cuda")

    def pack():
        return ckpt_pack(tensors, offsets, staging, sums=sums, partials=partials)

    pack()  # eager first: loads the code object outside the capture
    torch.cuda.synchronize()
    assert ckpt_sums_to_ints(sums) == _ref(tensors)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # a single chain of launches
        pack()
    with torch.no_grad():
        tensors[0].mul_(-3.0).add_(1.0)
        tensors[1].add_(2.0)
        tensors[2].bitwise_xor_(0x5A)
    sums.zero_()
    graph.replay()
    torch.cuda.synchronize()
    want = _ref(tensors)
    assert ckpt_sums_to_ints(sums) == want
    host = staging.cpu()
    for t, off in zip(tensors, offsets):
        assert torch.equal(host[off : off + _nbytes(t)], _bytes_of(t))


# -- shm writer / reader -------------------------------------------------------


def _tiny_train_state():
    from dlrover_amd.models import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(0)
    model = LlamaForCausalLM(LlamaConfig.tiny()).to("cuda").bfloat16()
    params = {n: p.detach() for n, p in model.named_parameters()}
    g = torch.Generator(device="cuda").manual_seed(3)
    opt = {
        i: {
            "master_param": p.float(),
            "exp_avg": torch.randn(p.shape, device="cuda", generator=g),
            "exp_avg_sq": torch.rand(p.shape, device="cuda", generator=g),
            "step": torch.tensor(9, dtype=torch.int64),  # a CPU tensor
        }
        for i, p in enumerate(params.values())
    }
    return {"model": params, "optimizer": {"state": opt}, "step": 9}


def _payload_bytes(h, tm):
    start = h._payload_offset() + tm.offset
    return bytes(h._shm.buf[start : start + tm.nbytes])


@pytest.mark.parametrize("chunked", [False, True])
def test_device_save_restore_verified(chunked, monkeypatch):
    from dlrover_amd.trainer.flash_checkpoint.shm_handler import (
        CheckpointCorruptError,
        SharedMemoryHandler,
        _get_by_path,
    )

    if chunked:
        monkeypatch.setenv("DLROVER_CKPT_FORCE_CHUNKED", "1")
    else:
        monkeypatch.delenv("DLROVER_CKPT_FORCE_CHUNKED", raising=False)
    state = _tiny_train_state()
    h = SharedMemoryHandler(
        f"ckint_gpu_{os.getpid()}_{time.time_ns()}", checksum=True
    )
    try:
        h.save_state_dict(9, state, block=False)
        h.wait_drained()
        assert h._stager._chunked is chunked
        meta = h.read_meta()
        assert meta is not None and meta.step == 9
        for tm in meta.tensors:
            assert tm.checksum is not None, tm.path
            assert tuple(tm.checksum) == ckpt_checksum_ref(_payload_bytes(h, tm)), tm.path
        dev = torch.device("cuda")
        out = h.load_state_dict(device=dev)
        for tm in meta.tensors:
            a = _get_by_path(out, tm.path)
            b = _get_by_path(state, tm.path)
            assert a.is_cuda and torch.equal(a.cpu(), b.cpu()), tm.path
        victim = next(
            tm for tm in meta.tensors if tm.path[-1] == "exp_avg" and tm.nbytes > 4096
        )
        h._shm.buf[h._payload_offset() + victim.offset + 1234] ^= 0x04
        with pytest.raises(CheckpointCorruptError) as ei:
            h.load_state_dict(device=dev)
        assert ei.value.paths == [victim.path]
        assert ei.value.source == "shm"
        assert h.load_state_dict(device=dev, verify=False) is not None
        with pytest.raises(CheckpointCorruptError):
            h.load_state_dict()  # host-side verification sees it too
    finally:
        h.unlink()


def test_snapshot_bytes_identical_to_unfused():
    from dlrover_amd.trainer.flash_checkpoint.shm_handler import SharedMemoryHandler

    state = _tiny_train_state()
    # a non-contiguous and a 2-byte-aligned source go through the same paths
    state["extra"] = {
        "t": torch.randn(24, 40, device="cuda").t(),
        "odd": torch.randn(301, device="cuda").bfloat16()[1:],
    }
    tag = f"{os.getpid()}_{time.time_ns()}"
    h_on = SharedMemoryHandler(f"ckint_on_{tag}", checksum=True)
    h_off = SharedMemoryHandler(f"ckint_off_{tag}", checksum=False)
    try:
        h_on.save_state_dict(2, state)
        h_off.save_state_dict(2, state)
        m_on, m_off = h_on.read_meta(), h_off.read_meta()
        assert [(t.path, t.offset, t.nbytes) for t in m_on.tensors] == [
            (t.path, t.offset, t.nbytes) for t in m_off.tensors
        ]
        assert all(t.checksum is None for t in m_off.tensors)
        for a, b in zip(m_on.tensors, m_off.tensors):
            assert _payload_bytes(h_on, a) == _payload_bytes(h_off, b), a.path
    finally:
        h_on.unlink()
        h_off.unlink()


def test_restore_into_verified(tmp_path, monkeypatch):
    """restore_into with checksums on a GPU: device load + device-side
    verification + device-to-device copies; a corrupt shm snapshot falls
    through to storage; when the second copy would not fit the restore runs
    unverified through the zero-copy path."""
    from dlrover_amd.trainer.flash_checkpoint.engine import ShardedCheckpointEngine

    monkeypatch.setenv("ELASTIC_JOB_NAME", f"ckri{os.getpid()}_{time.time_ns()}")
    torch.manual_seed(0)
    model = torch.nn.Sequential(
        torch.nn.Linear(64, 96), torch.nn.Linear(96, 33)
    ).cuda().bfloat16()
    eng = ShardedCheckpointEngine(str(tmp_path / "ckpt"), checksum=True)
    calls = []
    real_load = eng.shm_handler.load_state_dict

    def spy_load(**kw):
        calls.append(kw)
        return real_load(**kw)

    storage_loads = []
    real_storage = eng.load_from_storage

    def spy_storage(*a, **kw):
        storage_loads.append(1)
        return real_storage(*a, **kw)

    monkeypatch.setattr(eng.shm_handler, "load_state_dict", spy_load)
    monkeypatch.setattr(eng, "load_from_storage", spy_storage)

    def scramble():
        with torch.no_grad():
            for p in model.parameters():
                p.add_(1.0)

    def assert_restored():
        for p, w in zip(model.parameters(), want):
            assert torch.equal(p.detach(), w)

    try:
        eng.save_to_storage(3, eng.gather_state_dict(model, None))
        eng.wait_saving()
        want = [p.detach().clone() for p in model.parameters()]
        assert (tmp_path / "ckpt" / "3" / "rank_00000.sums").exists()

        scramble()
        assert eng.restore_into(model, None) is not None
        assert_restored()
        assert calls[-1]["verify"] is True and calls[-1]["device"].type == "cuda"
        assert not calls[-1].get("zero_copy") and not storage_loads

        # one flipped bit in shm: the snapshot is skipped, storage serves
        h = eng.shm_handler
        tm = next(t for t in h.read_meta().tensors if t.path == ("model", "0.weight"))
        h._shm.buf[h._payload_offset() + tm.offset + 100] ^= 0x01
        scramble()
        assert eng.restore_into(model, None) is not None
        assert_restored()
        assert calls[-1]["verify"] is True and len(storage_loads) == 1

        # no room for the transient second copy: unverified zero-copy restore,
        # as without the option (the damaged byte comes back unnoticed)
        _, total = torch.cuda.mem_get_info()
        monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a: (0, total))
        scramble()
        assert eng.restore_into(model, None) is not None
        assert calls[-1]["zero_copy"] is True and calls[-1]["verify"] is False
        assert len(storage_loads) == 1
        got = [p.detach() for p in model.parameters()]
        assert not torch.equal(got[0], want[0])
        assert all(torch.equal(a, b) for a, b in zip(got[1:], want[1:]))
    finally:
        eng.close()
        eng.shm_handler.unlink()
