"""The full elastic stack ON MI355X hardware: dlrover-run standalone spawns
the local master + elastic agent + a worker training nanoGPT over RCCL on
cuda:0 with flash checkpointing, then the same with an injected SIGKILL —
the agent must restart the worker, re-form the RCCL process group, and the
worker must resume from the shm/disk checkpoint (BASELINE.json configs #1/#2
semantics exercised on the real device)."""

import pytest

from tests.test_elastic_e2e import _read_progress, _run_cli

pytestmark = pytest.mark.gpu


def _job_name():
    import uuid

    return f"e2eg{uuid.uuid4().hex[:6]}"


@pytest.mark.timeout(540)
def test_nanogpt_rccl_clean_run_gpu(tmp_path):
    proc, progress, ckpt_dir = _run_cli(tmp_path, steps=8, ckpt_interval=4,
                                        nproc=1)
    assert proc.returncode == 0, (
        f"stdout:\n{proc.stdout[-3000:]}\nstderr:\n{proc.stderr[-5000:]}"
    )
    rows = _read_progress(progress)
    assert rows and rows[-1]["step"] == 8
    assert rows[-1]["device"].startswith("cuda"), rows[-1]
    from dlrover_amd.common.storage import read_tracker_step

    assert read_tracker_step(str(ckpt_dir)) == 8


@pytest.mark.timeout(540)
def test_nanogpt_rccl_sigkill_recovery_gpu(tmp_path):
    proc, progress, ckpt_dir = _run_cli(
        tmp_path, steps=12, ckpt_interval=3, nproc=1,
        extra_env={"DLROVER_TEST_KILL_AT_STEP": "7"},
    )
    assert proc.returncode == 0, (
        f"stdout:\n{proc.stdout[-3000:]}\nstderr:\n{proc.stderr[-5000:]}"
    )
    rows = _read_progress(progress)
    assert rows and rows[-1]["step"] == 12
    incarnations = {r.get("incarnation", 0) for r in rows}
    assert 1 in incarnations, f"no restart observed: {rows}"
    # the restarted worker resumed from the last committed step, not step 0
    resumed = [r for r in rows if r.get("incarnation") == 1]
    assert resumed and resumed[0].get("resumed_from", 0) >= 3, resumed[:2]


@pytest.mark.timeout(540)
def test_nanogpt_hiptimer_metrics_gpu(tmp_path):
    """--hiptimer preloads libhiptimer into the RCCL worker; the per-rank
    Prometheus file must show real kernel launches, per-communicator
    traffic, and hang=0 (config #5's detection plumbing, live on HW)."""
    import glob
    import os

    from dlrover_amd import xpu_timer

    # own job name: only this run's metrics dir is read, never another
    # job's (or another user's) leftovers under the same parent
    job = _job_name()
    proc, progress, ckpt_dir = _run_cli(
        tmp_path, steps=6, ckpt_interval=3, nproc=1,
        # HIPTIMER_SAMPLE=1 times every launch: with the default 1-in-32
        # sampling a 6-step tiny model may never have a GEMM land on a
        # sampled slot, and per-shape rows only exist for timed GEMMs
        extra_env={"DLROVER_HIPTIMER": "1", "HIPTIMER_DUMP_INTERVAL": "1",
                   "HIPTIMER_SAMPLE": "1", "ELASTIC_JOB_NAME": job},
    )
    assert proc.returncode == 0, (
        f"stdout:\n{proc.stdout[-3000:]}\nstderr:\n{proc.stderr[-5000:]}"
    )
    # the agent derives the metrics dir from the job name it generated; the
    # preloaded worker dumps every HIPTIMER_DUMP_INTERVAL (5 s), so poll
    # briefly for a file that already reflects the trained steps
    import time

    deadline = time.time() + 20
    last = {}
    while time.time() < deadline:
        candidates = glob.glob(f"/tmp/hiptimer_{job}/hiptimer_0.prom")
        for path in sorted(candidates, key=os.path.getmtime, reverse=True):
            m = xpu_timer.parse_metrics_file(path)
            last = m or last
            comm_keys = [k for k in m if k.startswith("hiptimer_comm_calls")]
            if (m.get("hiptimer_launched_total", 0) > 100
                    and m.get("XPU_TIMER_COMMON_HANG") == 0 and comm_keys):
                # round-2 depth: per-GEMM TFLOPS attribution and honest
                # collective busbw must be exported
                assert "hiptimer_gemm_tflops" in m, sorted(m)[:40]
                assert "hiptimer_comm_busbw_gbs" in m, sorted(m)[:40]
                if m.get('hiptimer_op_count{cat="gemm"}', 0) > 0:
                    # shapes only exist when the GEMMs actually route via
                    # hipblasLt (fp32 models may use plain rocBLAS)
                    gemm_shapes = [k for k in m if "gemm_m" in k]
                    assert gemm_shapes, sorted(m)[-40:]
                return
        time.sleep(1.0)
    raise AssertionError(f"no satisfying hiptimer metrics; last parsed: {last}")


@pytest.mark.timeout(540)
def test_hiptimer_timeline_dump_gpu(tmp_path):
    """Flag-file-triggered kernel-trace ring dump loads as chrome trace
    (perfetto-compatible; ref manager.h:50-62 + gen_trace_timeline)."""
    import glob
    import json
    import os
    import time

    job = _job_name()
    proc, progress, ckpt_dir = _run_cli(
        tmp_path, steps=25, ckpt_interval=30, nproc=1,
        extra_env={
            "ELASTIC_JOB_NAME": job,
            "DLROVER_HIPTIMER": "1",
            "HIPTIMER_DUMP_INTERVAL": "1",
            "DLROVER_TEST_TIMELINE_FLAG": "1",
            "HIPTIMER_SAMPLE": "1",
        },
    )
    assert proc.returncode == 0, proc.stderr[-4000:]
    # the worker (train_nanogpt) touches the dump flag mid-run when
    # DLROVER_TEST_TIMELINE_FLAG is set; find the dumped timeline
    deadline = time.time() + 15
    while time.time() < deadline:
        for path in glob.glob(f"/tmp/hiptimer_{job}/timeline_*.json"):
            data = json.load(open(path))
            evs = data.get("traceEvents", [])
            if len(evs) > 20:
                assert {"name", "ph", "ts", "dur"} <= set(evs[0])
                return
        time.sleep(1.0)
    raise AssertionError("no timeline dump found")
