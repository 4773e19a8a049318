import os
import tempfile

import pytest


def _shorten_temp_root():
    """AF_UNIX socket paths are capped at ~107 bytes, and the tests put their
    IPC sockets under tmp_path / tempfile dirs (<root>/pytest-of-U/pytest-N/
    <test>/ipc/<job>/ipc.sock is already ~90 bytes past the root). A deeply
    nested TMPDIR overflows that, so fall back to /tmp when the configured
    temp root is long. Set through TMPDIR so spawned agents/workers agree."""
    if len(tempfile.gettempdir()) <= 16:
        return
    if os.path.isdir("/tmp") and os.access("/tmp", os.W_OK | os.X_OK):
        os.environ["TMPDIR"] = "/tmp"
        tempfile.tempdir = None  # re-read TMPDIR on next gettempdir()


_shorten_temp_root()


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: test requires an MI355X (run on a GPU box)")


def pytest_collection_modifyitems(config, items):
    """Auto-skip gpu tests when no device is present, so `pytest tests` works
    everywhere; the driver still selects with -m gpu / -m 'not gpu'."""
    try:
        import torch

        has_gpu = torch.cuda.is_available()
    except Exception:  # noqa: BLE001
        has_gpu = False
    if has_gpu:
        return
    skip = pytest.mark.skip(reason="no GPU in this container")
    for item in items:
        if "gpu" in item.keywords:
            item.add_marker(skip)


@pytest.fixture(autouse=True)
def _isolate_ipc_dir(tmp_path, monkeypatch):
    """Each test gets its own IPC socket dir and job name."""
    monkeypatch.setenv("DLROVER_IPC_SOCKET_DIR", str(tmp_path / "ipc"))
    yield
