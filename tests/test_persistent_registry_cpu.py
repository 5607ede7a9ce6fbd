"""rstnet_amd/persistent.py without a GPU: what `ops` re-exports, that the registry stands on torch alone, and the answers for a device
nothing was ever registered on.  (The retire / rearm cycle needs device words: tests/test_persistent_host_gpu.py.)"""
import ast

import torch

from rstnet_amd import ops, persistent

NAMES = ("new_persistent_status", "persistent_epoch", "persistent_repairs", "persistent_rearm", "persistent_poll", "persistent_retired",
         "depth_frame_enabled")


def test_ops_re_exports_the_registry():
    for name in NAMES:
        assert getattr(ops, name) is getattr(persistent, name), name
    assert not hasattr(ops, "PERSISTENT_MAX_REPAIRS") and persistent.PERSISTENT_MAX_REPAIRS == 0
    assert ops.TEMPORAL_FRAME == "auto" and ops.TEMPORAL_FRAME_AUTO_POS == 2048          # assigned through `ops.` by tests and tools


def test_the_registry_imports_torch_only():
    with open(persistent.__file__) as f:
        tree = ast.parse(f.read())
    for node in ast.walk(tree):
        assert not (isinstance(node, ast.ImportFrom) and node.level > 0), "persistent.py imports from the package"
        if isinstance(node, (ast.Import, ast.ImportFrom)):
            assert node in tree.body, "an import inside a function"


def test_a_device_without_history(monkeypatch):
    dev = torch.device("cuda", 63)          # never touched: nothing here needs the device to exist
    assert persistent.persistent_retired(dev) is None and persistent.persistent_epoch(dev) == 0
    assert persistent.persistent_repairs(dev, synchronize=False) == 0
    monkeypatch.setenv("RST_DEPTH_FRAME", "1")
    assert persistent.depth_frame_enabled(dev) and persistent.depth_frame_enabled()
    monkeypatch.setenv("RST_DEPTH_FRAME", "0")
    assert not persistent.depth_frame_enabled(dev) and not persistent.depth_frame_enabled()
    persistent.persistent_poll(torch.device("cpu"))          # not a GPU: nothing to look at

