"""The host half of the three persistent frame launches (csrc/persist.h: lm_depth.hip, lm_temporal.hip, codec_tr.hip) and their health
registry, without launching one of them: the grid the library answers for a shape against the launcher's arithmetic restated in
Python, the shapes it must refuse, the workspace sizes, and the retire / rearm cycle of `persistent_poll` driven by tensor writes
into the status words."""
import gc
import warnings

import pytest
import torch

from rstnet_amd import _lib, ops
from tests.test_codec_tr_shapes_gpu import STREAM_SHAPES
from tests.helpers import depth_frame_ref as DR
from tests.helpers import temporal_frame_ref as TR

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LDS_LIMIT = 150 * 1024
# (E, H, F, L, cap, B, T): the five shapes of test_codec_tr_shapes_gpu.py at the most positions one of their steps carries
CODEC_SHAPES = [(E, H, F, L, cap, B, max(chunks)) for E, H, F, L, cap, B, chunks in STREAM_SHAPES]


@pytest.fixture(autouse=True)
def frames_enabled(monkeypatch):
    monkeypatch.setenv("RST_DEPTH_FRAME", "1")


def _cus():
    return torch.cuda.get_device_properties(DEV).multi_processor_count


# ---- the library's answers, asked on DEV ------------------------------------------------------------------------------------------------
def _depth(c):
    with torch.cuda.device(DEV):
        return int(_lib.lib().rst_depth_frame_supported(c.B, c.E, c.H, c.Hd, c.card, c.Q, c.L, c.top_k if 0 < c.top_k < c.card else c.card))


def _temporal(c):
    with torch.cuda.device(DEV):
        return int(_lib.lib().rst_temporal_frame_supported(c.E, c.H, c.Hd, c.L, c.cap, int(c.kv == "bf16")))


def _codec(E, H, F, L, cap, B, T):
    with torch.cuda.device(DEV):
        return int(_lib.lib().rst_codec_transformer_supported(B, T, E, H, F, L, cap))


def _codec_grid(E, H, F, B, cus):
    """rst_codec_tr_grid: every workgroup (4 waves) owns a row of the in-projection (3E rows) and of linear1 (F rows), at most one
    workgroup per CU, and every (stream, head) pair needs a workgroup."""
    G = min(cus, max(1, -(-min(3 * E, F) // 4)))
    return G if B * H <= G else 0


def _codec_lds(E, H, F, cap, B, T):
    """ct_lds_bytes of csrc/codec_tr.hip, restated here because no reference helper holds it.  The dynamic LDS of codec_tr_kernel in bytes: header | xs [R][max(E, F)] | x [R][E] | q, k, v of one head [T][3 D] | two score rows
    per row of cap slots plus a batch of 16384 / D | the reduction scratch."""
    R, D = B * T, E // H
    return (DR.DF_HDR_FLOATS + R * max(E, F) + R * E + T * 3 * D + 2 * R * (cap + 16384 // D) + (1024 + 2 * DR.DF_WAVES) * R) * 4


# ---- grids --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in DR.CASES])
def test_depth_grid_is_the_models(name):
    c = DR.BY_NAME[name]
    g = DR.grid(c, _cus())
    want = g.G if g.ok else 0
    first = _depth(c)
    assert first == want, f"{name}: the library answers {first} workgroups, the model {want}"
    assert _depth(c) == first, "the cached answer differs from the first"
    for _ in range(2):
        assert ops.depth_frame_supported(c.B, c.E, c.H, c.Hd, c.card, c.Q, c.L, c.top_k, device=DEV) == (want > 0)


@pytest.mark.parametrize("name", [c.name for c in TR.CASES])
def test_temporal_grid_is_the_models(name):
    c = TR.BY_NAME[name]
    g = TR.grid(c, _cus())
    want = g.G if g.ok else 0
    first = _temporal(c)
    assert first == want, f"{name}: the library answers {first} workgroups, the model {want}"
    assert _temporal(c) == first, "the cached answer differs from the first"
    for _ in range(2):
        assert ops.temporal_frame_supported(1, c.E, c.H, c.Hd, c.L, c.cap, c.kv == "bf16", device=DEV) == (want > 0)


@pytest.mark.parametrize("shape", CODEC_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_codec_grid_is_the_models(shape):
    E, H, F, L, cap, B, T = shape
    assert _codec_lds(E, H, F, cap, B, T) <= LDS_LIMIT
    want = _codec_grid(E, H, F, B, _cus())          # min(cus, max(1, ceil(min(3E, F) / 4))) when B * H <= G, else 0
    first = _codec(*shape)
    assert first == want, f"{shape}: the library answers {first} workgroups, the model {want}"
    assert _codec(*shape) == first, "the cached answer differs from the first"
    for _ in range(2):
        assert ops.codec_transformer_frame_supported(B, T, E, H, F, L, cap, device=DEV) == (want > 0)


# ---- refusals: each next to a neighbour that is served, so that the named gate is the one that refuses ------------------------------------
def test_depth_refusals():
    base = DR.BY_NAME["rows-B2"]
    assert _depth(base) > 0
    assert _depth(base._replace(B=3, text=("ok",) * 3)) == 0
    assert not ops.depth_frame_supported(3, base.E, base.H, base.Hd, base.card, base.Q, base.L, base.top_k, device=DEV)
    assert _depth(base._replace(card=4096)) > 0
    assert _depth(base._replace(card=4097)) == 0
    # the LDS formula past 150 KiB: the widest FFN that fits, then 8 more columns
    c = DR.BY_NAME["hd3080-B1"]
    while DR.lds_bytes(c._replace(Hd=c.Hd + 8)) <= LDS_LIMIT:
        c = c._replace(Hd=c.Hd + 8)
    over = c._replace(Hd=c.Hd + 8)
    assert DR.lds_bytes(c) <= LDS_LIMIT < DR.lds_bytes(over)
    assert _depth(c) > 0 and _depth(over) == 0


def test_temporal_refusals():
    assert _temporal(TR.Case("d128", 384, 3, 264, 70, "f32", 2)) > 0
    assert _temporal(TR.Case("d96", 384, 4, 264, 70, "f32", 2)) == 0
    base = TR.BY_NAME["d64-f32"]
    assert _temporal(base._replace(L=40)) > 0
    assert _temporal(base._replace(L=41)) == 0
    assert not ops.temporal_frame_supported(1, base.E, base.H, base.Hd, 41, base.cap, False, device=DEV)
    c = base
    while TR.lds_bytes(c._replace(Hd=c.Hd + 8)) <= LDS_LIMIT:
        c = c._replace(Hd=c.Hd + 8)
    over = c._replace(Hd=c.Hd + 8)
    assert TR.lds_bytes(c) <= LDS_LIMIT < TR.lds_bytes(over)
    assert _temporal(c) > 0 and _temporal(over) == 0


def test_codec_refusals():
    E, H, F, L, cap, B, T = CODEC_SHAPES[-1]          # four streams of one position
    assert (B, T) == (4, 1) and _codec(E, H, F, L, cap, 4, 1) > 0
    assert _codec(E, H, F, L, cap, 5, 1) == 0          # B * T = 5
    assert not ops.codec_transformer_frame_supported(5, 1, E, H, F, L, cap, device=DEV)
    assert _codec(192, 12, 512, 2, 20, 1, 1) > 0       # D = 16
    assert _codec(192, 8, 512, 2, 20, 1, 1) == 0       # D = 24
    E, H, F, L, cap, B, T = CODEC_SHAPES[0]
    while _codec_lds(E, H, F, cap + 1, B, T) <= LDS_LIMIT:          # the longest ring whose score rows fit, then one more slot
        cap += 1
    assert _codec_lds(E, H, F, cap, B, T) <= LDS_LIMIT < _codec_lds(E, H, F, cap + 1, B, T)
    assert _codec(E, H, F, L, cap, B, T) > 0 and _codec(E, H, F, L, cap + 1, B, T) == 0


# ---- workspace sizes: two sets of 8-byte granules (persistent launch | repair launch) ----------------------------------------------------
def test_workspace_bytes():
    lib = _lib.lib()
    for c in DR.CASES:
        n = c.B * (5 * c.E + c.Hd + c.card + 1)          # depth_frame_ref.read_handoff
        hist = DR.MAX_L * DR.MAX_Q * c.B * 2 * c.E * 4          # the repair launch's KV history
        assert lib.rst_depth_frame_workspace_bytes(c.B, c.E, c.Hd, c.card) == 16 * n + hist, c.name
    for c in TR.CASES:
        n = 5 * c.E + c.Hd + c.H * TR.TF_MAX_SPLITS * (c.E // c.H + 2)          # temporal_frame_ref.read_handoff
        assert lib.rst_temporal_frame_workspace_bytes(c.E, c.Hd, c.H) == 16 * n, c.name
    for E, H, F, L, cap, B, T in CODEC_SHAPES:
        n = B * T * (5 * E + F)          # gX | gQKV | gATT [R][E ..] and gH [R][F]
        assert lib.rst_codec_transformer_workspace_bytes(B * T, E, F) == 16 * n


# ---- health -------------------------------------------------------------------------------------------------------------------------------
def _served():
    """A temporal and a codec shape the device serves while its persistent launches are enabled."""
    t, (E, H, F, L, cap, B, T) = TR.BY_NAME["d64-f32"], CODEC_SHAPES[0]
    return (ops.temporal_frame_supported(1, t.E, t.H, t.Hd, t.L, t.cap, False, device=DEV),
            ops.codec_transformer_frame_supported(B, T, E, H, F, L, cap, device=DEV))


def test_synchronous_poll_retires_and_rearm_gives_back():
    ops.persistent_rearm(DEV)
    try:
        st = ops.new_persistent_status(DEV)
        assert ops.depth_frame_enabled(DEV) and _served() == (True, True)
        e0 = ops.persistent_epoch(DEV)
        st[1] = 1
        with pytest.warns(RuntimeWarning, match="persistent frame launches retired"):
            ops.persistent_poll(DEV, synchronize=True)
        assert not ops.depth_frame_enabled(DEV) and ops.persistent_epoch(DEV) == e0 + 1 and _served() == (False, False)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            ops.persistent_poll(DEV, synchronize=True)          # silent, changes nothing
        assert not ops.depth_frame_enabled(DEV) and ops.persistent_epoch(DEV) == e0 + 1
        ops.persistent_rearm(DEV)
        assert ops.depth_frame_enabled(DEV) and ops.persistent_epoch(DEV) == e0 + 2 and _served() == (True, True)
        assert st.tolist() == [0, 0, 0, 0] and ops.persistent_repairs(DEV) == 0
    finally:
        ops.persistent_rearm(DEV)


def test_asynchronous_poll_retires_on_the_next_call():
    ops.persistent_rearm(DEV)
    try:
        st = ops.new_persistent_status(DEV)
        e0 = ops.persistent_epoch(DEV)
        st[1] = 2
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            ops.persistent_poll(DEV)          # requests the copy only
        assert ops.depth_frame_enabled(DEV) and ops.persistent_epoch(DEV) == e0
        torch.cuda.synchronize()
        with pytest.warns(RuntimeWarning, match="persistent frame launches retired"):
            ops.persistent_poll(DEV)
        assert not ops.depth_frame_enabled(DEV) and ops.persistent_epoch(DEV) == e0 + 1
        assert ops.persistent_repairs(DEV, synchronize=False) == 2
    finally:
        ops.persistent_rearm(DEV)
    assert ops.depth_frame_enabled(DEV) and st.tolist() == [0, 0, 0, 0]


def test_a_dropped_status_tensor_no_longer_counts():
    ops.persistent_rearm(DEV)
    try:
        st = ops.new_persistent_status(DEV)
        st[1] = 3
        assert ops.persistent_repairs(DEV) == 3
        del st
        gc.collect()
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            ops.persistent_poll(DEV)
        assert ops.persistent_repairs(DEV) == 0 and ops.depth_frame_enabled(DEV)
    finally:
        ops.persistent_rearm(DEV)


def test_poll_is_a_no_op_during_capture():
    ops.persistent_rearm(DEV)
    try:
        st = ops.new_persistent_status(DEV)
        e0 = ops.persistent_epoch(DEV)
        st[1] = 1
        buf = torch.zeros(8, device=DEV)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.device(DEV), torch.cuda.graph(graph):
            buf.add_(1)
            ops.persistent_poll(DEV, synchronize=True)
            ops.persistent_poll(DEV)
        assert ops.depth_frame_enabled(DEV) and ops.persistent_epoch(DEV) == e0
        st.zero_()
    finally:
        ops.persistent_rearm(DEV)
