"""CPU checks of the weight-only MXFP4 skinny GEMM: the host restatement of its packed operand (tests/helpers/skinny_mxfp4w.py), the
exactness of the decode it relies on, the routing of ``ops._skinny_stored`` (launches replaced by recorders), the ``batched`` keyword of
``LMModel.quantize_weights_`` on stand-in copies, the three C-ABI entries, and the inputs of the GPU test's fp64 bound."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from rstnet_amd import _lib, ops, synth
from rstnet_amd.lm import model as M
from tests.helpers import lm_mxfp4 as Q4
from tests.helpers import skinny_fp8w as S8
from tests.helpers import skinny_mxfp4w as S
from tests.helpers.gemv_bounds import p_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the packed layout --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,interleave", [(33, 64, False), (64, 96, False), (64, 96, True), (96, 32, True)])
def test_code_offsets_are_a_bijection(N, K, interleave):
    off = S.code_offsets(N, K)
    n32 = S.rows32(N)
    assert off.shape == (n32, K // 2)
    assert np.array_equal(np.sort(off.ravel()), np.arange(n32 * K // 2)), "every byte of rows32(N) * K/2 is written exactly once"
    # a lane's 8 bytes: the 4 code bytes of 8 consecutive k of step 2p, then of the same octet of step 2p + 1; 64 lanes = 512 contiguous bytes
    for r, k in [(0, 0), (n32 - 1, K - 32), (17, 8)]:
        base = off[r, k // 2]
        assert base % 8 == 0
        assert np.array_equal(off[r, k // 2:k // 2 + 4], base + np.arange(4)) and np.array_equal(off[r, k // 2 + 8:k // 2 + 12], base + 4 + np.arange(4))
        assert base // 8 % 64 == 32 * ((k // 8) % 2) + r % 32
        assert base // 512 == (r // 32) * (K // 32) + k // 32, "a wave-level load is the pair's 512 bytes"
    so = S.scale_offsets(N, K)
    assert np.array_equal(np.sort(so.ravel()), np.arange(n32 * K // 32))
    live = S.src_rows(N, interleave)
    assert np.array_equal(np.sort(live[live >= 0]), np.arange(N)), "every source row lands in exactly one packed row"


def test_the_layout_is_the_fp8_operands_at_half_the_bytes():
    """Code byte (r, k / 2) sits at half the offset of fp8 byte (r, k) (k even): same tile / pair / lane order."""
    N, K = 96, 128
    assert np.array_equal(S.code_offsets(N, K), S8.packed_offsets(N, K)[:, 0::2] // 2)


def test_nibble_order_survives_packing():
    """Even k stays in the low nibble: unpacking the packed bytes in k order gives the stored bytes back, so codes_of reads the same codes."""
    N, K = 40, 96
    g = torch.Generator().manual_seed(2)
    q = torch.randint(0, 256, (N, K // 2), generator=g, dtype=torch.int32).to(torch.uint8)
    s = torch.randint(2, 246, (N, K // 32), generator=g, dtype=torch.int32).to(torch.uint8)
    qp, sp = S.pack_weight_ref(q, s)
    codes, sb = S.unpack_ref(qp, sp, N, K)
    assert torch.equal(codes[:N], q) and torch.equal(Q4.codes_of(codes[:N]), Q4.codes_of(q))
    assert not codes[N:].any(), "pad rows are zero codes"
    assert torch.equal(sb[:N], s) and bool((sb[N:] == S.PAD_SCALE).all()), "pad rows carry the scale byte 127"
    off = S.code_offsets(N, K)
    k = 37                                    # odd k: the high nibble of byte k / 2
    assert (int(qp[off[5, k // 2]]) >> 4) == int(Q4.codes_of(q)[5, k]) and (int(qp[off[5, (k - 1) // 2]]) & 15) == int(Q4.codes_of(q)[5, k - 1])


def test_every_lane_load_reads_the_scale_of_its_own_block():
    """Packed (row r, pair p): the 8 bytes at lane 32 h + r % 32 (h = 0, 1) of pair p hold k = 32 p + 8 h + 0..7 and 32 p + 16 + 8 h + 0..7 --
    all inside block p -- and the byte the lane loads next to them, sp[(tile * K/32 + p) * 32 + r % 32], is scale[r][p]."""
    N, K = 70, 160
    g = torch.Generator().manual_seed(3)
    q = torch.randint(0, 256, (N, K // 2), generator=g, dtype=torch.int32).to(torch.uint8)
    s = (torch.arange(N)[:, None] * 7 + torch.arange(K // 32)[None, :] * 3 + 2).remainder(244).add(2).to(torch.uint8)
    assert len({(int(a), int(b)) for a, b in zip(s[:, 0], s[:, 1])}) == N
    qp, sp = S.pack_weight_ref(q, s)
    for r in (0, 31, 32, 69):
        for p in range(K // 32):
            for h in (0, 1):
                at = (((r // 32) * (K // 32) + p) * 64 + 32 * h + r % 32) * 8
                want = torch.cat([q[r, (32 * p + 8 * h) // 2:(32 * p + 8 * h) // 2 + 4], q[r, (32 * p + 16 + 8 * h) // 2:(32 * p + 16 + 8 * h) // 2 + 4]])
                assert torch.equal(qp[at:at + 8], want)
                assert int(sp[((r // 32) * (K // 32) + p) * 32 + r % 32]) == int(s[r, p])


@pytest.mark.parametrize("N,K", [(64, 64), (160, 32)])
def test_interleave_permutes_codes_and_scales_alike(N, K):
    g = torch.Generator().manual_seed(N + K)
    q = torch.randint(0, 256, (N, K // 2), generator=g, dtype=torch.int32).to(torch.uint8)
    s = torch.randint(2, 246, (N, K // 32), generator=g, dtype=torch.int32).to(torch.uint8)
    codes, sb = S.unpack_ref(*S.pack_weight_ref(q, s, interleave=True), N, K)
    for t in range(N // 32):
        u, v = slice(16 * t, 16 * t + 16), slice(N // 2 + 16 * t, N // 2 + 16 * t + 16)
        assert torch.equal(codes[32 * t:32 * t + 16], q[u]) and torch.equal(codes[32 * t + 16:32 * t + 32], q[v]), f"tile {t}: u rows, then the matching v rows"
        assert torch.equal(sb[32 * t:32 * t + 16], s[u]) and torch.equal(sb[32 * t + 16:32 * t + 32], s[v])


def test_decode_is_exact_for_every_code_and_scale_byte():
    """code * 2^e for scale bytes 2 .. 245: two significant bits, between 2^-126 and 6 * 2^118 -- a normal bf16 number, so the upper half
    of the fp32 the scaled convert yields is the value itself."""
    q, s = S.exhaustive_codes(32)
    v = Q4.dequant_ref(q, s)
    assert v.shape == (244, 32) and Q4.is_exactly_bf16(v)
    nz = v[v != 0].abs()
    assert float(nz.min()) == 2.0 ** -126 and float(nz.max()) == 6 * 2.0 ** 118
    assert not (v.float().view(torch.int32) & 0xFFFF).any(), "nothing below the bf16 half of the fp32 pattern"
    assert torch.equal(ops.dequantize_blocks_mxfp4(q, s).double(), v)
    q2, s2 = S.exhaustive_codes(64, block=1)
    assert bool((s2[:, 0] != s2[:, 1]).all()) and torch.equal(Q4.dequant_ref(q2, s2)[:, 32:], v)


# ---- routing --------------------------------------------------------------------------------------------------------------------------------
class _Launches:
    def __init__(self, monkeypatch):
        self.log = []
        for name in ("gemm_skinny", "gemm_skinny_fp8w", "gemm_skinny_mxfp4w"):
            monkeypatch.setattr(ops, name, lambda x, *a, _n=name, **kw: self.log.append((_n, x.shape[0], tuple(a[0].shape))) or _n)


def _copies(N, K):
    w = torch.zeros(N, K, dtype=torch.bfloat16)
    q4, s4 = torch.zeros(N, K // 2, dtype=torch.uint8), torch.zeros(N, max(K // 32, 1), dtype=torch.uint8)
    return w, q4, s4


def test_skinny_stored_routes_by_the_type_of_the_copy(monkeypatch):
    rec = _Launches(monkeypatch)
    w, q4, s4 = _copies(96, 512)
    x = torch.zeros(8, 512)
    assert ops._skinny_stored(x, w, ops.Mxfp4Copy(q4, s4)) == "gemm_skinny", "a plain Mxfp4Copy keeps the bf16 route"
    assert ops._skinny_stored(x, w, ops.Mxfp4BatchedCopy(q4, s4)) == "gemm_skinny_mxfp4w"
    assert ops._skinny_stored(x, w, (torch.zeros(96, 512, dtype=torch.uint8), torch.ones(96))) == "gemm_skinny_fp8w", "an fp8 pair routes as before"
    assert ops._skinny_stored(x, w, None) == "gemm_skinny"
    assert rec.log == [("gemm_skinny", 8, (96, 512)), ("gemm_skinny_mxfp4w", 8, (96, 256)), ("gemm_skinny_fp8w", 8, (96, 512)),
                       ("gemm_skinny", 8, (96, 512))]
    c = ops.Mxfp4BatchedCopy(q4, s4)
    assert isinstance(c, ops.Mxfp4Copy) and len(c) == 2 and c._fields == ("q", "scale") and c.q is q4 and c.scale is s4


def test_opted_in_copies_of_unserved_shapes_do_not_reach_the_new_launch(monkeypatch):
    rec = _Launches(monkeypatch)
    w, q4, s4 = _copies(96, 272)                        # K % 32 != 0
    assert ops._skinny_stored(torch.zeros(8, 272), w, ops.Mxfp4BatchedCopy(q4, s4)) == "gemm_skinny"
    w, q4, s4 = _copies(96, 512)                        # B > 64: lm_linear chunks, a direct call takes bf16
    assert ops._skinny_stored(torch.zeros(65, 512), w, ops.Mxfp4BatchedCopy(q4, s4)) == "gemm_skinny"
    assert [n for n, *_ in rec.log] == ["gemm_skinny", "gemm_skinny"]


def test_lm_linear_chunks_rows_above_64_onto_the_new_launch(monkeypatch):
    log = []
    monkeypatch.setattr(ops, "gemm_skinny_mxfp4w", lambda x, q, s, **kw: log.append(x.shape[0]) or torch.zeros(x.shape[0], q.shape[0]))
    monkeypatch.setattr(ops, "gemm_skinny", lambda *a, **kw: pytest.fail("the bf16 route was taken"))
    w, q4, s4 = _copies(96, 512)
    y = ops.lm_linear(torch.zeros(70, 512), w, w8=ops.Mxfp4BatchedCopy(q4, s4))
    assert log == [64, 6] and y.shape == (70, 96)


# ---- the keyword ----------------------------------------------------------------------------------------------------------------------------
def _standin_model():
    """LM_TINY on the CPU with stand-in copies of the shapes the device quantisers return (tests/test_temporal_pass_cpu.py::_lm)."""
    cfg = dict(synth.LM_TINY)
    model = M.LMModel.from_state_dict(synth.lm_state_dict(cfg, 3), cfg)
    as4 = {(id(m), n) for m, n in model._layer_weights()}
    for mod, name in model._covered_weights():
        N, K = getattr(mod, name).shape
        if (id(mod), name) in as4:
            M._attach_copy(mod, name, "4", torch.zeros(N, K // 2, dtype=torch.uint8), torch.zeros(N, K // 32, dtype=torch.uint8))
        else:
            M._attach_copy(mod, name, "8", torch.zeros(N, K, dtype=torch.uint8), torch.zeros(N, dtype=torch.float32))
    model.weight_dtype = model.transformer.weight_dtype = "mxfp4"
    return model


def _copy_types(model):
    return {type(lin.w8) for view in model.transformer._views() for lin in (view.qkv, view.out, view.fc, view.proj)}


def test_batched_keyword_switches_the_route_on_without_requantising():
    model = _standin_model()
    assert model.mxfp4_batched is False and _copy_types(model) == {ops.Mxfp4Copy}
    before = [(m, n, getattr(m, n + "_q4"), getattr(m, n + "_s4")) for m, n in model._layer_weights()]
    assert model.quantize_weights_("mxfp4") is model and model.mxfp4_batched is False and _copy_types(model) == {ops.Mxfp4Copy}
    assert model.quantize_weights_("mxfp4", batched=True) is model
    assert model.mxfp4_batched is True and model.transformer.mxfp4_batched is True and model.weight_dtype == "mxfp4"
    assert _copy_types(model) == {ops.Mxfp4BatchedCopy}
    assert all(getattr(m, n + "_q4") is q and getattr(m, n + "_s4") is s for m, n, q, s in before), "the stored copies are the same tensors"
    model.quantize_weights_("mxfp4", batched=True)          # idempotent
    assert model.mxfp4_batched is True and _copy_types(model) == {ops.Mxfp4BatchedCopy}
    assert type(M._w8(model.text_linear)) is tuple, "the heads stay fp8 pairs"


def test_batched_keyword_is_refused_for_fp8_and_bf16():
    cfg = dict(synth.LM_TINY)
    model = M.LMModel.from_state_dict(synth.lm_state_dict(cfg, 3), cfg)
    with pytest.raises(ValueError, match="already serve every batch size"):
        model.quantize_weights_("fp8", batched=True)
    with pytest.raises(ValueError):
        model.quantize_weights_("bf16", batched=True)
    assert model.weight_dtype == "bf16" and model.mxfp4_batched is False


def test_server_flag():
    src = open(os.path.join(ROOT, "rstnet_amd", "server.py")).read()
    assert '"--lm-mxfp4-batched"' in src and "lm_mxfp4_batched" in src


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------------------
def _header():
    text = open(os.path.join(ROOT, "include", "rstnet_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


@pytest.mark.parametrize("name,n_args", [("rst_skinny_pack_weight_mxfp4w", 8), ("rst_gemm_skinny_mxfp4w_supported", 3),
                                         ("rst_gemm_skinny_mxfp4w_f32", 15)])
def test_abi_entries(name, n_args):
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, _header(), flags=re.S)
    assert m, f"{name} is not declared in include/rstnet_hip.h"
    assert len([a for a in m.group(1).split(",") if a.strip()]) == n_args
    assert len(_lib.SIGNATURES[name]) == n_args
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, name)
    lib.rst_version.restype = ctypes.c_int
    assert lib.rst_version() >= 125


def test_supported_predicate():
    ok = ops.gemm_skinny_mxfp4w_supported
    assert ok(3, 1001, 1024) and ok(1, 5, 32) and ok(64, 4096, 8192) and ok(32, 22528, 4096) and ok(33, 4096, 11264) and ok(8, 50, 704)
    assert not ok(8, 64, 272) and not ok(8, 64, 16) and not ok(65, 64, 1024) and not ok(0, 64, 1024) and not ok(8, 0, 1024)


# ---- the inputs of the GPU test's bound -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,K,mode,res,bias", S.BOUND_CASES)
def test_the_bound_cases_stay_in_the_normal_range(B, N, K, mode, res, bias):
    """The fp64 reference of every case is finite and no output's magnitude sum falls below 2^-110, except the all-zero weight row
    without res / bias (magnitude 0, held to exact zeros): the relative bound needs no underflow floor."""
    x, alpha, r, b, w = S.bound_inputs(B, N, K, mode, res, bias)
    q, s = Q4.quant_blocks_ref(w)
    assert not q[1].any() and int(s.min()) >= 2 and len(set(s.flatten().tolist())) > 20
    w64 = Q4.dequant_ref(q, s)
    P = p_ref(x.double(), K, mode, alpha.double())
    ref = P @ w64.t() + (b.double() if bias else 0) + (r.double() if res else 0)
    mag = P.abs() @ w64.abs().t() + (b.double().abs() if bias else 0) + (r.double().abs() if res else 0)
    assert bool(torch.isfinite(ref).all()) and float(ref.abs().max()) < 2.0 ** 120
    live = torch.ones(N, dtype=torch.bool)
    if not (res or bias):
        assert not mag[:, 1].any()
        live[1] = False
    assert float(mag[:, live].min()) >= 2.0 ** -110, float(mag[:, live].min())
