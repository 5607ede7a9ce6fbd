"""Host side of the GPT multi-position pass (no GPU): the window and route rules as pure functions, the frequency table against the
oracle's rope cache, the ``kv_dtype`` plumbing and the C-ABI entries of the grouped-KV prefill."""
import os
import re

import pytest
import torch

from oracle import gpt_oracle as Gp
from rstnet_amd import _lib, ops, synth
from rstnet_amd.lm import gpt as G
from rstnet_amd.lm.generate import GPTGen
from rstnet_amd.lm.model import PREFILL_CHUNK, StreamingTransformer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16 = torch.float32, torch.bfloat16
NEW_SYMBOLS = {"rst_lm_attn_prefill_gqa_workspace_bytes": 6, "rst_lm_attn_prefill_gqa_f32": 21, "rst_lm_ring_append_gqa": 17}


@pytest.mark.parametrize("context,cap,want", [(10, 10, 9), (10, 11, 10), (3000, 3001, 3000), (3000, 3000, 2999), (100, 128, 100),
                                              (10, 7, 6), (None, 7, 6), (96, 65, 64)])
def test_window_is_what_single_steps_see(context, cap, want):
    assert G.prefill_window(context, cap) == want
    if context is not None:      # the rule of the Moshi-style transformer
        tr = StreamingTransformer(64, 1, 0, 64, context, "none")
        assert tr.window(cap) == want


ROUTES = [  # cap, pos, T, dtype, route
    (10, 0, 6, F32, G.ROUTE_APPEND_FIRST), (10, 3, 6, F32, G.ROUTE_APPEND_FIRST),
    (10, 4, 6, F32, G.ROUTE_PREFILL),       # fills the ring exactly: appending first would hide position 0 from every query of the chunk (Q1)
    (10, 5, 6, F32, G.ROUTE_PREFILL), (10, 8, 6, F32, G.ROUTE_PREFILL), (10, 23, 2, F32, G.ROUTE_PREFILL),
    (11, 12, 6, F32, G.ROUTE_PREFILL), (3001, 0, 256, F32, G.ROUTE_APPEND_FIRST), (3001, 2900, 256, F32, G.ROUTE_PREFILL),
    (96, 0, 6, BF16, G.ROUTE_PREFILL), (96, 90, 20, BF16, G.ROUTE_PREFILL), (3001, 0, 256, BF16, G.ROUTE_PREFILL)]


@pytest.mark.parametrize("cap,pos,T,dtype,route", ROUTES)
def test_route_chooser(cap, pos, T, dtype, route):
    assert G.prefill_route(cap, pos, T, dtype) == route


def test_chunk_plan():
    A, P = G.ROUTE_APPEND_FIRST, G.ROUTE_PREFILL
    assert PREFILL_CHUNK == 256
    # a call that is right today stays ONE pass, whatever its length
    assert G.prefill_chunks(3001, 0, 1024, F32, 256) == [(0, 1024, A)]
    assert G.prefill_chunks(10, 0, 6, F32, 256) == [(0, 6, A)]
    # otherwise chunks of min(chunk, cap), each with its own route
    assert G.prefill_chunks(10, 8, 6, F32, 256) == [(0, 6, P)]
    assert G.prefill_chunks(10, 0, 25, F32, 256) == [(0, 10, P), (10, 10, P), (20, 5, P)]
    assert G.prefill_chunks(10, 0, 9, F32, 256) == [(0, 9, A)] and G.prefill_chunks(10, 0, 10, F32, 256) == [(0, 10, P)]
    assert G.prefill_chunks(32, 40, 21, F32, 8) == [(0, 8, P), (8, 8, P), (16, 5, P)]
    assert G.prefill_chunks(3001, 0, 600, BF16, 256) == [(0, 256, P), (256, 256, P), (512, 88, P)]
    for cap, pos, T, dt, chunk in [(10, 3, 40, F32, 256), (96, 90, 20, BF16, 8), (11, 12, 6, F32, 4)]:
        plan = G.prefill_chunks(cap, pos, T, dt, chunk)
        assert [t0 for t0, _, _ in plan] == [sum(n for _, n, _ in plan[:i]) for i in range(len(plan))]
        assert sum(n for _, n, _ in plan) == T and all(n <= cap for _, n, _ in plan)
        assert all(r == G.prefill_route(cap, pos + t0, n, dt) for t0, n, r in plan)


@pytest.mark.parametrize("base,n", [(10000, 32), (10000, 64), (1000000, 64), (1000000, 128)])
def test_frequency_table_is_the_oracles(base, n):
    """The table handed to the kernels IS the angle of position 1 in ``build_rope_cache`` (the kernels multiply it by the position
    in fp32, as the outer product there does)."""
    tab = ops.gpt_rope_freqs(torch.device("cpu"), float(base), n)
    cos, sin = Gp.build_rope_cache(4, n, base)
    assert tab.dtype == torch.float32 and tab.shape == (n // 2,)
    assert torch.equal(torch.cos(tab), cos[1, :n // 2]) and torch.equal(torch.sin(tab), sin[1, :n // 2])
    assert torch.equal(torch.cos(tab * 3.0), cos[3, :n // 2])
    assert ops.gpt_rope_freqs(torch.device("cpu"), float(base), n) is tab      # once per (device, base, n)


def _model(**kw):
    cfg_d = dict(synth.GPT_TINY_GQA)
    return G.GPT.from_state_dict(synth.gpt_state_dict(cfg_d, 1), G.Config.from_dict(cfg_d), **kw), cfg_d


def test_kv_dtype_plumbing():
    model, cfg_d = _model()
    assert model.kv_dtype == F32 and model.transformer.kv_dtype == F32
    st = model.transformer._make_state(2, 10)
    assert st.k[0].dtype == F32 and st.k[0].shape == (2, cfg_d["n_query_groups"], 10, 64)
    model, cfg_d = _model(kv_dtype=BF16)
    assert model.kv_dtype == BF16
    st = model.transformer._make_state(2, 96)
    assert all(t.dtype == BF16 and t.shape == (2, cfg_d["n_query_groups"], 96, 64) for t in st.k + st.v) and st.scratch is not None
    assert model.transformer._make_state(2, 10, kv_dtype=F32).k[0].dtype == F32          # the argument overrides the model's
    with pytest.raises(ValueError, match="short-ring decode kernel"):
        model.transformer._make_state(2, 64)
    assert model.transformer._make_state(2, 65).v[1].dtype == BF16
    with pytest.raises(ValueError, match="short-ring decode kernel"):                   # context = 10
        with model.streaming(1):
            pass
    with pytest.raises(ValueError, match="float32 or torch.bfloat16"):
        _model(kv_dtype=torch.float16)
    with pytest.raises(ValueError, match="float32 or torch.bfloat16"):
        model.transformer._make_state(2, 96, kv_dtype=torch.float16)
    model, _ = _model(merge_lora=False, kv_dtype=BF16)
    assert model.kv_dtype == BF16


def test_gptgen_begin_takes_a_kv_dtype():
    model, cfg_d = _model()
    gen = GPTGen(model, use_sampling=False)
    with pytest.raises(ValueError, match="short-ring decode kernel"):                   # the ring of context + 1 = 11 slots
        gen.begin(1, kv_dtype=BF16)
    assert model.transformer._streaming_state is None and gen._saved is None


def _header():
    text = open(os.path.join(ROOT, "include", "rstnet_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_new_symbols_in_header_and_ctypes_table():
    text = _header()
    for name, n_args in NEW_SYMBOLS.items():
        m = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, text, flags=re.S)
        assert m, f"{name} not declared in include/rstnet_hip.h"
        assert len([a for a in m.group(1).split(",") if a.strip()]) == n_args
        assert len(_lib.SIGNATURES[name]) == n_args
    # the existing entry points keep their signatures
    assert len(_lib.SIGNATURES["rst_lm_attn_prefill_f32"]) == 20 and len(_lib.SIGNATURES["rst_lm_ring_append"]) == 16
    assert len(_lib.SIGNATURES["rst_lm_attn_prefill_workspace_bytes"]) == 5


def test_run_asks_for_the_launches_of_its_route(monkeypatch):
    """The host logic of ``run`` on CPU tensors, with recording stand-ins for the launches: which attention launches a chunk asks for, on
    which rows, with which window / heads / frequency table, and that the host counter follows."""
    from tests.helpers.ops_recorder import OpsRecorder
    rec = OpsRecorder().install(monkeypatch, ops)
    f32 = lambda *shape: torch.zeros(*shape, dtype=torch.float32)      # noqa: E731
    extra = {
        "lm_rope_append": lambda a: f32(a["qkv"].shape[0], a["heads"], a["qkv"].shape[1], a["k_cache"].shape[3]),
        "attention": lambda a: f32(a["q"].shape[0], a["q"].shape[2], a["q"].shape[1] * a["q"].shape[3]),
        "lm_attn_prefill": lambda a: f32(a["qkv"].shape[0] * a["qkv"].shape[1], a["heads"] * a["k_cache"].shape[3]),
        "lm_ring_append": lambda a: None,
        "rmsnorm": lambda a: f32(*a["x"].shape),
        "lm_rope_table": lambda a: f32(a["D"] // 2, 2),
    }
    for name, out in extra.items():
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *args, _n=name, _r=real, _o=out, **kw: _o(rec._record(_n, _r, args, kw)))
    monkeypatch.setattr(G._lm_model, "PREFILL_CHUNK", 4)
    model, cfg_d = _model()
    tr, L, H, Gk = model.transformer, cfg_d["n_layer"], cfg_d["n_head"], cfg_d["n_query_groups"]
    st = tr._make_state(2, 10)

    def attn_launches():
        out = [line for line in rec.log if line.split("(")[0] in extra and not line.startswith(("rmsnorm", "lm_rope_table"))]
        rec.log.clear()
        return out

    def run(T):
        y = tr.run(torch.zeros(2 * T, cfg_d["n_embd"]), 2, T, st)
        assert y.shape == (2 * T, cfg_d["n_embd"])
        return attn_launches()

    log = run(6)                                                  # positions 0 .. 5: one pass, the launches it always took
    assert [l.split("(")[0] for l in log] == ["lm_rope_append", "attention"] * L and st.offset_cpu == 6
    assert f"qkv=f32[2, 6, {(H + 2 * Gk) * 64}]" in log[0]
    log = run(7)                                                  # positions 6 .. 12: chunks of 4 and 3, attention before the append
    assert [l.split("(")[0] for l in log] == ["lm_attn_prefill", "lm_ring_append"] * (2 * L) and st.offset_cpu == 13
    rows = [int(l.split("qkv=f32[2, ")[1].split(",")[0]) for l in log]
    assert rows == [4, 4] * L + [3, 3] * L
    assert all(f"heads={H}" in l and "rope_dims=32" in l and "freqs=f32[16]" in l for l in log)
    assert all("window=9" in l for l in log[0::2])              # min(context, cap - 1)
    st11 = tr._make_state(2, 11)                                  # GPTGen's ring of context + 1 slots: the plain context
    st11.offset_cpu = 9
    tr.run(torch.zeros(2 * 3, cfg_d["n_embd"]), 2, 3, st11)
    assert all("window=10" in l for l in attn_launches()[0::2]) and st11.offset_cpu == 12
