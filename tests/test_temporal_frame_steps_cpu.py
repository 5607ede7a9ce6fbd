"""tests/helpers/temporal_frame_ref.py checked without a GPU: the case table of tests/test_temporal_frame_steps_gpu.py reaches every
path of the persistent temporal-frame launch (csrc/lm_temporal.hip) that `grid` names, every case is a shape the launcher serves, the
ring map is a brute-force write history's and RingKV.complete's, the dtype-generic reference streamed over a wrap agrees with
oracle/lm_oracle.py, and the acceptance function of the GPU test rejects every defect the cases are there to find."""
import functools

import pytest
import torch

from oracle import lm_oracle as L
from rstnet_amd import synth
from tests.helpers import temporal_frame_ref as R


def test_the_cases_reach_every_path():
    seen = {}
    for c in R.CASES:
        g = R.grid(c, 256)
        assert g.ok and g.lds <= 150 * 1024, f"{c.name}: not a shape the launcher serves (G {g.G}, LDS {g.lds})"
        assert c.L == 2 and g.lds > 48 * 1024          # every case needs the opt-in to large dynamic LDS
        seen[c.name] = R.case_flags(c, 256)
    missing = set(R.FLAGS) - set().union(*seen.values())
    assert not missing, f"no case for {sorted(missing)}"
    assert set(R.RING_CASES) | set(R.SHAPE_CASES) == set(R.BY_NAME) and set(R.CONTEXT_CASES) | set(R.STREAM_CASES) <= set(R.RING_CASES)
    # what each case is in the table for
    want = {"d128-f32": {"f32_d128", "kv_blocks_2", "splits_1", "splits_2", "splits_8", "wave_without_slot", "ctx_split_invisible", "ctx_1",
                         "ctx_over_wrap", "wrap_end0", "no_rope"},
            "d64-bf16": {"bf16_d64", "kv_blocks_2", "splits_8", "ctx_split_invisible", "ctx_1", "ctx_over_wrap", "wrap_end0"},
            "d64-f32": {"f32_d64", "splits_1", "splits_2", "wrap_end0"},
            "d128-bf16": {"bf16_d128", "splits_1", "splits_2", "wrap_end0"},
            "tab-off": {"tab_off", "Hd_tail", "Hd_k_blocks", "no_rope"},
            "e1088": {"E_tail", "rows_pair_ragged", "no_rope"},
            "rows": {"rows2_out", "no_rope"},
            "s6": {"S_lt_8", "wg_without_head", "splits_2", "no_rope"},
            "hd3848": {"k_block_partial8", "no_rope"}}
    for name, flags in want.items():
        assert flags <= seen[name], f"{name}: no longer takes {sorted(flags - seen[name])}"
    # a device with fewer CUs than a case's grid changes the paths, and `grid` says so (the GPU test asserts on it)
    assert "wg_without_head" not in R.case_flags(R.BY_NAME["s6"], 240)
    for name, st in R.repair_steps():
        assert name in R.BY_NAME and st.pos >= 0


def test_the_named_shapes_have_the_geometry_the_table_promises():
    assert [R.kv_geometry(R.BY_NAME[n]).U for n in R.RING_CASES] == [64, 256, 128, 128]
    a = R.BY_NAME["d128-f32"]
    g = R.grid(a, 256, R.Step(512, None, True))
    assert (g.G, g.S, g.active, g.per) == (64, 8, 8, 65) and "kv_blocks_2" in g.flags
    assert "kv_blocks_2" not in R.grid(a, 256, R.Step(511, None, True)).flags
    g = R.grid(R.BY_NAME["d64-bf16"], 256, R.Step(2048, None, True))
    assert (g.active, g.per) == (8, 257) and "kv_blocks_2" in g.flags
    g = R.grid(R.BY_NAME["tab-off"], 256, R.Step(35, None, True))
    assert g.blocks_per_layer[0] > R.TF_TAB_MAX and g.blocks_per_layer == (55, 57) and g.lds == 108544
    g = R.grid(R.BY_NAME["s6"], 256, R.Step(299, None, True))
    assert (g.G, g.S, g.active) == (256, 6, 2)
    g = R.grid(R.BY_NAME["rows"], 256)
    assert (g.G, g.W) == (256, 1024)
    moshi = R.Case("moshi", 4096, 32, 11264, 3000, "bf16", 32)
    g = R.grid(moshi, 256, R.Step(2999, None, True))
    assert g.ok and g.S == 8 and g.blocks_per_layer[1] <= 28 and not g.flags & {"tab_off", "S_lt_8", "E_tail", "wg_without_head", "k_block_partial8"}
    assert [n for n in R.BY_NAME if "k_block_partial8" in R.grid(R.BY_NAME[n], 256).flags] == ["hd3848"]
    for p in (0, 15, 16, 63, 64, 511, 512, 528, 529, 530, 531, 1059, 1063):
        assert p in R.positions(a)
    assert 1024 not in R.positions(R.BY_NAME["d64-f32"])


def test_ring_map_is_a_write_history_with_the_next_slot_hidden():
    for cap in range(1, 10):
        held = {}
        for pos in range(3 * cap + 1):
            held[pos % cap] = pos          # the append of position `pos`
            end = pos + 1
            for context in [None] + list(range(1, cap + 3)):
                want = []
                for s, p in held.items():
                    if s == end % cap:
                        p = end            # RingKVCache.complete counts the slot the next append takes as position `end`
                    if 0 <= pos - p and (context is None or pos - p < context):
                        want.append(s)
                assert R.visible_slots(pos, cap, context) == sorted(want), (cap, pos, context)
                if end >= cap > 1 and (context is None or context >= cap):
                    assert len(want) == cap - 1          # a full ring shows cap - 1 keys


def test_ring_map_is_ringkv_complete_with_the_streaming_mask():
    combos = {(c.cap, ctx) for c in R.CASES if c.cap <= 300 for ctx in (None, 5, c.cap)} | {(7, 3), (7, 7), (7, 9), (1, None), (2, 1)}
    for cap, context in sorted(combos, key=str):
        ring = L.RingKV(1, 1, 1, cap)
        for pos in range(2 * cap + 4):
            _, _, pos_k = ring.complete(torch.zeros(1, 1, 1, 1), torch.zeros(1, 1, 1, 1))
            delta = pos - pos_k
            mask = (pos_k >= 0) & (delta >= 0)
            if context is not None:
                mask = mask & (delta < context)
            assert R.visible_slots(pos, cap, context) == [s for s in range(cap) if bool(mask[s])], (cap, context, pos)


def test_reference_in_fp32_streamed_over_a_wrap_is_the_oracle():
    cfg = synth.LM_TINY
    sd = {k: v.float() for k, v in synth.lm_state_dict(cfg, seed=11).items()}
    E, H, nl, cap = cfg["dim"], cfg["num_heads"], cfg["num_layers"], cfg["context"]
    p = "transformer.layers"
    Hd = sd[f"{p}.0.gating.linear_out.weight"].shape[1]
    case = R.Case("tiny", E, H, Hd, cap, "f32", nl)
    co = R.SimpleNamespace(case=case, eps=float(torch.tensor(1e-8, dtype=torch.float32)),
                           in_proj=[sd[f"{p}.{l}.self_attn.in_proj_weight"] for l in range(nl)],
                           out_proj=[sd[f"{p}.{l}.self_attn.out_proj.weight"] for l in range(nl)],
                           gate_in=[sd[f"{p}.{l}.gating.linear_in.weight"] for l in range(nl)],
                           gate_out=[sd[f"{p}.{l}.gating.linear_out.weight"] for l in range(nl)],
                           norm1=[sd[f"{p}.{l}.norm1.alpha"].view(-1) for l in range(nl)], norm2=[sd[f"{p}.{l}.norm2.alpha"].view(-1) for l in range(nl)])
    g = torch.Generator().manual_seed(5)
    st = L.new_transformer_state(1, nl, H, E // H, cap)
    rings = [(torch.zeros(H, cap, E // H), torch.zeros(H, cap, E // H)) for _ in range(nl)]
    for pos in range(2 * cap + 3):
        x = torch.randn(E, generator=g)
        want = L.transformer_step(sd, "transformer", x.view(1, 1, E), st, num_heads=H, context=cfg["context"], rope=True, max_period=cfg["max_period"])
        step = R.Step(pos, cfg["context"], True)
        got = R.reference(co, step, rings, R.rope_table(pos, E // H, cfg["max_period"]), dtype=torch.float32, x=x)
        assert got.xs.dtype == torch.float32
        assert R.ratio(got.xs[-1], want[0, 0]) < 1e-5, pos
        R.append(rings, step, got, case)
    assert R.reference(co, step, rings, None, x=x).xs.dtype == torch.float64


@functools.lru_cache(maxsize=2)
def _operands(name):
    return R.make_case(R.BY_NAME[name])


def _judge(name, step, defect):
    """The acceptance of the GPU test applied to the reference carrying `defect` in place of a launch: teacher-forced with the row the
    defective run wrote, the tolerance from the fp32 run."""
    co = _operands(name)
    c = co.case
    rings = R.make_rings(co, step)
    table = R.rope_table(step.pos, c.E // c.H) if step.rope else None
    bad = R.reference(co, step, rings, table, defect=defect)
    own = R.rows_of(bad)
    ref64 = R.reference(co, step, rings, table, own=own)
    ref32 = R.reference(co, step, rings, table, own=own, dtype=torch.float32)
    tol = R.tolerance(ref32, ref64, c)
    return R.accept(bad, ref64, tol, c), tol, (ref32, ref64)


def _ctx_steps(name):
    return [s for s in R.steps(R.BY_NAME[name]) if s.context]


def _at(name, pos):
    return [s for s in R.steps(R.BY_NAME[name]) if s.pos == pos and s.context is None and s.rope][:1]


# defect -> (case, steps of that case's own table on which the acceptance must reject it, the flag those steps claim)
DEFECT_CASES = {
    "ctx_ignored": [("d128-f32", [s for s in _ctx_steps("d128-f32") if s.context == 5], "ctx_split_invisible"),
                    ("d64-bf16", [s for s in _ctx_steps("d64-bf16") if s.context == 259], None)],
    "oldest_slot_visible": [("d128-f32", _at("d128-f32", 529) + _at("d128-f32", 530) + _at("d128-f32", 1063), "wrap_end0"),
                            ("d128-bf16", _at("d128-bf16", 141), None)],
    "own_slot_stale": [("d64-f32", _at("d64-f32", 0) + _at("d64-f32", 140), None), ("d128-bf16", _at("d128-bf16", 139), "wrap_end0")],
    "own_kv_unrounded": [("d128-bf16", _at("d128-bf16", 0), "bf16_d128"), ("d64-bf16", [s for s in _ctx_steps("d64-bf16") if s.context == 1], "ctx_1")],
    "k_unrotated": [("d64-f32", _at("d64-f32", 31), "f32_d64"), ("d128-bf16", _at("d128-bf16", 127), None)],
    "last_slot_dropped": [("d128-f32", _at("d128-f32", 63) + _at("d128-f32", 528), None), ("d64-f32", _at("d64-f32", 139), None)],
    "last_split_dropped": [("d64-f32", _at("d64-f32", 128), "splits_2"), ("d128-f32", _at("d128-f32", 512), "splits_8")],
    "second_kv_block_dropped": [("d128-f32", _at("d128-f32", 512) + _at("d128-f32", 1063), "kv_blocks_2"), ("d64-bf16", _at("d64-bf16", 2048), "kv_blocks_2")],
    "wave1_slots_dropped": [("d64-f32", _at("d64-f32", 32), None), ("d128-bf16", _at("d128-bf16", 32), None)],
    "merge_unscaled": [("d128-f32", _at("d128-f32", 64) + _at("d128-f32", 512), "splits_8"), ("d128-bf16", _at("d128-bf16", 128), "splits_2")],
    "rotate_half_instead_of_pairs": [("d128-bf16", _at("d128-bf16", 32), None), ("d64-f32", _at("d64-f32", 141), None)],
    "k_tail_E": [("e1088", R.steps(R.BY_NAME["e1088"])[1:2], "E_tail")],
    "k_tail_Hd": [("tab-off", R.steps(R.BY_NAME["tab-off"])[1:2], "Hd_tail")],
    "second_row_dropped": [("rows", R.steps(R.BY_NAME["rows"])[1:2], "rows2_out")],
    "norm2_on_layer_input": [("d64-f32", _at("d64-f32", 127), None)],
}


def test_every_defect_has_cases():
    assert set(DEFECT_CASES) == set(R.DEFECTS)
    for defect, rows in DEFECT_CASES.items():
        for name, sts, flag in rows:
            assert sts, f"{defect}: the step it is judged on has left {name}'s table"
            if flag:
                assert any(flag in R.grid(R.BY_NAME[name], 256, s).flags for s in sts), f"{defect}: no step of {name} claims {flag}"


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_acceptance_rejects_the_defect(defect):
    for name, sts, _ in DEFECT_CASES[defect]:
        for step in sts:
            (ok, where, r), tol, _ = _judge(name, step, defect)
            assert not ok, f"{defect} on {name} at {step}: worst {where} {r:.3e} passes tol {tol:.3e}"


@pytest.mark.parametrize("name,index", [("d128-f32", 6), ("d128-f32", 17), ("d64-bf16", 9), ("d64-bf16", 13), ("d64-f32", 5), ("d128-bf16", 8),
                                        ("e1088", 2), ("tab-off", 3)])
def test_clean_fp32_reference_is_accepted(name, index):
    step = R.steps(R.BY_NAME[name])[index]
    (ok, where, r), tol, (ref32, ref64) = _judge(name, step, None)
    assert ok and r < 2.0 ** -23, f"{name} at {step}: the fp64 reference against itself: {where} {r:.3e}"
    assert R.TOL_FLOOR <= tol <= R.TOL_CEIL
    c = R.BY_NAME[name]
    ok, where, r = R.accept(ref32, ref64, tol, c)
    assert ok, f"{name} at {step}: {where} {r:.3e} vs tol {tol:.3e}"
    nan = ref32._replace(xs=ref32.xs.clone())
    nan.xs[0, 0] = float("nan")
    assert not R.accept(nan, ref64, tol, c)[0]
    # the poison is where the step must not look, its own slot included, and the step sees the rest as it was drawn
    co = _operands(name)
    K, V = R.make_rings(co, step)[0]
    vis = [s for s in R.visible_slots(step.pos, c.cap, step.context) if s != step.pos % c.cap]
    hidden = sorted(set(range(c.cap)) - set(vis))
    assert float(K[:, hidden].abs().max()) == 0.0 and float(V[:, hidden].abs().min()) == R.POISON and step.pos % c.cap in hidden
    assert torch.equal(K[:, vis], co.ring_base[0][0][:, vis]) and bool(torch.isfinite(V).all())


def test_half_ulp_and_row_bound():
    x = torch.tensor([1.0, 1.5, 0.99, 2.0 ** -10, 0.0, -3.0])
    assert R.half_ulp_bf16(x).tolist() == [2.0 ** -8, 2.0 ** -8, 2.0 ** -9, 2.0 ** -18, 0.0, 2.0 ** -7]
    c16, c32 = R.BY_NAME["d128-bf16"], R.BY_NAME["d128-f32"]
    new = torch.linspace(-1.3, 1.7, 128, dtype=torch.float64)
    assert R.row_ratio(R.round_to_ring(new, c16), new, c16) == 0.0
    assert R.row_ratio(new.float(), new, c32) < 2.0 ** -24
    off = R.round_to_ring(new, c16).clone()
    off[5] += 2.0 ** -7          # the other bf16 neighbour of an element near 1.2
    assert R.row_ratio(off, new, c16) > 1e-3 and R.row_ratio(new.float() + 1e-4, new, c32) > 5e-5
