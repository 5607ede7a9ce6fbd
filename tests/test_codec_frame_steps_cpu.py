"""tests/helpers/codec_frame_ref.py checked without a GPU: the case table of tests/test_codec_frame_steps_gpu.py reaches every path of
the persistent codec-transformer launch (csrc/codec_tr.hip) that `grid` names, every case is a shape the launcher serves, the ring map
is a brute-force write history's, the dtype-generic reference streamed over a wrap agrees with oracle/mimi_oracle.py's
TransformerStream, the granule layout and epochs are those of a small model of the kernel's publish order, and the acceptance
function of the GPU test rejects every defect the cases are there to find."""
import functools

import numpy as np
import pytest
import torch

from oracle import mimi_oracle as O
from tests.helpers import codec_frame_ref as R


def test_the_cases_reach_every_path():
    seen = {}
    for c in R.CASES:
        assert c.L == 2
        for T in R.TS[c.name]:
            g = R.grid(c, T, 256)
            assert g.ok and 0 < g.lds <= R.LDS_LIMIT, f"{c.name} T {T}: not a shape the launcher serves (G {g.G}, LDS {g.lds})"
        seen[c.name] = R.case_flags(c, 256)
    missing = set(R.FLAGS) - set().union(*seen.values())
    assert not missing, f"no case for {sorted(missing)}"
    assert set(R.RING_CASES) | set(R.SHAPE_CASES) == set(R.BY_NAME) and set(R.STREAM_CASES) <= set(R.BY_NAME)
    # every (streams, positions) instance: R = 1 .. 4 are four kernels
    assert {c.B * T for c in R.CASES for T in R.TS[c.name]} == {1, 2, 3, 4}
    # what each case is in the table for
    ring = {"ring_empty", "unwritten_slots", "wrap_end0", "ctx_1", "ctx_masks_old", "ctx_gt_cap", "ctx_none", "ctx_over_wrap", "no_rope"}
    want = {"d16": ring | {"d16", "R1", "R2", "slot_batches_2", "wg_without_head", "step_wraps", "ctx_over_wrap"},
            "d32": ring | {"d32", "R3", "R4", "T3", "T4", "inproj_rounds_3", "outproj_rounds_2", "lin1_row_masked", "step_wraps", "ctx_lt_T"},
            "d64": ring | {"d64", "R4", "step_wraps", "ctx_over_wrap", "ctx_lt_T"},
            "d128": ring | {"d128", "R4", "T4", "slot_batches_2", "step_wraps", "ctx_lt_T"},
            "d256": ring | {"d256", "R2", "slot_batches_2", "slot_batches_3"},
            "e528": {"k_chunk_2", "k_chunk_partial", "odd_heads", "no_rope", "step_wraps"},
            "e1088": {"k_chunk_3", "k_chunk_partial", "ln_tail", "odd_heads", "no_rope"},
            "f2056": {"lin2_k_block_2", "lin2_k_block_partial8", "R3", "no_rope"},
            "rows4": {"BH_eq_G", "R4", "no_rope"},
            "short": {"short_ring", "step_wraps", "T4"},
            "short4": {"short_ring", "cap_eq_T", "empty_row", "T4"},
            "noscale": {"no_scale", "no_rope"}}
    assert set(want) == set(R.BY_NAME)
    for name, flags in want.items():
        assert flags <= seen[name], f"{name}: no longer takes {sorted(flags - seen[name])}"
    # a device with fewer CUs than a case's grid changes the paths, and `grid` says so (the GPU test asserts on it)
    assert "BH_eq_G" not in R.case_flags(R.BY_NAME["rows4"], 8) and not R.grid(R.BY_NAME["rows4"], 1, 8).ok
    for name, st in R.repair_steps():
        assert R.grid(R.BY_NAME[name], st.T, 256, st).ok


def test_the_named_shapes_have_the_geometry_the_table_promises():
    geo = {n: R.kv_geometry(R.BY_NAME[n]) for n in R.RING_CASES}
    assert [(g.D, g.GS, g.NC, g.SPB) for g in geo.values()] == [(16, 4, 64, 1024), (32, 8, 32, 512), (64, 16, 16, 256), (128, 32, 8, 128), (256, 64, 4, 64)]
    assert geo["d16"].capS == 2124 and geo["d256"].capS == 214
    g = R.grid(R.BY_NAME["d16"], 2, 256, R.Step(1023, 1100, True, 2))
    assert (g.G, g.W, g.nb) == (16, 64, 2) and "slot_batches_2" in g.flags
    assert "slot_batches_2" not in R.grid(R.BY_NAME["d16"], 2, 256, R.Step(1022, 1100, True, 2)).flags
    g = R.grid(R.BY_NAME["d32"], 4, 256)
    assert (g.G, g.W) == (16, 64) and g.rounds == {"in_proj": (3, 1), "out_proj": (2, 1), "linear1": (1, 1), "linear2": (2, 1)}
    g = R.grid(R.BY_NAME["d64"], 2, 256)          # Mimi's layer: one round of everything but the out-projection rows at 256 CUs
    assert (g.G, g.W, g.lds) == (256, 1024, R.lds_bytes(R.BY_NAME["d64"], 2)) and g.rounds["linear2"] == (1, 1)
    assert R.grid(R.BY_NAME["d256"], 1, 256, R.Step(150, 150, True, 1)).nb == 3
    assert R.grid(R.BY_NAME["e528"], 2, 256).rounds["in_proj"][1] == 2 and R.grid(R.BY_NAME["e1088"], 1, 256).rounds["out_proj"][1] == 3
    assert R.grid(R.BY_NAME["f2056"], 3, 256).rounds["linear2"] == (1, 2)
    g = R.grid(R.BY_NAME["rows4"], 1, 256)
    assert g.G == 16 == R.BY_NAME["rows4"].B * R.BY_NAME["rows4"].H
    # the refusals of rst_codec_tr_grid, each next to a served neighbour
    base = R.BY_NAME["d64"]
    assert R.grid(base, 2, 256).ok
    for bad, T in ((base._replace(H=3), 1), (base._replace(E=192, H=4), 1), (base._replace(E=64, H=8), 1), (base._replace(B=1), 5),
                   (base._replace(B=5), 1), (base._replace(B=1, cap=3), 4), (base._replace(F=2044), 2), (base._replace(E=100, H=5), 1),
                   (base._replace(B=1, F=24), 1), (base._replace(cap=4000), 2)):
        assert not R.grid(bad, T, 256).ok, (bad, T)
    assert R.grid(base._replace(B=1, cap=4), 4, 256).ok and R.grid(base._replace(B=1, F=32), 1, 256).ok


def test_ring_map_is_a_write_history_with_the_next_slot_hidden():
    """Positions appended one step at a time in several cuts; what each slot holds is recorded.  After a step of T from `pos` the
    restated map says for every slot either the recorded position or -- for the slot the next append takes -- the future position
    `end`; the visible set of every query follows.  Every (cap, T, pos, context) of the table is among those walked."""
    wanted = {(c.cap, st.T, st.pos, st.context) for c in R.CASES for st in R.steps(c)} | \
             {(R.BY_NAME[n].cap, st.T, st.pos, st.context) for n, st in R.repair_steps()}
    contexts, last, at = {}, {}, {}
    for cap, T, pos, ctx in wanted:
        contexts.setdefault((cap, T), set()).add(ctx)
        at.setdefault((cap, T), set()).add(pos)
        last[cap, T] = max(last.get((cap, T), 0), pos)
    walked = set()
    for (cap, T), ctxs in sorted(contexts.items()):
        ctxs = sorted(ctxs, key=lambda v: v or 0)
        for lead in range(T):          # `lead` single steps first, then steps of T: every position is the start of a step of T
            held, end = {}, 0

            def push(n):
                nonlocal end
                for p in range(end, end + n):
                    held[p % cap] = p
                end += n
            for _ in range(lead):
                push(1)
            while end <= last[cap, T]:
                pos = end
                push(T)
                if (cap > 40 or pos > 3 * cap + 4) and pos not in at[cap, T]:          # long rings, far positions: the table's only
                    continue
                for s in range(cap):
                    p = R.slot_position(s, end, cap)
                    assert p == (None if s not in held else end if s == end % cap else held[s]), (cap, T, pos, s)
                for ctx in ctxs:
                    if (cap > 40 or pos > 3 * cap + 4) and (cap, T, pos, ctx) not in wanted:
                        continue
                    for t in range(T):
                        want = []
                        for s, p in held.items():
                            if s == end % cap:
                                p = end
                            if 0 <= pos + t - p and (not ctx or pos + t - p < ctx):
                                want.append(s)
                        assert R.visible_slots(pos + t, end, cap, ctx) == sorted(want), (cap, T, pos, ctx, t)
                    assert R.step_mask(R.Step(pos, ctx, True, T), cap).tolist() == \
                        [[s in R.visible_slots(pos + t, end, cap, ctx) for s in range(cap)] for t in range(T)] if cap <= 40 else True
                    walked.add((cap, T, pos, ctx))
    assert wanted <= walked, sorted(wanted - walked, key=str)[:5]
    # a full ring shows cap - 1 keys to its last query; a ring as long as the step shows its first query none
    assert len(R.visible_slots(43, 44, 20, None)) == 19 and R.visible_slots(8, 12, 4, None) == [] and R.visible_slots(11, 12, 4, None) == [1, 2, 3]


def test_ring_map_is_ringkvcache_complete_with_the_streaming_mask():
    for cap, cuts in ((5, (4, 4, 1, 2, 4, 3)), (4, (4, 4, 2, 4)), (20, (3, 4, 1, 2) * 4), (37, (3, 4, 1, 2) * 7)):
        ring = O.RingKVCache(1, 1, 1, cap)
        pos = 0
        for T in cuts:
            _, _, pos_k = ring.complete(torch.zeros(1, 1, T, 1), torch.zeros(1, 1, T, 1))
            for ctx in (None, 1, 3, cap, cap + 2):
                for t in range(T):
                    delta = pos + t - pos_k
                    mask = (pos_k >= 0) & (delta >= 0)
                    if ctx is not None:
                        mask = mask & (delta < ctx)
                    assert R.visible_slots(pos + t, pos + T, cap, ctx) == mask.nonzero().view(-1).tolist(), (cap, pos, T, ctx, t)
            pos += T


def _oracle_state(co):
    c, sd = co.case, {}
    for l in range(c.L):
        p = f"tr.transformer.layers.{l}"
        sd[f"{p}.norm1.weight"], sd[f"{p}.norm1.bias"] = co.norm1_w[l], co.norm1_b[l]
        sd[f"{p}.norm2.weight"], sd[f"{p}.norm2.bias"] = co.norm2_w[l], co.norm2_b[l]
        sd[f"{p}.self_attn.in_proj_weight"], sd[f"{p}.self_attn.out_proj.weight"] = co.in_proj[l], co.out_proj[l]
        sd[f"{p}.linear1.weight"], sd[f"{p}.linear2.weight"] = co.linear1[l], co.linear2[l]
        sd[f"{p}.layer_scale_1.scale"] = co.scale1[l] if co.scale1[l] is not None else torch.ones(c.E)
        sd[f"{p}.layer_scale_2.scale"] = co.scale2[l] if co.scale2[l] is not None else torch.ones(c.E)
    return sd


@pytest.mark.parametrize("name,cuts", [("short", (4, 1, 4, 2, 4, 4, 3)), ("short4", (4, 4, 1, 4, 2, 4)), ("d32", (3, 4, 1, 2) * 8 + (4,) * 3),
                                       ("rows4", (1,) * 45), ("noscale", (2, 1, 2) * 9), ("e1088", (1,) * 24), ("d256", (1, 2) * 4)])
def test_reference_in_fp32_streamed_over_a_wrap_is_the_oracle(name, cuts):
    co = R.make_case(R.BY_NAME[name])
    c = co.case
    cfg = O.MimiConfig(latent_dim=c.E, num_heads=c.H, num_layers=c.L, context=c.cap, dim_feedforward=c.F, max_period=R.MAX_PERIOD)
    ts = O.TransformerStream(_oracle_state(co), "tr", cfg, c.B)
    rings = [(torch.zeros(c.B, c.H, c.cap, c.E // c.H), torch.zeros(c.B, c.H, c.cap, c.E // c.H)) for _ in range(c.L)]
    g = torch.Generator().manual_seed(5)
    pos = 0
    for T in cuts:
        co.x = torch.randn(c.B, 4, c.E, generator=g)
        with torch.no_grad():
            want = ts.step(co.x[:, :T].transpose(1, 2)).transpose(1, 2)
        step = R.Step(pos, c.cap, True, T)
        got = R.reference(co, step, rings, dtype=torch.float32)
        assert got.xs.dtype == torch.float32
        assert R.ratio(got.xs[-1], want) < 1e-5, (name, pos, T)
        R.append(rings, step, got, c)
        for l in range(c.L):          # the rings themselves
            assert R.ratio(rings[l][0], ts.rings[l].k) < 1e-5 and R.ratio(rings[l][1], ts.rings[l].v) < 1e-5
        pos += T
    assert pos > c.cap or name == "d256", "the stream must pass the ring wrap"
    assert R.reference(co, step, rings).xs.dtype == torch.float64


def test_granule_layout_and_epochs_are_the_publish_orders():
    """A numpy model of what codec_tr_kernel publishes, in its order: per layer QKV (epoch l + 1), ATT (l + 1), X (2l + 1: the residual
    after attention), H (l + 1), X (2l + 2); granule = tag << 32 | value bits, arrays X | QKV | ATT | H of [rows][width] granules,
    row = stream * T + t, the repair launch's set one set further on.  `read_handoff` must find every value and tag."""
    for name, T in (("d32", 3), ("d64", 2), ("f2056", 3), ("rows4", 1)):
        c = R.BY_NAME[name]
        E, F, Rr, L = c.E, c.F, c.B * T, 3
        n = Rr * (5 * E + F)
        assert R.granules(c, T) == n
        for solo in (False, True):
            ws = np.zeros(2 * n, dtype=np.uint64)
            base = n if solo else 0
            gX, gQKV, gATT, gH = base, base + Rr * E, base + Rr * 4 * E, base + Rr * 5 * E
            value = {}

            def publish(first, width, epoch, tagname):
                for row in range(Rr):
                    for r in range(width):
                        v = np.float32(epoch * 1000 + row * 7 + r * 0.25 + len(tagname))
                        ws[first + row * width + r] = (np.uint64(epoch) << np.uint64(32)) | np.uint64(v.view(np.uint32))
                        value[tagname, row, r] = float(v)
            eX = 0
            for l in range(L):
                publish(gQKV, 3 * E, l + 1, "QKV")
                publish(gATT, E, l + 1, "ATT")
                eX += 1
                publish(gX, E, eX, "X")
                publish(gH, F, l + 1, "H")
                eX += 1
                publish(gX, E, eX, "X")
            hand = R.read_handoff(torch.from_numpy(ws.view(np.int64)), c, T, solo=solo)
            other = R.read_handoff(torch.from_numpy(ws.view(np.int64)), c, T, solo=not solo)
            for nm, width in (("X", E), ("QKV", 3 * E), ("ATT", E), ("H", F)):
                vals, tags = getattr(hand, nm), getattr(hand, nm + "_tag")
                assert tuple(vals.shape) == (c.B, T, width) and bool((tags == R.epochs(L)[nm]).all())
                assert vals.reshape(Rr, width).tolist() == [[value[nm, row, r] for r in range(width)] for row in range(Rr)]
                assert not bool(getattr(other, nm + "_tag").any())          # the memset in front of every launch covers both sets
    assert [(nm, off) for nm, off, _, _ in R.layout(R.BY_NAME["d32"], 3)] == [("X", 0), ("QKV", 384), ("ATT", 1536), ("H", 1920)]


# ---- every defect is rejected --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _operands(name):
    return R.make_case(R.BY_NAME[name])


def _judge(name, step, defect):
    """The acceptance of the GPU test applied to the reference carrying `defect` in place of a launch: teacher-forced with the rows the
    defective run wrote, the tolerance from the fp32 run."""
    co = _operands(name)
    c = co.case
    rings = R.make_rings(co, step)
    bad = R.reference(co, step, rings, defect=defect)
    own = R.rows_of(bad)
    ref64 = R.reference(co, step, rings, own=own)
    ref32 = R.reference(co, step, rings, own=own, dtype=torch.float32)
    tol = R.tolerance(ref32, ref64, c)
    return R.accept(bad, ref64, tol, c), tol, (ref32, ref64)


def _sel(name, **kw):
    """The steps of `name`'s own table that match (pos / context / T / rope)."""
    return [s for s in R.steps(R.BY_NAME[name]) if all(getattr(s, k) == v for k, v in kw.items())]


def _cap(name):
    return R.BY_NAME[name].cap


# defect -> (case, steps of that case's own table on which the acceptance must reject it, the flag those steps claim)
DEFECT_CASES = {
    "window_wide": [("d16", _sel("d16", pos=1107, context=2) + _sel("d16", pos=1107, context=1027), "ctx_masks_old"),
                    ("d128", _sel("d128", pos=144, context=4), None)],
    "window_narrow": [("d32", _sel("d32", pos=44, context=36), None), ("d256", _sel("d256", pos=157, context=67), "ctx_masks_old"),
                      ("d64", _sel("d64", pos=246, context=2), None)],
    "own_hidden": [("d64", _sel("d64", pos=0), "ring_empty"), ("short", _sel("short", pos=8), "short_ring"), ("d256", _sel("d256", pos=151), None)],
    "end_offset_is_pos": [("d32", _sel("d32", pos=0, T=3) + _sel("d32", pos=38, T=4), None), ("short", _sel("short", pos=4), "step_wraps"),
                          ("d128", _sel("d128", pos=149), "step_wraps")],
    "append_per_query": [("d128", _sel("d128", pos=150) + _sel("d128", pos=303), None), ("short", _sel("short", pos=8), "short_ring"),
                         ("d64", _sel("d64", pos=249, context=250), "step_wraps")],
    "rope_pos_ignores_t": [("d32", _sel("d32", pos=36, T=4), None), ("d64", _sel("d64", pos=0), None), ("noscale", _sel("noscale", pos=10), None)],
    "unused_slot_read": [("d16", _sel("d16", pos=0, T=1) + _sel("d16", pos=1023, T=2), "unwritten_slots"), ("d256", _sel("d256", pos=63), "unwritten_slots")],
    "k_tail_dropped": [("e528", _sel("e528", pos=10), "k_chunk_partial"), ("e1088", _sel("e1088", pos=10), "k_chunk_partial"),
                       ("f2056", _sel("f2056", pos=10), "lin2_k_block_partial8")],
    "ln_tail_dropped": [("e1088", _sel("e1088", pos=0) + _sel("e1088", pos=23), "ln_tail")],
    "ln_unbiased": [("d32", _sel("d32", pos=0, T=3), None), ("d64", _sel("d64", pos=251, context=250), None)],
    "scale_skipped": [("d16", _sel("d16", pos=0, T=1), None), ("rows4", _sel("rows4", pos=10), None)],
    "second_batch_dropped": [("d16", _sel("d16", pos=1024, T=1) + _sel("d16", pos=2203, T=2), "slot_batches_2"),
                             ("d256", _sel("d256", pos=64), "slot_batches_2"), ("d128", _sel("d128", pos=128), "slot_batches_2")],
    "head_of_other_stream": [("d64", _sel("d64", pos=250), None), ("d256", _sel("d256", pos=149), None), ("rows4", _sel("rows4", pos=23), None)],
}


def test_every_defect_has_cases():
    assert set(DEFECT_CASES) == set(R.DEFECTS)
    for defect, rows in DEFECT_CASES.items():
        for name, sts, flag in rows:
            assert sts, f"{defect}: the step it is judged on has left {name}'s table"
            if flag:
                assert any(flag in R.grid(R.BY_NAME[name], s.T, 256, s).flags for s in sts), f"{defect}: no step of {name} claims {flag}"


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_acceptance_rejects_the_defect(defect):
    for name, sts, _ in DEFECT_CASES[defect]:
        for step in sts:
            (ok, where, r), tol, _ = _judge(name, step, defect)
            assert not ok, f"{defect} on {name} at {step}: worst {where} {r:.3e} passes tol {tol:.3e}"


@pytest.mark.parametrize("name,index", [("d16", 3), ("d16", 20), ("d32", 12), ("d64", 5), ("d128", 8), ("d256", 14), ("e1088", 2), ("f2056", 1),
                                        ("short", 3), ("short4", 2), ("noscale", 4)])
def test_clean_fp32_reference_is_accepted(name, index):
    step = R.steps(R.BY_NAME[name])[index]
    (ok, where, r), tol, (ref32, ref64) = _judge(name, step, None)
    assert ok and r < 2.0 ** -23, f"{name} at {step}: the fp64 reference against itself: {where} {r:.3e}"
    assert R.TOL_FLOOR <= tol <= R.TOL_CEIL
    c = R.BY_NAME[name]
    ok, where, r = R.accept(ref32, ref64, tol, c)
    assert ok, f"{name} at {step}: {where} {r:.3e} vs tol {tol:.3e}"
    nan = ref32._replace(xs=ref32.xs.clone())
    nan.xs[0, 0, 0, 0] = float("nan")
    assert not R.accept(nan, ref64, tol, c)[0]
    # the poison is where no query of the step may look, the new positions' slots included, and the step sees the rest as it was drawn
    co = _operands(name)
    K, V = R.make_rings(co, step)[0]
    new = set(R.new_slots(step, c.cap))
    vis = sorted({s for t in range(step.T) for s in R.visible_slots(step.pos + t, step.pos + step.T, c.cap, step.context)} - new)
    hidden = sorted(set(range(c.cap)) - set(vis))
    assert new <= set(hidden) and float(K[:, :, hidden].abs().max()) == 0.0 and float(V[:, :, hidden].abs().min()) == R.POISON
    assert torch.equal(K[:, :, vis], co.ring_base[0][0][:, :, vis]) and bool(torch.isfinite(V).all())
