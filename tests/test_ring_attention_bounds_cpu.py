"""tests/helpers/ring_attention_ref.py without a GPU: its ring-by-position against oracle.lm_oracle.RingKV stepped that many times, the
designed scores of every (case, profile, position) after rounding to the ring's dtype, the fp32 run of the reference (and the
emulation of prefill_attn_bf16_kernel's hi + lo operand planes) inside the bound, every listed defect rejected by a NAMED (case,
profile, position), and the case table's coverage of the kernel instances the launchers reach."""
import pytest
import torch

from oracle import lm_oracle as L
from tests.helpers import ring_attention_ref as R
from tests.helpers.temporal_frame_ref import visible

CUS = (256, 304, 64)
SKIPPED_PAIRS = ()          # (case, profile) pairs left out of the GPU test: none


def triples(cus=256):
    for case in R.CASES:
        c = R.resolve(case, cus)
        for profile in c.profiles:
            if (c.name, profile) in SKIPPED_PAIRS:
                continue
            for position in c.positions:
                yield c, profile, position


_MEASURED = {}


def measured(c, profile, position):
    """(operands, fp64 / fp32 runs and tolerance) of one triple; kept for the tests of this module that share them."""
    key = (c.name, profile, position)
    if key not in _MEASURED:
        b = R.build(c, profile, position)
        _MEASURED[key] = (b, R.measure(b))
    return _MEASURED[key]


# ---- the ring map ---------------------------------------------------------------------------------------------------------------------------
def _stepped(cap, upto):
    """RingKV stepped `upto` times with key = value = the step's position: per number of steps n the slots' contents before step n and
    the (slot -> position) vector `complete` returned for step n - 1."""
    ring = L.RingKV(1, 1, 1, cap)
    content, pos_k = {0: ring.k[0, 0, :, 0].clone() - 1}, {}
    held = torch.full((cap,), -1.0)
    for n in range(upto):
        x = torch.full((1, 1, 1, 1), float(n))
        k, _, pk = ring.complete(x, x)
        held = held.clone()
        held[n % cap] = float(n)
        assert torch.equal(k[0, 0, :, 0][held >= 0], held[held >= 0])
        content[n + 1], pos_k[n + 1] = held, pk.clone()
    return content, pos_k


def _named_positions():
    out = {}
    for case in R.CASES:
        c = R.resolve(case, 256)
        for position in c.positions:
            for p in R.stream_pos(c, position):
                out.setdefault(c.cap, set()).add(p + c.T)
    for cap in (2, 3):
        out[cap] |= set(range(3 * cap + 4))
    return out


def test_ring_by_position_is_the_stepped_ring():
    """`held`, the entries `queries` lists and the poison map of `build` against RingKV: every number of steps in 0 .. 3 cap + 3 for the
    two smallest rings, and the named positions of every case."""
    for cap, ns in sorted(_named_positions().items()):
        content, pos_k = _stepped(cap, max(ns) + 1)
        for n in sorted(ns):
            for s in range(cap):
                h = R.held(s, n, cap)
                assert (-1 if h is None else h) == int(content[n][s]), (cap, n, s)
            if n:          # the mask _ring_attention_case builds from ring.complete for the step at position n - 1
                pk = pos_k[n]
                for ctx in (None, 1, 2, cap - 1, cap):
                    delta = (n - 1) - pk
                    mask = (pk >= 0) & (delta >= 0) & ((delta < ctx) if ctx else torch.ones_like(pk, dtype=torch.bool))
                    assert [bool(m) for m in mask] == [visible(s, n - 1, cap, ctx) for s in range(cap)], (cap, n, ctx)
    for case in R.CASES:
        c = R.resolve(case, 256)
        for position in c.positions:
            for P in set(R.stream_pos(c, position)):
                content, pos_k = _stepped_cached(c.cap)
                qs = R.queries(c, P)
                for t, rows in enumerate(qs):
                    # (a chunk of a whole ring: the first query's slot is end_offset % cap, the future -- that query sees nothing)
                    assert any(r[2] == P + t for r in rows) or (c.entry == "qpre" and c.T == c.cap and t == 0 and not rows), "the query's own key"
                    n_ring = P + c.T if c.entry == "qpre" else P
                    for kind, i, p in rows:
                        if kind == "ring":
                            assert int(content[n_ring][i]) == p, (c.name, P, t, i)
                        else:
                            assert P + i == p and i <= t
                    if c.entry in ("decode", "gemv"):
                        pk = pos_k[P + 1]
                        delta = P - pk
                        mask = (pk >= 0) & (delta >= 0) & ((delta < c.context) if c.context else torch.ones_like(pk, dtype=torch.bool))
                        assert sorted(int(s) for s in mask.nonzero()) == sorted(i if kind == "ring" else P % c.cap for kind, i, p in rows)
                    elif c.entry == "qpre":
                        pk = pos_k[P + c.T]
                        delta = P + t - pk
                        mask = (pk >= 0) & (delta >= 0) & ((delta < c.context) if c.context else torch.ones_like(pk, dtype=torch.bool))
                        assert sorted(int(s) for s in mask.nonzero()) == sorted(i for _, i, _ in rows)
                    else:
                        assert sorted(p for _, _, p in rows) == list(range(max(0, P + t - c.context + 1), P + t + 1))


_STEPPED = {}


def _stepped_cached(cap):
    if cap not in _STEPPED:
        _STEPPED[cap] = _stepped(cap, max(_named_positions()[cap]) + 1)
    return _STEPPED[cap]


# ---- the designed scores --------------------------------------------------------------------------------------------------------------------
def test_designed_scores_after_rounding():
    """Every (case, profile, position): all operands finite, every achieved |score| <= 100, the profile's defining inequalities on the
    achieved scores of every live query, and every poisoned key's would-be score >= 30 above the query's visible maximum (`k0`: 0)."""
    n = 0
    for c, profile, position in triples():
        b, m = measured(c, profile, position)
        kind, variant = (profile.split("/") + ["dominant"])[:2]
        assert all(bool(torch.isfinite(x).all()) for x in (b.qkv, b.K, b.V)), (c.name, profile)
        ref = m.ref64
        assert bool(torch.isfinite(ref.out).all())
        for bi in range(c.B):
            d = b.designed[bi]
            for t in R.live_queries(c, bi):
                if c.entry == "qpre" and c.T == c.cap and t == 0:          # sees nothing (its own slot counts as the future): the launch returns 0
                    assert (bi, t) not in ref.scores and float(ref.out[bi, t].abs().max()) == 0.0
                    continue
                sc, rows, _ = ref.scores[bi, t]
                where = (c.name, profile, position, bi, t)
                assert float(sc.abs().max()) <= 100.0, where
                top = sc.max(-1).values
                # poison: every ring slot and chunk row outside the launch's key universe
                seen = {k[:2] for k in d.keys}
                hid = [s for s in range(c.cap) if ("ring", s) not in seen]
                qpk = c.H // c.G
                if hid:
                    kp = b.K[bi][:, hid].double()[torch.arange(c.H) // qpk]
                    would = torch.einsum("hd,hnd->hn", ref.qrot[bi][:, t], kp) / c.D ** 0.5
                    if variant == "k0":
                        assert float(would.abs().max()) == 0.0
                    else:
                        assert float((would.min(-1).values - top).min()) >= 30.0, where
                    assert float(b.V[bi][:, hid].abs().min()) == R.POISON
                pos_of = [r[2] for r in rows]
                order = pos_of if c.entry == "prefill" else [(p % c.cap, p) for p in pos_of]
                by = sorted(range(len(rows)), key=lambda i: order[i])
                s_ord = sc[:, by]
                ring = torch.tensor([rows[i][0] == "ring" for i in by])
                if kind.startswith("peak") and d.peak is not None and d.peak in rows and len(rows) > 1:
                    i = rows.index(d.peak)
                    rest = torch.cat([sc[:, :i], sc[:, i + 1:]], 1)
                    assert float((sc[:, i] - rest.max(-1).values).min()) >= 30.0, where
                    vrow = (b.V[bi][:, d.peak[1]] if d.peak[0] == "ring" else ref.v_row[bi][:, d.peak[1]]).double()[torch.arange(c.H) // qpk]
                    assert float((ref.out[bi, t] - vrow).abs().max()) <= 1e-9, where          # the output is that key's value row
                elif kind in ("low", "high"):
                    e = min(90.0, c.smax)
                    lo, hi = (e - 10.0, e) if kind == "high" else (-e, -e + 10.0)
                    assert lo <= float(sc.min()) and float(sc.max()) <= hi, where
                elif kind.startswith("ramp") and len(rows) > 1:
                    sgn = -1.0 if kind == "ramp_down" else 1.0
                    tg = {k[:2]: float(v) for k, v in zip(d.keys, d.targets)}
                    want = torch.tensor([tg[rows[i][:2]] for i in by], dtype=torch.float64)
                    if int(ring.sum()) > 1:          # ring keys: monotone in the launch's order (1e-3: the query's own fp32 rounding)
                        assert float((sgn * s_ord[:, ring].diff(dim=-1)).min()) >= -1e-3, where
                    assert float((s_ord - want).abs().max()) <= 0.5 + abs(float(want.diff().abs().max())) * 2, where
        n += 1
    assert n == sum(len(c.profiles) * len(c.positions) for c in R.CASES)
    # the spans as designed, on the largest key sets
    for name, profile, span in (("many-c2048-d64-f32", "ramp_wide", 109.0), ("split-c300-d128-f32", "ramp_up", 59.0),
                                ("pf-t33-w299-d128-f32", "ramp_wide", 109.0), ("pf-t33-w299-d128-bf16", "ramp_wide", 61.0)):
        c = R.resolve(R.BY_NAME[name], 256)
        b, m = measured(c, profile, c.positions[-1])
        sc, first = m.ref64.scores[0, c.T - 1][0], m.ref64.scores[0, 0][0]
        # (a prefill query sees its window of the chunk's ramp: the whole span lies between the first query's oldest and the last one's own key)
        assert float((sc.max(-1).values - first.min(-1).values).min()) >= span, name
        assert float((sc.max(-1).values - sc.min(-1).values).min()) >= 0.85 * span, name
        if profile == "ramp_wide":
            assert len(set(R._groups(c, b.pos[0], c.T - 1, m.ref64.scores[0, c.T - 1][1]))) >= 3, "three splits / key tiles"


# ---- the reference inside its bound --------------------------------------------------------------------------------------------------------
def test_reference_stands_inside_its_bound():
    """The fp32 run against the fp64 run: quotient <= 1/16 wherever the tolerance is not the 1e-3 ceiling (there: inside the bound),
    rings and written rows included.  The emulation of prefill_attn_bf16_kernel's operand planes passes with t_op, and t_op stays
    under the ceiling on every profile (`smax`)."""
    worst_planes, at_ceiling = 0.0, 0
    for c, profile, position in triples():
        b, m = measured(c, profile, position)
        got32 = R.reference(c, (b.K, b.V), b.qkv, b.pos, torch.float32, own=(m.ref64.k_row, m.ref64.v_row))
        ok, name, r = R.accept(got32, m.ref64, m.tol, b)
        assert ok, (c.name, profile, position, name, r, m.tol)
        if m.tol < R.TOL_CEIL:
            assert m.r32 <= m.tol / 16, (c.name, profile, position, m.r32, m.tol)
        else:
            at_ceiling += 1
        if c.entry == "prefill" and c.kv == "bf16":
            assert m.t_op < R.TOL_CEIL, (c.name, profile, position, m.t_op)
            emu = R.reference(c, (b.K, b.V), b.qkv, b.pos, torch.float64, planes=True)
            q = R.out_ratio(emu.out, m.ref64, c) / m.tol
            worst_planes = max(worst_planes, q)
            assert q <= 1.0, (c.name, profile, position, q)
    print(f"RATIO planes-emulation worst quotient {worst_planes:.3f}; {at_ceiling} triples at the 1e-3 ceiling")


# ---- the bound has teeth -------------------------------------------------------------------------------------------------------------------
# defect -> the (case, profile, position) that must reject it
CAUGHT_BY = {
    "window_wide_old": ("small-c64-d64-ctx", "peak@own", 63),
    "window_narrow_old": ("split-c130-d64-f32", "peak@oldest", 63),
    "own_hidden": ("split-c300-d128-f32", "peak@own", 100),
    "q1_visible": ("split-c130-d64-f32", "low", 129),
    "end_offset_ignored": ("pf-t1-w31-d64-f32", "flat", 0),          # the -pos clamp of the prefill kernels
    "own_stale": ("gemv-c3", "flat", 2),
    "no_rescale": ("pf-t33-w299-d128-bf16", "ramp_up", 0),
    "combine_unscaled": ("many-c2048-d64-f32", "peak@split_last", 600),
    "max_not_subtracted": ("many-c2048-d64-f32", "high", 600),
    "q_lo_dropped": ("pf-t33-w299-d128-bf16", "high", 0),
    "p_lo_dropped": ("pf-t32-w33-d64-bf16", "flat", 0),
    "kv_head_h": ("split-c300-d64-bf16-gqa2", "peak@oldest", 150),
    "shared_pos": ("ps-c130-d64-f32", "flat", (57, 129, 130, 397)),
    "ragged_row_appended": ("pf-ragged-d64-f32", "flat", (0, 100, 129, 397)),
    "rope_pos_not_t": ("pf-t31-w32-d128-f32", "low", 0),
    "own_unrounded": ("split-c130-d128-bf16", "ramp_up", 5),
}


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_defect_is_rejected(defect):
    name, profile, position = CAUGHT_BY[defect]
    c = R.resolve(R.BY_NAME[name], 256)
    assert profile in c.profiles and position in c.positions, "the case table no longer has the triple that catches this defect"
    b, m = measured(c, profile, position)
    got = R.reference(c, (b.K, b.V), b.qkv, b.pos, torch.float64, defect=defect)
    ok, what, r = R.accept(got, m.ref64, m.tol, b)
    print(f"defect {defect}: {name} {profile} {position}: {what} ratio {r:.3e} against tol {m.tol:.3e}")
    assert not ok
    sound = R.reference(c, (b.K, b.V), b.qkv, b.pos, torch.float32)
    assert R.accept(sound, m.ref64, m.tol, b)[0]


def test_every_defect_has_a_catcher():
    assert set(CAUGHT_BY) == set(R.DEFECTS)


# ---- coverage ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cus", CUS)
def test_case_table_names_every_reachable_instance(cus):
    named = set()
    for case in R.CASES:
        named |= R.case_names(case, cus)
        c = R.resolve(case, cus)
        assert c.B >= 1 and c.H % c.G == 0 and c.T <= c.cap
        if case.B == 0:          # the dense cases: the fewest streams that take the dense kernel on this device
            assert R.instance(case, cus).dense and not R.instance(R.replace(c, B=c.B - 1), cus).dense
        if c.rope != "off" and c.entry == "decode":
            assert max(max(R.stream_pos(c, p)) for p in c.positions) <= R.ROPE_POS_LIMIT
        if c.entry == "prefill" and c.kv == "bf16":
            assert c.smax == 31.0
    assert named == R.REACHABLE, sorted(R.REACHABLE - named)


def test_no_pair_is_skipped():
    assert len(SKIPPED_PAIRS) == 0
    assert len({(c.name, p) for c, p, _ in triples()}) == sum(len(c.profiles) for c in R.CASES)
    assert len({c.name for c in R.CASES}) == len(R.CASES)
