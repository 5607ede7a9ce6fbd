"""tests/helpers/utterance_attention_ref.py without a GPU: its fp64 reference against an independent formulation (oracle.mimi_oracle's
rope_interleaved + attention_mask + scaled_dot_product_attention in fp64; oracle.mimi_oracle.ring_attention for the ring walk), the
visibility rebuilt from `geometry` against the window definition, the designed scores of every (case, profile), the fp32 run of the
reference inside the bound, every listed defect rejected by a NAMED (case, profile) by a factor of ten, and the coverage of the
kernel's geometry by the case table."""
import pytest
import torch
import torch.nn.functional as F

from oracle import mimi_oracle as M
from tests.helpers import ring_attention_ref as R
from tests.helpers import utterance_attention_ref as U

_MEASURED = {}


def measured(c, profile):
    """(operands, fp64 / fp32 runs and tolerance) of one pair, shared by the tests of this module and left unchanged."""
    key = (c.name, profile)
    if key not in _MEASURED:
        b = U.build(c, profile)
        _MEASURED[key] = (b, U.measure(b))
    return _MEASURED[key]


def pairs():
    for c in U.CASES:
        for profile in c.profiles:
            yield c, profile


# ---- the reference --------------------------------------------------------------------------------------------------------------------------
def test_reference_is_the_oracles_attention():
    """Every case at `flat`: raw q / k through rope_interleaved (its own fp32 table, which `cpu_table` must reproduce byte for byte),
    attention_mask, SDPA in fp64."""
    for c in U.CASES:
        b, m = measured(c, "flat")
        q, k, v = b.q.double().contiguous(), b.k.double().contiguous(), b.v.double()
        if b.table is not None:
            q, k = M.rope_interleaved(q, k, 0, U.MAX_PERIOD)
        want = F.scaled_dot_product_attention(q, k, v, M.attention_mask(c.T, c.context), dropout_p=0.0).permute(0, 2, 1, 3)
        assert want.dtype == torch.float64
        assert float((m.ref64.out - want).abs().max()) <= 1e-12, c.name
        assert torch.equal(m.ref64.mask, M.attention_mask(c.T, c.context))


@pytest.mark.parametrize("name", R.WALK_CASES)
def test_ring_reference_is_the_oracles_ring_attention(name):
    """The ring walk at `flat`: the ring as that many positions left it, then oracle.mimi_oracle.ring_attention appending the T new rows
    (the same bytes the ring already holds there) in fp64.  A query without a visible key (T = cap: its own slot counts as the future)
    is 0 in the reference; what the oracle's softmax makes of an empty row is not compared."""
    c = R.BY_NAME[name]
    for position in c.positions:
        b = R.build(c, "flat", position)
        ref = U.reference(c, b, torch.float64)
        P = b.pos[0]
        ring = M.RingKVCache(c.B, c.H, c.D, c.cap)
        ring.k, ring.v, ring.end_offset = b.K.double().clone(), b.V.double().clone(), P
        slots = (P + torch.arange(c.T)) % c.cap
        want = M.ring_attention(b.qkv.double(), ring.k[:, :, slots].clone(), ring.v[:, :, slots].clone(), ring, P, c.context, None)
        want = want.view(c.B, c.T, c.H, c.D)
        for bi in range(c.B):
            for t in range(c.T):
                if (bi, t) in ref.scores:
                    assert float((ref.out[bi, t] - want[bi, t]).abs().max()) <= 1e-12, (name, position, t)
                else:
                    assert c.T == c.cap and t == 0 and float(ref.out[bi, t].abs().max()) == 0.0


def test_geometry_walk_is_the_window_definition():
    """The (query, key) pairs the kernel's staged / skipped / interior / masked walk lets through are the window's, on every case and on
    every T up to 70 with the contexts around a tile."""
    shapes = {(c.T, c.context) for c in U.CASES} | {(T, ctx) for T in range(1, 71) for ctx in (None, 1, 31, 32, 33, 64)}
    for T, ctx in sorted(shapes, key=str):
        assert torch.equal(U.kernel_mask(T, ctx), U.window_mask(T, ctx)), (T, ctx)
        assert torch.equal(U.window_mask(T, ctx), M.attention_mask(T, ctx))


# ---- the designed scores --------------------------------------------------------------------------------------------------------------------
def test_designed_scores():
    """Every (case, profile): the achieved score of every visible (query, key) within 0.5 of the key's target, the ramps strictly
    monotone inside a period for every query, `low` / `high` inside their bands, the stairs' peaks >= 25 above their background."""
    n = 0
    for c, profile in pairs():
        b, m = measured(c, profile)
        assert all(bool(torch.isfinite(x).all()) for x in (b.q, b.k, b.v)) and bool(torch.isfinite(m.ref64.out).all())
        sc, tg = m.ref64.scores, b.targets
        assert float((sc - tg.view(1, 1, 1, -1)).abs().max()) <= 0.5, (c.name, profile)
        if profile in ("low", "high"):
            lo, hi = (80.0, 90.0) if profile == "high" else (-90.0, -80.0)
            assert lo <= float(sc.min()) and float(sc.max()) <= hi, (c.name, profile)
        if profile.startswith("ramp") and c.T > 1:
            Wd = c.context or c.T
            d = sc.diff(dim=-1) * (-1.0 if profile == "ramp_down" else 1.0)
            inside = (torch.arange(1, c.T) % Wd) != 0
            if Wd > 1:
                assert float(d[..., inside].min()) > 0.0, (c.name, profile)
                if bool((~inside).any()):          # the resets
                    assert float(d[..., ~inside].max()) < 0.0, (c.name, profile)
            span = 110.0 if profile == "ramp_wide" else 60.0
            if c.T >= Wd > 1:
                assert float((sc.max(-1).values - sc.min(-1).values).min()) >= span - 1.0, (c.name, profile)
        if profile.startswith("stairs"):
            j = torch.arange(c.T)
            peak = ((j // 32) % 3 == 0) & (j % 32 == (0 if profile == "stairs_first" else 31))
            if bool(peak.any()):
                assert float(sc[..., peak].min()) >= 29.5, (c.name, profile)
            if bool((~peak).any()):
                assert float(sc[..., ~peak].abs().max()) <= 2.0, (c.name, profile)
        n += 1
    assert n == len(U.CASES) * len(U.PROFILES)


# ---- the reference inside its bound --------------------------------------------------------------------------------------------------------
def test_reference_stands_inside_its_bound():
    """16 r32 <= 1e-3 on every (case, profile): the tolerance is never the ceiling's to give, and the fp32 run is accepted."""
    worst = (0.0, ("", ""))
    for c, profile in pairs():
        b, m = measured(c, profile)
        assert U.TOL_FACTOR * m.r32 <= U.TOL_CEIL, (c.name, profile, m.r32)
        assert U.TOL_FLOOR <= m.tol <= U.TOL_CEIL
        assert U.accept(m.ref32.out, m.ref64, m.tol)[0]
        worst = max(worst, (m.r32, (c.name, profile)))
    print(f"RATIO worst fp32 reference ratio {worst[0]:.3e} at {worst[1]}")


# ---- the bound has teeth -------------------------------------------------------------------------------------------------------------------
# defect -> the (case, profile[, position]) that must reject it by a factor of ten
CAUGHT_BY = {
    "no_rescale_o": ("plain-t545-d128", "ramp_up"),
    "no_rescale_l": ("fused-t700-c250-d64", "stairs_last"),
    "causal_plus_one": ("fused-t321-d128", "ramp_up"),
    "context_plus_one": ("fused-t700-c40-d32", "ramp_down"),
    "context_minus_one": ("plain-t700-c33-d32", "ramp_down"),
    "diagonal_as_interior": ("plain-t256-d64", "ramp_wide"),
    "context_edge_as_interior": ("fused-t700-c250-d128", "ramp_down"),
    "stage_one_tile_late": ("plain-t700-c250-d64", "stairs_first"),
    "stage_one_tile_short": ("fused-t257-d64", "flat"),
    "twin_tiles_swapped": ("plain-t161-d64", "ramp_up"),
    "wrong_head_v": ("fused-norope-t1-d128", "flat"),
    "table_row_of_tile_start": ("fused-t33-d32", "high"),
    "q1_slot_visible": ("walk-c250-d64-t12", "low", 245),
    "unwritten_slot_visible": ("walk-c70-d128-t40", "flat/k0", 0),
}


@pytest.mark.parametrize("defect", U.DEFECTS)
def test_defect_is_rejected(defect):
    name, profile, *position = CAUGHT_BY[defect]
    if position:
        c = R.BY_NAME[name]
        assert profile in c.profiles and position[0] in c.positions
        b = R.build(c, profile, position[0])
        m = R.measure(b)
        r = R.out_ratio(U.reference(c, b, torch.float64, defect).out, m.ref64, c)
        sound = R.out_ratio(m.ref32.out, m.ref64, c)
    else:
        c = U.BY_NAME[name]
        assert profile in c.profiles
        b, m = measured(c, profile)
        r = U.out_ratio(U.reference(c, b, torch.float64, defect).out, m.ref64)
        sound = m.r32
    print(f"defect {defect}: {name} {profile} {position}: ratio {r:.3e} against tol {m.tol:.3e}")
    assert r >= 10 * m.tol
    assert sound <= m.tol


def test_every_defect_has_a_catcher():
    assert set(CAUGHT_BY) == set(U.DEFECTS)
    assert set(U.RING_DEFECTS.values()) <= set(R.DEFECTS)


# ---- coverage ------------------------------------------------------------------------------------------------------------------------------
def test_case_table_covers_the_geometry():
    seen = set()
    for c in U.CASES:
        geo = U.geometry(c.T, c.context)
        assert len(geo) == 2 * -(-c.T // 256)
        for wg in geo:
            if wg.s_begin > 0:
                seen.add("s_begin>0")
                assert wg.group >= 1 or (wg.twin == 1 and c.context <= 32), "the first group stages from key 0 unless the twin's first tile cannot see it"
            if wg.l_last < 0:
                seen.add("twin without a tile")
                assert wg.hi_wg == -1 and not wg.staged and not any(w.has_q for w in wg.waves)
            for w in wg.waves:
                if not w.has_q:
                    seen.add("wave without a query")
                    assert not w.interior and not w.masked
                    continue
                if w.interior and w.masked:
                    seen.add("interior and masked tiles in one wave")
                vis = U.window_mask(c.T, c.context)[w.q0:w.q0 + 32]
                for s0 in w.masked:
                    per_query = vis[:, s0:s0 + 32].sum(-1)
                    if s0 + 31 < w.q0 and int(per_query[0]) == 1 and int(per_query.sum()) == 1:
                        seen.add("a tile with exactly one visible key")          # for the wave's first query, none for the others
                    if s0 + 31 < w.q0 and int(per_query[-1]) == 1:
                        seen.add("a tile with one visible key for the last query")
                    if int(per_query.min()) == 0 and s0 == w.masked[0]:
                        seen.add("a lane whose first tile is all masked")
                if c.context and any(s0 < w.lo for s0 in w.skipped) and any(s0 + 32 == w.lo for s0 in w.skipped):
                    seen.add("a skipped tile at the context edge")
        seen.add((c.entry, c.D))
        seen.add("T<32" if c.T < 32 else "T=32" if c.T == 32 else "T>32")
        seen.add("T<256" if c.T < 256 else "T=256" if c.T == 256 else "T>256")
    want = {"s_begin>0", "twin without a tile", "wave without a query", "a tile with exactly one visible key",
            "a skipped tile at the context edge", "interior and masked tiles in one wave", "a tile with one visible key for the last query",
            "a lane whose first tile is all masked", "T<32", "T=32", "T>32", "T<256", "T=256", "T>256"}
    want |= {(e, D) for e in ("plain", "fused") for D in (32, 64, 128)}
    assert seen == want, sorted(map(str, want - seen))
    assert {(c.entry, c.rope) for c in U.CASES} == {("plain", False), ("fused", True), ("fused", False)}
    # the issue's shapes, and the third group's first staged tile under the codec's context
    shapes = {(c.T, c.context) for c in U.CASES}
    assert shapes >= {(T, None) for T in (1, 31, 32, 33, 225, 256, 257, 321, 545)} | {(700, x) for x in (250, 40, 34, 33, 32, 1)} | {(33, 250)}
    assert sorted(wg.s_begin for wg in U.geometry(700, 250) if wg.group == 2) == [256, 288]
    assert [wg.l_last for wg in U.geometry(257, None)][2:] == [0, -1]
    assert [wg.l_last for wg in U.geometry(321, None)][2:] == [2, 1]
    assert len({c.name for c in U.CASES}) == len(U.CASES)


def test_ring_walk_cases_take_this_kernel():
    """The walk cases are the ones ops.attention(ring=True) sends to attention_kernel, every D; the older qpre cases are not."""
    kernels = {}
    for c in R.CASES:
        if c.entry == "qpre":
            kernels[c.name] = R.instance(c, 256).kernel
    assert {n for n, k in kernels.items() if k.endswith(":ring")} == set(R.WALK_CASES)
    assert {kernels[n] for n in R.WALK_CASES} == {f"attention<{D}>:ring" for D in (32, 64, 128)}
    for n in R.WALK_CASES:
        assert "flat/k0" in R.BY_NAME[n].profiles and "flat" in R.BY_NAME[n].profiles
