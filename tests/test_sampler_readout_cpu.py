"""tests/helpers/sampler_readout.py held to account without a GPU: the case tables reach the kernel instances they name, the designed
inputs meet the conditions under which a readout is valid (the oracle's own sample_token reads back the stable descending order through
them), and a torch sampler carrying one defect at a time fails the assertion that tests/test_sampler_readout_gpu.py makes -- while the
seeded random-noise inputs of tests/test_lm_gpu.py::test_sampling_matches_oracle let the boundary, tail and tie defects through."""
import pytest
import torch

from oracle import lm_oracle as L
from tests.helpers import sampler_readout as SR

ORACLE_ROWS = 24          # rows of a readout that also go through the oracle above 32768 ids (its topk sorts every row it is given)


def _thin(rows, V):
    return rows if V <= 32768 or len(rows) <= ORACLE_ROWS else rows[::len(rows) // ORACLE_ROWS]


def _oracle(l, temp, k, noise):
    return L.sample_token(l[None].expand(noise.shape[0], -1), True, temp, k, noise)


def test_tables_reach_the_instances_they_name():
    for c in SR.TOPK_CASES + SR.EXTRA_CASES + SR.COLLAPSED_CASES:
        for two_level, inst in SR.routes_of(c):
            assert SR.route(c.V, c.k, two_level=two_level) == inst, (c, two_level)
        assert len(SR.read_ranks(SR.k_eff(*c[1:]))) * c.V <= SR.MAX_ELEMS, c
    assert {c.inst for c in SR.TOPK_CASES} == {c.inst for c in SR.EXTRA_CASES} == {SR.S8, SR.S16, SR.S32, SR.SPLIT, SR.BIG}
    # the thresholds of the launcher, from both sides
    for V, inst in ((2048, SR.S8), (2049, SR.S16), (4096, SR.S16), (4097, SR.S32), (32768, SR.S32), (32769, SR.SPLIT)):
        assert SR.route(V, 25) == inst and SR.route(V, 25, sampling=False) == inst
        assert (V, inst) in {(c.V, c.inst) for c in SR.TOPK_CASES}
    assert SR.route(151936, 273) == SR.SPLIT and SR.route(151936, 274) == SR.BIG and 15 * 273 <= SR.SPLIT_CAP < 15 * 274
    assert SR.route(151936, 1024, sampling=False) == SR.SPLIT and SR.route(151936, 25, two_level=False) == SR.BIG
    assert SR.route(32768, 8192) == SR.S32
    for V, k in ((32768, 8193), (32769, 1025), (32769, 0)):
        with pytest.raises(ValueError):
            SR.route(V, k)
    assert SR.route(151936, 25, top_p=0.5) == SR.TOP_P and SR.route(151936, 25, top_p=0.5, sampling=False) == SR.SPLIT
    # chunk geometry of the split + merge rows: last chunks of 2049 ids and of one id
    assert 32769 - 3 * SR.SPLIT_CHUNK == 2049 and 40961 - 4 * SR.SPLIT_CHUNK == 1
    assert SR.GREEDY_V == sorted({1, 2, 50, 2047, 2048, 2049, 2050, 4096, 4097, 32000, 32768, 32769, 40961, 65536, 151936})


def _assert_same_order(ref, limit, what):
    assert torch.equal(ref.order, SR.key_order(ref, limit)), (what, "the order by probability is not the order by scaled logit")


def _assert_readout(c, kind, l, temp, oracle):
    """Conditions of one readout launch; returns (ref, ranks, noise, expected tokens)."""
    ref = SR.reference(l, temp, c.limit, c.k)
    kk = ref.order.numel()
    assert kk == SR.k_eff(c.V, c.k, c.limit)
    _assert_same_order(ref, c.limit, (c, kind))
    ranks = SR.read_ranks(kk)
    noise = SR.readout_noise(ranks, kk)
    exp = SR.expected(ref, noise)
    live = ref.probs[ref.order[ranks]] > 0
    assert torch.equal(exp[live], ref.order[ranks][live]), (c, kind)
    if oracle:
        p = ref.p64[ref.order[ranks]]
        assert bool((ref.p64.max() / p < 2.0 ** 60).all()), (c, kind, "a read rank is not live")
        assert bool(live.all())
        if not c.limit:        # the oracle has no id blanking
            rows = _thin(list(range(len(ranks))), c.V)
            assert torch.equal(_oracle(l, temp, kk, noise[rows]), ref.order[ranks][rows]), (c, kind, "the oracle's own readout")
    return ref, ranks, noise, exp


def _caught(l, temp, c, noise, exp, defect):
    return not torch.equal(SR.emulate(l, temp, c.limit, c.k, noise, defect), exp)


@pytest.mark.parametrize("c", SR.TOPK_CASES, ids=SR.case_id)
def test_topk_case_is_valid_and_catches_the_defects(c):
    n, kk = SR.live_ids(c.V, c.limit), SR.k_eff(c.V, c.k, c.limit)
    kinds = SR.kind_rows(c)
    assert ("b" in [k for k, _, _ in kinds]) == (kk < n)
    for kind, l, temp in kinds:
        ref, ranks, noise, exp = _assert_readout(c, kind, l, temp, oracle=kind == "a")
        assert torch.equal(SR.emulate(l, temp, c.limit, c.k, noise), exp)            # the emulation without a defect is the reference
        if kind == "a":
            assert _caught(l, temp, c, noise, exp, "swap_last_two") == (kk >= 2)
            assert _caught(l, temp, c, noise, exp, "swap_2_3") == (kk >= 4)
            if c.limit:
                assert int(l.argmax()) >= n and _caught(l, temp, c, noise, exp, "blanked_stay")
        if kind == "b":
            # five equal values (four at k = 1) around the threshold, of which the top-k takes the lowest ids; spread over the row
            pos = SR.tie_positions(c.V, c.k, c.limit)
            srt = torch.argsort(l[:n], descending=True, stable=True)
            ids = srt[pos]
            assert bool((l[ids] == l[ids[0]]).all()) and int((l[:n] == l[ids[0]]).sum()) == len(pos)
            assert 0 < kk - pos[0] < len(pos)                                         # need < n_eq: the index search runs
            assert ids.tolist() == sorted(SR.tie_targets(n, len(pos)))
            if n >= 1024:
                assert len({int(i) % 64 for i in ids}) > 1 and len({int(i) % 256 // 64 for i in ids}) > 1
            if n > 2 * SR.SPLIT_CHUNK:
                assert len({int(i) // SR.SPLIT_CHUNK for i in ids}) >= 3
        if kind in ("b", "c1") or (kind == "c3" and n >= 50):
            if kk < n:
                assert _caught(l, temp, c, noise, exp, "kth_is_next"), (c, kind)
            if n >= 2:
                assert _caught(l, temp, c, noise, exp, "ties_to_highest_id"), (c, kind)
    # the pair race, on (a)
    l = SR.row_distinct(c.V, c.limit)
    for temp in SR.PAIR_TEMPS:
        ref = SR.reference(l, temp, c.limit, c.k)
        pairs = SR.pair_ranks(ref, c.V + c.k)
        assert bool(pairs) == (kk >= 2)
        if not pairs:
            continue
        _assert_same_order(ref, c.limit, (c, "pair", temp))
        noise, win = SR.pair_noise(ref, pairs)
        assert len(pairs) >= 3 and not torch.equal(win[0::2], win[1::2])
        used = ref.order[torch.tensor(pairs).flatten()]
        assert float((ref.scaled.max() - ref.scaled[used]).max()) <= 40.0            # the range the 2^-12 margin was budgeted for
        assert torch.equal(SR.expected(ref, noise), win), (c, temp, "the fp32 reference does not decide the pairs as designed")
        if not c.limit:
            assert torch.equal(_oracle(l, temp, kk, noise), win), (c, temp, "the fp32 oracle does not decide the pairs as designed")
        if temp != 1.0:
            assert _caught(l, temp, c, noise, win, "no_temperature"), (c, temp)


@pytest.mark.parametrize("c", SR.EXTRA_CASES, ids=SR.case_id)
def test_extra_kinds_are_valid(c):
    kk = SR.k_eff(c.V, c.k, c.limit)
    for kind, l, temp in SR.extra_rows(c):
        ref, ranks, noise, exp = _assert_readout(c, kind, l, temp, oracle=kind == "f")
        if kind.startswith("d"):
            m = int((ref.probs > 0).sum())
            assert 0 < m < kk and int((ref.probs[ref.order[ranks]] == 0).sum()) > 0
            assert bool((l[l < -1e30] == (float("-inf") if kind == "d-inf" else -3.4e38)).all())
            assert bool(torch.isfinite(ref.scaled).all()) == (kind != "d-inf")       # temp = 1 keeps -3.4e38 finite
        if kind.startswith("e"):
            z = l == 0
            assert int((z & torch.signbit(l)).sum()) > 0 and int((z & ~torch.signbit(l)).sum()) > 0
            assert int(((l != 0) & (l.abs() < 2.0 ** -126)).sum()) > 0 and len(set(ref.order.tolist())) == kk
            if kind == "e-zero":     # the maximum is the zero plateau and begins with -0.0
                assert float(l.max()) == 0.0 and bool(torch.signbit(l[0])) and int(l.argmax()) == 0


@pytest.mark.parametrize("V", SR.GREEDY_V)
def test_greedy_rows(V):
    rows = SR.greedy_rows(V)
    assert rows.shape[1] == V and not bool(torch.isnan(rows).any())
    # argmax: lowest id on ties, signed zeros included
    for r in rows:
        assert int(r.argmax()) == int((r == r.max()).nonzero()[0])


@pytest.mark.parametrize("c", SR.COLLAPSED_CASES, ids=SR.case_id)
def test_collapsed_row_separates_the_two_orders(c):
    """Row (g): the reference ranks the run by id, a sampler that compares scaled logits ranks it by value."""
    l, ids = SR.row_collapsed(c.V)
    ref = SR.reference(l, 1.0, 0, c.k)
    assert len(set(l[ids].tolist())) == SR.COLLAPSED_RUN and bool((torch.diff(l[ids]) > 0).all())
    assert len(set(ref.probs[ids].tolist())) == 1 and float(ref.probs[ids][0]) > float(ref.probs.sum() - ref.probs[ids].sum())
    assert torch.equal(ref.order, ids[:c.k])
    assert torch.equal(SR.key_order(ref), ids.flip(0)[:c.k])
    assert (set(ref.order.tolist()) == set(SR.key_order(ref).tolist())) == (c.k == SR.COLLAPSED_RUN)


@pytest.mark.parametrize("nc", SR.NUCLEUS_CASES, ids=lambda nc: f"V{nc.V}-m{nc.m}")
def test_nucleus_case_is_valid(nc):
    temp = SR.T_NUCLEUS
    for kind, l in SR.nucleus_rows(nc.V):
        for limit in (0, nc.V // 2):
            top_p, m = SR.nucleus_top_p(l, temp, limit, nc.m)
            ps, idx, p64 = SR.nucleus_reference(l, temp, limit, top_p)
            assert int((ps > 0).sum()) == m and bool((ps[:m] > 0).all()), (kind, limit)
            excl = torch.cat([torch.zeros(1, dtype=torch.float64), torch.cumsum(p64, 0)])
            assert abs(float(excl[m - 1]) - top_p) > 1e-5 and abs(float(excl[m]) - top_p) > 1e-5, (kind, limit)
            # the sampler sorts (scaled logit, id): the same order over the nucleus and the two positions behind it
            n = SR.live_ids(nc.V, limit)
            by_key = torch.argsort((l / temp)[:n], descending=True, stable=True)
            assert torch.equal(by_key[:m + 2], idx[:min(m + 2, n)]), (kind, limit)
            positions = list(range(min(m + 2, nc.V)))
            assert len(positions) * nc.V <= SR.MAX_ELEMS
            rows = _thin(positions, nc.V)
            noise = SR.readout_noise(rows, nc.V)
            exp = SR.nucleus_expected(ps, idx, noise)
            want = torch.stack([idx[r] if r < m else idx[0] for r in rows])      # positions past the nucleus are not drawn
            assert torch.equal(exp, want), (kind, limit)
            if not limit:
                assert torch.equal(L.sample_token(l[None].expand(len(rows), -1), True, temp, 0, noise, top_p=top_p), want), (kind, limit)
    if nc.V == 2048 and nc.m == 300:
        assert int((ps[:m].unique(return_counts=True)[1] > 1).sum()) > 0             # the quantised row has plateaus inside the nucleus


def test_random_noise_inputs_miss_boundary_tail_and_tie_defects():
    """Why the readout exists: the inputs of test_lm_gpu.py::test_sampling_matches_oracle (8 (V, k) cases, 3 rows, one seeded Exp(1)
    draw each) through the emulated sampler.  A defect at the k-th candidate, in the order of the tail or in the direction of the tie
    break changes no token of any case; only a swap near the top does, in some."""
    caught = {d: 0 for d in SR.DEFECTS[:4]}
    for V, k in [(2048, 250), (32, 7), (32000, 25), (50, 25), (4000, 250), (151936, 25), (40000, 300), (151936, 1000)]:
        g = torch.Generator().manual_seed(V)
        logits = torch.randn(3, V, generator=g) * 3
        logits[0, 5] = logits[0, 3]
        noise = torch.empty(3, k).exponential_(1, generator=g)
        ref = L.sample_token(logits, True, 0.8, k, noise)
        for d in caught:
            got = torch.stack([SR.emulate(logits[b], 0.8, 0, k, noise[b:b + 1], d)[0] for b in range(3)])
            caught[d] += int(not torch.equal(got, ref))
        assert torch.equal(torch.stack([SR.emulate(logits[b], 0.8, 0, k, noise[b:b + 1])[0] for b in range(3)]), ref)
    assert caught["kth_is_next"] == caught["swap_last_two"] == caught["ties_to_highest_id"] == 0, caught
    assert 0 < caught["swap_2_3"] < 8, caught
