"""ops.lm_sample read out rank by rank: every kernel rst_launch_lm_sample dispatches to (sample_kernel<256, 8 | 16>, <1024, 32>, split +
merge, sample_big_kernel by the candidate cap and by two_level=False, the nucleus sampler) against the plain reference of
tests/helpers/sampler_readout.py, through noise that is designed instead of drawn.  Row r of a readout launch has noise 2^-40 at sorted
position r and 2^40 elsewhere, so its token is the candidate the kernel ranked r-th: the rows of a launch spell out the kernel's
ordered top-k, the threshold, the tie break and the tail included.  The pair races put two ranks 2^-12 apart and pin the race terms.
Every assertion is exact equality of tokens.  tests/test_sampler_readout_cpu.py checks, without a GPU, that the inputs meet the
conditions under which this is valid and that emulated defects fail these same assertions."""
import pytest
import torch

from rstnet_amd import ops
from tests.helpers import sampler_readout as SR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _sample(l, noise, temp, k, *, limit=0, two_level=True, **kw):
    logits = l.to(DEV)[None].expand(noise.shape[0], -1).contiguous()
    return ops.lm_sample(logits, use_sampling=True, temp=temp, top_k=k, noise=noise.to(DEV), limit=limit, two_level=two_level, **kw).cpu()


def _assert_tokens(tok, exp, what):
    bad = (tok != exp).nonzero().flatten()
    assert bad.numel() == 0, (what, f"{bad.numel()} of {exp.numel()} rows", [(int(r), int(tok[r]), int(exp[r])) for r in bad[:8]])


def _readout(c, kind, l, temp):
    ref = SR.reference(l, temp, c.limit, c.k)
    noise = SR.readout_noise(SR.read_ranks(ref.order.numel()), ref.order.numel())
    exp = SR.expected(ref, noise)
    for two_level, inst in SR.routes_of(c):
        _assert_tokens(_sample(l, noise, temp, c.k, limit=c.limit, two_level=two_level), exp, (c, kind, inst))
    return ref, noise, exp


@pytest.mark.parametrize("c", SR.TOPK_CASES, ids=SR.case_id)
def test_topk_readout(c):
    """Kinds (a) distinct, (b) five equal values around the threshold, (c) plateaus of three values and one value: the token of every
    read rank is the reference's order[r] (stable descending sort of the fp32 probabilities, ids >= limit blanked)."""
    for kind, l, temp in SR.kind_rows(c):
        _readout(c, kind, l, temp)


@pytest.mark.parametrize("c", [c for c in SR.TOPK_CASES if SR.k_eff(c.V, c.k, c.limit) >= 2], ids=SR.case_id)
def test_topk_pair_race(c):
    """noise[r1] = 1 against noise[r2] = p[r2] / p[r1] * (1 +- 2^-12): r1 wins the (+) row and r2 the (-) row, at three temperatures."""
    l = SR.row_distinct(c.V, c.limit)
    for temp in SR.PAIR_TEMPS:
        ref = SR.reference(l, temp, c.limit, c.k)
        noise, win = SR.pair_noise(ref, SR.pair_ranks(ref, c.V + c.k))
        for two_level, inst in SR.routes_of(c):
            _assert_tokens(_sample(l, noise, temp, c.k, limit=c.limit, two_level=two_level), win, (c, temp, inst))


@pytest.mark.parametrize("c", SR.EXTRA_CASES, ids=SR.case_id)
def test_readout_few_live_keys_signed_zeros_wide_range(c):
    """Kinds (d) all but k / 2 ids at -inf or -3.4e38 (ranks of probability 0 cannot be read: their rows take the reference's token),
    (e) +0.0, -0.0 and denormals (-0.0 ties with +0.0, lowest id first), (f) -50 + 10 * randn."""
    for kind, l, temp in SR.extra_rows(c):
        _readout(c, kind, l, temp)


@pytest.mark.parametrize("c", SR.COLLAPSED_CASES, ids=SR.case_id)
def test_deviation_collapsed_probabilities_rank_by_scaled_logit(c):
    """Row (g): eight consecutive fp32 logits, increasing with the id, whose fp32 probabilities are one number.  The reference ranks
    them by id; the kernels compare (scaled logit, id) keys and rank them by value -- with k = 4 the two top-k SETS differ.  This is
    where "the oracle's tokens" ends; what is pinned here is the kernels' order."""
    l, ids = SR.row_collapsed(c.V)
    ref = SR.reference(l, 1.0, 0, c.k)
    by_key = SR.key_order(ref)
    noise = SR.readout_noise(list(range(c.k)), c.k)
    assert not torch.equal(by_key, SR.expected(ref, noise))
    for two_level, inst in SR.routes_of(c):
        _assert_tokens(_sample(l, noise, 1.0, c.k, two_level=two_level), by_key, (c, inst))


@pytest.mark.parametrize("V", SR.GREEDY_V)
def test_greedy_is_argmax_lowest_id(V):
    rows = SR.greedy_rows(V)
    for two_level in (True, False) if V > 32768 else (True,):
        tok = ops.lm_sample(rows.to(DEV), use_sampling=False, temp=SR.T_READ, top_k=25, two_level=two_level).cpu()
        _assert_tokens(tok, rows.argmax(-1), (V, two_level))
    # temp = 0 is greedy too, whatever use_sampling says
    tok = ops.lm_sample(rows.to(DEV), use_sampling=True, temp=0.0, top_k=25).cpu()
    _assert_tokens(tok, rows.argmax(-1), (V, "temp 0"))


@pytest.mark.parametrize("nc", SR.NUCLEUS_CASES, ids=lambda nc: f"V{nc.V}-m{nc.m}")
def test_nucleus_readout(nc):
    """Sorted positions 0 .. m + 1 of a nucleus of m entries: the first m are drawn in the reference's order, the two behind the end are
    not (their rows fall back to position 0).  Row (a) and its quantised image, without and with id blanking, top_k = 25 alongside."""
    temp = SR.T_NUCLEUS
    for kind, l in SR.nucleus_rows(nc.V):
        for limit in (0, nc.V // 2):
            top_p, m = SR.nucleus_top_p(l, temp, limit, nc.m)
            ps, idx, _ = SR.nucleus_reference(l, temp, limit, top_p)
            noise = SR.readout_noise(list(range(min(m + 2, nc.V))), nc.V)
            exp = SR.nucleus_expected(ps, idx, noise)
            noise = noise.to(DEV)
            for top_k in (0, 25):
                _assert_tokens(_sample(l, noise, temp, top_k, limit=limit, top_p=top_p), exp, (nc, kind, limit, top_k))


# ---- argument plumbing: how lm/model.py, lm/generate.py and lm/depth_frame.py call the sampler ----------------------------------------
PLUMBING = [SR.Case(SR.S8, 2048, 250, 2000), SR.Case(SR.S16, 2050, 250, 2049), SR.Case(SR.S32, 32000, 25, 30000), SR.Case(SR.SPLIT, 40961, 25, 10241)]


@pytest.mark.parametrize("c", PLUMBING, ids=SR.case_id)
def test_noise_slice_out_column_and_device_limit(c):
    l = SR.row_distinct(c.V, c.limit)
    ref = SR.reference(l, SR.T_READ, c.limit, c.k)
    kk = ref.order.numel()
    noise = SR.readout_noise(SR.read_ranks(kk), kk)
    exp = SR.expected(ref, noise)
    B = noise.shape[0]
    logits = l.to(DEV)[None].expand(B, -1).contiguous()
    # noise as a column slice of a wider buffer; whatever surrounds the slice would win every race if it were read
    wide = torch.full((B, kk + 16), SR.LO * 2.0 ** -20, device=DEV)
    wide[:, 7:7 + kk] = noise.to(DEV)
    # out as a column of an int64 [B, 3] buffer
    limit_dev = torch.tensor([c.limit], dtype=torch.int32, device=DEV)
    for two_level, inst in SR.routes_of(c):
        for lim in (dict(limit=c.limit), dict(limit_dev=limit_dev)):
            out = torch.full((B, 3), -7, dtype=torch.int64, device=DEV)
            ret = ops.lm_sample(logits, use_sampling=True, temp=SR.T_READ, top_k=c.k, noise=wide[:, 7:7 + kk], out=out[:, 1], two_level=two_level, **lim)
            assert ret.data_ptr() == out[:, 1].data_ptr()
            _assert_tokens(out[:, 1].cpu(), exp, (c, inst, list(lim)))
            assert bool((out[:, 0] == -7).all()) and bool((out[:, 2] == -7).all())


def test_candidate_stage_limits_are_errors():
    """k = 8192 at V = 32768 (64 KiB of candidate list next to the static scratch) launches and is read out in test_topk_readout; one
    more candidate, or more than 1024 above 32768 ids, is refused by the launcher before anything runs."""
    for V, k in ((32768, 8193), (32769, 1025), (32769, 0)):
        assert SR.k_eff(V, k, 0) > (SR.K_STAGE if V <= 32768 else SR.BIG_K)
        logits = torch.zeros(1, V, device=DEV)
        out = torch.full((1,), -7, dtype=torch.int64, device=DEV)
        with pytest.raises((ValueError, RuntimeError), match="top-k"):
            ops.lm_sample(logits, use_sampling=True, temp=1.0, top_k=k, noise=torch.ones(1, SR.k_eff(V, k, 0), device=DEV), out=out)
        assert int(out[0]) == -7
