"""Every step of the persistent depth-frame launch (csrc/lm_depth.hip, rst_depth_decode_frame behind ops.depth_decode_frame) and of its
one-workgroup repair launch against an fp64 reference, at the smallest shapes that turn each loop of the kernel
(tests/helpers/depth_frame_ref.py: the case table, `grid`), plus an exact readout of the in-kernel sampler's plumbing.

A launch keeps one step's logits at a time, so step q - 1 is read out of the hand-off workspace after a launch over the first q steps'
weights (`prefix_tables`): with the full frame's ring capacity that launch computes what the full one computes up to there, and its
tokens are asserted to be the full launch's.  The reference is teacher-forced with the kernel's own tokens, so no assertion hangs on
a near-tie; the tokens themselves are checked against the read-back logits, exactly.

Bound, per (step, batch row) vector: max |got - ref64| <= tol * max |ref64|, tol = 16 x the same ratio of the reference run in fp32,
within [2^-18, 1e-3] (depth_frame_ref.tolerance).  Every comparison prints a `RATIO` line (run with -s): the kernel's worst ratio, the
fp32 reference's and their quotient; the same figures are in the assertion messages."""
import pytest
import torch

from rstnet_amd import ops
from tests.helpers import depth_frame_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture
def clean_health():
    yield
    ops.persistent_rearm(DEV)          # the repair counters of this test must not retire the path for later tests


_BUILT = {}


def _build(name):
    """Operands, device tables and the workspace of one case; one case is kept at a time (the wide ones hold ~100 MB)."""
    if name not in _BUILT:
        _BUILT.clear()
        co = R.make_case(R.BY_NAME[name])
        _BUILT[name] = (co, R.device_tables(co, DEV))
    return _BUILT[name]


@pytest.fixture(scope="module", params=[c.name for c in R.CASES])
def built(request):
    """Module scope: pytest groups the tests of one case, so its operands are built once."""
    return _build(request.param)


def _check_shape(c):
    assert ops.depth_frame_supported(c.B, c.E, c.H, c.Hd, c.card, c.Q, c.L, c.top_k, device=DEV), f"{c.name}: not served by the persistent launch"
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    here, meant = R.grid(c, cus), R.grid(c, 256)
    assert here.ok and here.flags >= meant.flags, \
        f"{c.name}: on {cus} CUs the grid is {here.G} (not {meant.G}) and the case no longer takes {sorted(meant.flags - here.flags)}"


def _handoff(c, solo=False):
    return R.read_handoff(R.workspace(ops, c.B, c.E, c.Hd, c.card), c, c.B, solo=solo)


def _lowest_argmax(row):
    return int((row == row.max()).nonzero()[0])


def _frame_and_prefixes(d, **kw):
    """The full launch, then the prefixes q = 1 .. Q: (tokens [B, Q + 1 (+ pad)], hand-off of the full launch, per-step logits
    [Q, B, card]); prefix tokens and the last prefix's logits are asserted to be the full launch's."""
    c = d.case
    tokens = R.launch(d, d.full, **kw)
    full = _handoff(c)
    assert d.full.status.tolist() == [0, 0, 0, 0], f"{c.name}: hand-offs timed out: {d.full.status.tolist()}"
    logits = []
    for q in range(1, c.Q + 1):
        t = R.prefix_tables(d, q)
        tq = R.launch(d, t, **kw)
        assert t.status.tolist() == [0, 0, 0, 0], f"{c.name}: prefix {q}: hand-offs timed out: {t.status.tolist()}"
        assert torch.equal(tq[:, :q + 1], tokens[:, :q + 1]), f"{c.name}: prefix {q} drew {tq[:, 1:q + 1].tolist()}, the frame {tokens[:, 1:q + 1].tolist()}"
        assert torch.equal(tq[:, q + 1:], torch.full_like(tq[:, q + 1:], -7)), f"{c.name}: prefix {q} wrote past its {q} tokens"
        logits.append(_handoff(c).LOG.clone())
    assert torch.equal(logits[-1], full.LOG), f"{c.name}: the full launch and its own prefix disagree in the last step's logits"
    assert torch.equal(tokens[:, c.Q + 1:], torch.full_like(tokens[:, c.Q + 1:], -7)), f"{c.name}: tokens written past column {c.Q}"
    assert torch.equal(full.TOK.long(), tokens[:, c.Q]), f"{c.name}: the token hand-off holds {full.TOK.tolist()}"
    return tokens, full, torch.stack(logits)


def _refs(co, tokens):
    ref64, ref32 = R.reference(co, tokens), R.reference(co, tokens, dtype=torch.float32)
    return ref64, ref32, R.tolerance(ref32, ref64, co.case.H)


def _hold(c, what, got, ref64, ref32, tol):
    ok, where, r = R.accept(got, ref64, tol, c.H)
    r32 = R.worst(R.ratios(ref32, ref64, c.H))[1]
    print(f"RATIO {c.name} {what}: kernel {r:.3e} ({where}) / fp32 reference {r32:.3e} = {r / max(r32, 1e-30):.2f}; tol {tol:.3e}")
    assert ok, f"{c.name} {what}: {where} is off by {r:.3e} of the vector's scale; tol {tol:.3e} = 16 x the fp32 reference's {r32:.3e} (kernel / fp32 = {r / max(r32, 1e-30):.1f})"


def test_every_step_of_the_greedy_frame_against_fp64(built, clean_health):
    co, d = built
    c = co.case
    _check_shape(c)
    tokens, full, logits = _frame_and_prefixes(d)
    for k in range(c.Q):
        for b in range(c.B):
            assert int(tokens[b, k + 1]) == _lowest_argmax(logits[k, b]), f"{c.name}: step {k} row {b}: token {int(tokens[b, k + 1])} is not the first maximum"
    ref64, ref32, tol = _refs(co, tokens)
    _hold(c, "greedy", R.Ref(logits, full.QKV, full.ATT, full.H, full.X), ref64, ref32, tol)


@pytest.mark.parametrize("name", R.REPAIR_CASES)
def test_repair_launch_against_fp64(name, clean_health):
    co, d = _build(name)
    c = co.case
    _check_shape(c)
    want = R.launch(d, d.full)
    assert d.full.status.tolist() == [0, 0, 0, 0]
    code = 1 << 20
    got = R.launch(d, d.full, status_code=code)
    assert d.full.status.tolist() == [0, 1, code, 0], d.full.status.tolist()
    assert torch.equal(got, want), f"{c.name}: repaired frame {got.tolist()} vs undisturbed {want.tolist()}"
    solo = _handoff(c, solo=True)
    assert torch.equal(solo.TOK.long(), got[:, c.Q])
    for b in range(c.B):
        assert int(got[b, c.Q]) == _lowest_argmax(solo.LOG[b]), f"{c.name}: row {b}: the repaired last token is not the first maximum of the repair launch's logits"
    ref64, ref32, tol = _refs(co, got)
    last = R.Ref(solo.LOG[None], solo.QKV, solo.ATT, solo.H, solo.X)
    _hold(c, "repair", last, ref64._replace(logits=ref64.logits[-1:]), ref32._replace(logits=ref32.logits[-1:]), tol)


@pytest.mark.parametrize("noise_extra,tok_pad", [(0, 0), (3, 3)])
def test_sampler_plumbing_read_out(built, noise_extra, tok_pad, clean_health):
    """Temperature 1, noise 2^-40 at column k * top_k + r(b, k) of row b and 2^40 elsewhere: the token of step k is the r(b, k)-th id of
    that step's logits among the ids below limits[k].  The first blanked id carries +8 of head bias."""
    co, d = built
    c = co.case
    _check_shape(c)
    limits = R.design_limits(c)
    key = ("sampler", c.name)
    if key not in _BUILT:          # the case's weights with the designed bias: built once for both stride variants
        _BUILT[key] = R.device_tables(R.make_case(c, limits=limits), DEV)
    ds = _BUILT[key]
    noise = R.design_noise(c, limits, noise_extra).to(DEV)
    lim_dev = torch.tensor(limits, dtype=torch.int32, device=DEV)
    tokens, _, logits = _frame_and_prefixes(ds, noise=noise, limits=lim_dev, tok_pad=tok_pad)
    want, gap = R.expected_tokens(logits, c, limits)
    assert float(gap.max()) < 50, f"{c.name}: a rank read lies {float(gap.max()):.1f} below its row's maximum: 2^80 of noise no longer decides the race"
    assert torch.equal(tokens[:, 1:c.Q + 1], want), f"{c.name}: drew {tokens[:, 1:c.Q + 1].tolist()}, the logits' ranks say {want.tolist()} (limits {limits})"
