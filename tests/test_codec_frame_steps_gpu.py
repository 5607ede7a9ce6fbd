"""Every step of the persistent codec-transformer launch (csrc/codec_tr.hip, rst_codec_transformer_frame behind
ops.codec_transformer_frame) and of its one-workgroup repair launch against an fp64 reference, one step at a time with the rings as an
input, at the smallest shapes that turn each loop of the kernel (tests/helpers/codec_frame_ref.py: the case table, `steps`, `grid`).

The test chooses the position, the number of new positions, the context, rope or none and the ring contents: 0.5 randn where a query
of the step looks, K = 0 / V = +-2^14 in every slot none may see, the new positions' own stale rows included.  Read back per step: y,
the output of every layer (launches over the first l layers), the rows written to every layer's K and V, the status words, the last
layer's qkv / attention / GELU / x hand-offs with their epoch tags, and the whole rings (every slot but the T new ones must be
bit-identical to what was uploaded).  The fp64 reference attends to the rows the launch wrote (teacher forcing); the rows themselves
are bounded against the reference's own keys and values.  Every weight matrix and gamma / beta / scale vector is followed by a row of
NaN and every ring by a head of NaN (codec_frame_ref.device_case): a load past the operand shows even where it is multiplied by zero.

Bound, per vector (per row = (stream, position); the attention output also per head): max |got - ref64| <= tol * max |ref64|,
tol = 16 x the same ratio of the reference run in fp32, within [2^-18, 1e-3], per case and step (codec_frame_ref.tolerance).  Every
comparison prints a `RATIO` line (run with -s): the kernel's worst ratio, the fp32 reference's and their quotient.

Worst quotient kernel / fp32 reference per case, MI355X (256 CUs):
  d16 1.04 | d32 1.14 | d64 1.38 | d128 2.24 | d256 1.91 | e528 0.64 | e1088 1.23 | f2056 1.10 | rows4 0.69 | short 0.58 |
  short4 0.73 | noscale 1.30
  streaming over the wrap: d64 1.38, short 0.84 | repair launch: d16 1.01, d64 1.01, e1088 0.46, rows4 0.55
(the kernel's worst ratio was 1.5e-7 .. 2.3e-5 of scale against tolerances of 3.9e-6 .. 2.9e-4; the large ones are the rotated keys at
positions past 1000, where the fp32 angle (pos + t) * freq is the error of the kernel and of the fp32 reference alike: 1.201e-5 both
at d16, pos 1108.  No defect of the kernel was found.)"""
import pytest
import torch

from rstnet_amd import _lib, ops
from tests.helpers import codec_frame_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture
def clean_health():
    yield
    ops.persistent_rearm(DEV)          # the repair counters of this test must not retire the path for later tests


_BUILT = {}


def _build(name):
    """Operands, device tensors and rings of one case; one case is kept at a time."""
    if name not in _BUILT:
        _BUILT.clear()
        co = R.make_case(R.BY_NAME[name])
        _BUILT[name] = (co, R.device_case(co, DEV))
    return _BUILT[name]


@pytest.fixture(scope="module", params=[c.name for c in R.CASES])
def built(request):
    """Module scope: pytest groups the tests of one case, so its operands are built once."""
    return _build(request.param)


def _library_grid(c, T):
    with torch.cuda.device(DEV):
        return int(_lib.lib().rst_codec_transformer_supported(c.B, T, c.E, c.H, c.F, c.L, c.cap))


def _check_shape(c, Ts=None):
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    for T in Ts or R.TS[c.name]:
        g = R.grid(c, T, cus)
        assert ops.codec_transformer_frame_supported(c.B, T, c.E, c.H, c.F, c.L, c.cap, device=DEV), f"{c.name} T {T}: not served by the persistent launch"
        assert g.ok and _library_grid(c, T) == g.G, f"{c.name} T {T}: the library's grid is {_library_grid(c, T)}, the restated one {g.G if g.ok else 0}"
    here, meant = R.case_flags(c, cus), R.case_flags(c, 256)
    assert here >= meant, f"{c.name}: on {cus} CUs the grid is {R.grid(c, 1, cus).G} (not {R.grid(c, 1, 256).G}) and the case no longer takes {sorted(meant - here)}"


def _bits(t):
    return t.contiguous().view(torch.int32)


def _step(co, d, step, rings, what, *, status_code=0):
    """One step on `rings`: launch, read back, hold everything to the fp64 reference.  Returns the kernel / fp32 quotient."""
    c = co.case
    R.upload_rings(d, rings)
    got, status, tags, x_after, after = R.launch(d, step, status_code=status_code)
    want_status = [0, 1, status_code, 0] if status_code else [0, 0, 0, 0]
    assert all(s == want_status for s in status), f"{c.name} {what}: status words {status}, expected {want_status} for every launch"
    assert torch.equal(_bits(x_after), _bits(co.x[:, :step.T])), f"{c.name} {what}: the input was written"
    for name, epoch in R.epochs(c.L).items():
        assert bool((tags[name] == epoch).all()), f"{c.name} {what}: {name} granules carry tags {sorted(set(tags[name].view(-1).tolist()))}, this launch's is {epoch}"
    keep = torch.ones(c.cap, dtype=torch.bool)
    keep[R.new_slots(step, c.cap)] = False
    for l in range(c.L):
        for n, before, now in (("K", rings[l][0], after[l][0]), ("V", rings[l][1], after[l][1])):
            moved = ((_bits(before) != _bits(now)).any(-1) & keep).nonzero().tolist()
            assert not moved, f"{c.name} {what}: layer {l} {n}: slots other than {R.new_slots(step, c.cap)} were written: (stream, head, slot) {moved[:8]}"
    own = R.rows_of(got)
    ref64 = R.reference(co, step, rings, own=own)
    ref32 = R.reference(co, step, rings, own=own, dtype=torch.float32)
    tol = R.tolerance(ref32, ref64, c)
    ok, where, r = R.accept(got, ref64, tol, c)
    r32 = R.reference_error(ref32, ref64, c)[1]
    quot = r / max(r32, 1e-30)
    print(f"RATIO {c.name} {what}: kernel {r:.3e} ({where}) / fp32 reference {r32:.3e} = {quot:.2f}; tol {tol:.3e}")
    assert ok, f"{c.name} {what}: {where} is off by {r:.3e} of the vector's scale; tol {tol:.3e} = 16 x the fp32 reference's {r32:.3e} (kernel / fp32 = {quot:.1f})"
    return quot, after


def _name(step):
    return f"pos {step.pos} T {step.T} ctx {step.context}" + ("" if step.rope else " no rope")


def test_every_step_against_fp64(built, clean_health):
    co, d = built
    c = co.case
    _check_shape(c)
    quots = [_step(co, d, st, R.make_rings(co, st), _name(st))[0] for st in R.steps(c)]
    print(f"RATIO {c.name} worst quotient over {len(quots)} steps: {max(quots):.2f}")


@pytest.mark.parametrize("name", R.STREAM_CASES)
def test_streaming_over_the_wrap_against_fp64(name, clean_health):
    """Six consecutive steps of 1, 2 and 4 positions from pos = cap - 3 on the rings the launch itself leaves: each step's reference
    gets the rings read back before it (the slots no query of the step may see poisoned again, the new positions' own included: the
    launch must replace those, the ring map hides the others)."""
    co, d = _build(name)
    c = co.case
    cuts = R.stream_cuts(c)
    _check_shape(c, sorted(set(cuts)))
    pos = c.cap - 3
    rings, quots = R.make_rings(co, R.Step(pos, c.cap, True, cuts[0])), []
    for i, T in enumerate(cuts):
        st = R.Step(pos, c.cap, True, T)
        q, after = _step(co, d, st, rings, f"stream {_name(st)}")
        quots.append(q)
        pos += T
        if i + 1 < len(cuts):
            rings = R.poison(co, [(K.clone(), V.clone()) for K, V in after], R.Step(pos, c.cap, True, cuts[i + 1]))
    assert pos > c.cap + 3
    print(f"RATIO {c.name} worst quotient over {len(quots)} streamed steps: {max(quots):.2f}")


@pytest.mark.parametrize("name,step", R.repair_steps(), ids=[f"{n}-{s.pos}" for n, s in R.repair_steps()])
def test_repair_launch_against_fp64(name, step, clean_health):
    """A planted time-out code (nothing times out): the one-workgroup launch behind every persistent one recomputes the step from the
    untouched input and the rings -- every (stream, head) pair in turn --, counts the repair and clears the code; y, the rows and the
    repair launch's own granule set are held to fp64 like the persistent launch's."""
    co, d = _build(name)
    _check_shape(co.case, [step.T])
    _step(co, d, step, R.make_rings(co, step), f"repair {_name(step)}", status_code=1 << 20)


# (what is refused, case): E H F L cap B scale, T
REFUSED = [
    ("head dim 48", R.Case("D48", 192, 4, 512, 2, 20, 1, None), 1),
    ("head dim 8", R.Case("D8", 64, 8, 512, 2, 20, 1, None), 1),
    ("five positions", R.Case("T5", 64, 4, 64, 2, 20, 1, None), 5),
    ("five rows", R.Case("R5", 64, 4, 512, 2, 20, 5, None), 1),
    ("a ring shorter than the step", R.Case("cap3", 64, 4, 64, 2, 3, 1, None), 4),
    ("E not a multiple of 8", R.Case("E100", 100, 5, 512, 2, 20, 1, None), 1),
    ("F not a multiple of 8", R.Case("F68", 64, 4, 68, 2, 20, 1, None), 1),
    ("more (stream, head) pairs than workgroups", R.Case("BH", 64, 4, 8, 2, 20, 1, None), 1),
]


def _over_lds():
    """The longest ring whose score rows fit the LDS limit at four rows, and one slot more."""
    c = R.Case("lds", 64, 4, 64, 2, 3000, 1, None)
    while R.lds_bytes(c._replace(cap=c.cap + 1), 4) <= R.LDS_LIMIT:
        c = c._replace(cap=c.cap + 1)
    return c, c._replace(cap=c.cap + 1)


def test_unserved_shapes_are_refused():
    """The launcher's gates (rst_codec_tr_grid), each on a shape of its own: ops.codec_transformer_frame_supported says no, the library's
    own answer is 0 workgroups, and the entry itself returns an error before it enqueues anything: the rings and the status words
    are as they were."""
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    fits, over = _over_lds()
    assert R.lds_bytes(fits, 4) <= R.LDS_LIMIT < R.lds_bytes(over, 4)
    assert R.grid(fits, 4, cus).ok and _library_grid(fits, 4) == R.grid(fits, 4, cus).G
    status = ops.codec_transformer_status(torch.device(DEV))
    for what, c, T in REFUSED + [("an LDS footprint over the limit", over, 4)]:
        assert not R.grid(c, T, cus).ok, what
        assert not ops.codec_transformer_frame_supported(c.B, T, c.E, c.H, c.F, c.L, c.cap, device=DEV), what
        assert _library_grid(c, T) == 0, what
        D = c.E // c.H
        layers = []
        for _ in range(c.L):
            ly = {"in_proj": torch.zeros(3 * c.E, c.E, device=DEV), "out_proj": torch.zeros(c.E, c.E, device=DEV),
                  "linear1": torch.zeros(c.F, c.E, device=DEV), "linear2": torch.zeros(c.E, c.F, device=DEV)}
            ly.update({n: torch.ones(c.E, device=DEV) for n in ("norm1_w", "norm1_b", "norm2_w", "norm2_b")})
            ly.update(scale1=None, scale2=None, k_cache=torch.full((c.B, c.H, c.cap, D), 3.0, device=DEV),
                      v_cache=torch.full((c.B, c.H, c.cap, D), 5.0, device=DEV))
            layers.append(ly)
        before = status.tolist()
        with pytest.raises((ValueError, _lib.RstError)):
            ops.codec_transformer_frame(torch.ones(c.B, T, c.E, device=DEV), layers, torch.zeros(1, dtype=torch.int64, device=DEV), H=c.H,
                                        context=c.cap, rope=True, max_period=R.MAX_PERIOD, eps=R.EPS)
        torch.cuda.synchronize()
        assert status.tolist() == before, what
        for ly in layers:
            assert bool((ly["k_cache"] == 3.0).all()) and bool((ly["v_cache"] == 5.0).all()), f"{what}: the refused call wrote the rings"
