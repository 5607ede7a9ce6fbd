"""Every step of the persistent temporal-frame launch (csrc/lm_temporal.hip, rst_temporal_decode_frame behind ops.temporal_decode_frame)
and of its one-workgroup repair launch against an fp64 reference, one step at a time with the ring as an input, at the smallest
shapes that turn each loop of the kernel (tests/helpers/temporal_frame_ref.py: the case table, `steps`, `grid`).

The launch is driven through ops.TemporalFrameTables directly, so the test chooses the position, the context and the ring contents:
0.5 randn where the step looks, K = 0 / V = +-2^14 in every slot it must not see, its own stale row included.  Read back per step:
y, the output of every layer (launches over the first l layers), the row written to every layer's K and V, the status words, the
last layer's qkv / attention / gated-activation / x hand-offs with their epoch tags, and the whole rings (every other slot must be
bit-identical to what was uploaded).  The fp64 reference attends to the row the launch wrote (teacher forcing: no assertion hangs
on a bf16 rounding flip); the row itself is bounded against the reference's unrounded key and value.  Every weight matrix is followed
by a row of NaN and every ring by a head of NaN (temporal_frame_ref.device_case): a load past the operand shows even where it is
multiplied by zero.  That is how case `hd3848` found the one defect so far: a k block of 3585 .. 4095 columns was loaded as a whole
block of 4096, the last row's load running past the matrix (NaN in y before the fix in the descriptor decode).

Bound, per vector (the attention output per head): max |got - ref64| <= tol * max |ref64|, tol = 16 x the same ratio of the reference
run in fp32, within [2^-18, 1e-3], per case and step (temporal_frame_ref.tolerance).  Every comparison prints a `RATIO` line (run
with -s): the kernel's worst ratio, the fp32 reference's and their quotient.

Worst quotient kernel / fp32 reference per case, MI355X (256 CUs):
  d128-f32 1.44 | d64-bf16 0.95 | d64-f32 0.90 | d128-bf16 0.88 | tab-off 0.43 | e1088 0.77 | rows 0.49 | s6 0.51 |
  hd3848 0.64
  streaming over the wrap: d64-f32 0.67, d128-bf16 0.78 | repair launch: 0.94 (e1088 at pos 40)
(the kernel's worst ratio was 2.0e-7 .. 6.4e-7 of scale against tolerances of 5.0e-6 .. 2.6e-5: its single k chain per row and its
split softmax are, if anything, closer to fp64 than aten's fp32)"""
import pytest
import torch

from rstnet_amd import ops
from tests.helpers import temporal_frame_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture
def clean_health():
    yield
    ops.persistent_rearm(DEV)          # the repair counters of this test must not retire the path for later tests


_BUILT = {}


def _build(name):
    """Operands, device tables and rings of one case; one case is kept at a time (the wide ones hold ~100 MB)."""
    if name not in _BUILT:
        _BUILT.clear()
        co = R.make_case(R.BY_NAME[name])
        _BUILT[name] = (co, R.device_case(co, DEV))
    return _BUILT[name]


@pytest.fixture(scope="module", params=[c.name for c in R.CASES])
def built(request):
    """Module scope: pytest groups the tests of one case, so its operands are built once."""
    return _build(request.param)


def _check_shape(c):
    assert ops.temporal_frame_supported(1, c.E, c.H, c.Hd, c.L, c.cap, c.kv == "bf16", DEV), f"{c.name}: not served by the persistent launch"
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    here, meant = R.case_flags(c, cus), R.case_flags(c, 256)
    assert R.grid(c, cus).ok and here >= meant, \
        f"{c.name}: on {cus} CUs the grid is {R.grid(c, cus).G} (not {R.grid(c, 256).G}) and the case no longer takes {sorted(meant - here)}"


def _step(co, d, step, rings, what, *, status_code=0):
    """One step on `rings`: launch, read back, hold everything to the fp64 reference.  Returns the kernel / fp32 quotient."""
    c = co.case
    R.upload_rings(d, rings)
    x_before = d.x.clone()
    got, status, tags, table, after = R.launch(d, step, status_code=status_code)
    want_status = [0, 1, status_code, 0] if status_code else [0, 0, 0, 0]
    assert all(s == want_status for s in status), f"{c.name} {what}: status words {status}, expected {want_status} for every launch"
    assert torch.equal(d.x, x_before), f"{c.name} {what}: the input was written"
    for name, epoch in (("QKV", c.L), ("ATT", c.L), ("H", c.L), ("X", 2 * c.L)):
        assert bool((tags[name] == epoch).all()), f"{c.name} {what}: {name} granules carry tags {sorted(set(tags[name].tolist()))}, this launch's is {epoch}"
    slot = step.pos % c.cap
    keep = torch.arange(c.cap) != slot
    for l in range(c.L):
        for n, before, now in (("K", rings[l][0], after[l][0]), ("V", rings[l][1], after[l][1])):
            moved = ((before != now).any(-1) & keep).nonzero().tolist()
            assert not moved, f"{c.name} {what}: layer {l} {n}: slots other than {slot} were written: (head, slot) {moved[:8]}"
    own = R.rows_of(got)
    ref64 = R.reference(co, step, rings, table, own=own)
    ref32 = R.reference(co, step, rings, table, own=own, dtype=torch.float32)
    tol = R.tolerance(ref32, ref64, c)
    ok, where, r = R.accept(got, ref64, tol, c)
    r32 = R.worst(R.ratios(ref32, ref64, c, rows=False))[1]
    quot = r / max(r32, 1e-30)
    print(f"RATIO {c.name} {what}: kernel {r:.3e} ({where}) / fp32 reference {r32:.3e} = {quot:.2f}; tol {tol:.3e}")
    assert ok, f"{c.name} {what}: {where} is off by {r:.3e} of the vector's scale; tol {tol:.3e} = 16 x the fp32 reference's {r32:.3e} (kernel / fp32 = {quot:.1f})"
    return quot, after


def _name(step):
    return f"pos {step.pos} ctx {step.context}" + ("" if step.rope else " no rope")


def test_every_step_against_fp64(built, clean_health):
    co, d = built
    c = co.case
    _check_shape(c)
    quots = [_step(co, d, st, R.make_rings(co, st), _name(st))[0] for st in R.steps(c)]
    print(f"RATIO {c.name} worst quotient over {len(quots)} steps: {max(quots):.2f}")


@pytest.mark.parametrize("name", R.STREAM_CASES)
def test_streaming_over_the_wrap_against_fp64(name, clean_health):
    """Six consecutive steps from pos = cap - 3 on the rings the launch itself leaves: each step's reference gets the rings read
    back before it (the step's own slot poisoned again: the launch must replace it, the ring map hides the slot behind it)."""
    co, d = _build(name)
    c = co.case
    _check_shape(c)
    first = R.Step(c.cap - 3, None, True)
    rings, quots = R.make_rings(co, first), []
    for i in range(R.STREAM_STEPS):
        st = R.Step(first.pos + i, None, True)
        q, after = _step(co, d, st, rings, f"stream {_name(st)}")
        quots.append(q)
        rings = R.poison(co, [(K.clone(), V.clone()) for K, V in after], R.Step(st.pos + 1, None, True))
    print(f"RATIO {c.name} worst quotient over {len(quots)} streamed steps: {max(quots):.2f}")


@pytest.mark.parametrize("name,step", R.repair_steps(), ids=[f"{n}-{s.pos}" for n, s in R.repair_steps()])
def test_repair_launch_against_fp64(name, step, clean_health):
    """A planted time-out code (nothing times out): the one-workgroup launch behind every persistent one recomputes the step from the
    untouched input and the rings, counts the repair and clears the code; y, the rows and the repair launch's own granule set are
    held to fp64 like the persistent launch's."""
    co, d = _build(name)
    _check_shape(co.case)
    _step(co, d, step, R.make_rings(co, step), f"repair {_name(step)}", status_code=1 << 20)
