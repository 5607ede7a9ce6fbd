"""The launch-per-op ring attention held to fp64 at designed scores: every case of tests/helpers/ring_attention_ref.py runs every one of
its profiles at every one of its positions through the public entry point (ops.lm_attn_decode, ops.gemv_attn, ops.lm_attn_prefill +
ops.lm_ring_append[_ragged], ops.attention(ring=True)), one launch on freshly uploaded rings each.  The fp64 reference attends to the
bytes the launch wrote for its new positions (teacher forcing); those rows are bounded against the reference's unrounded key / value,
every other ring byte must be bit-identical to what was uploaded, and every (stream, query, head) vector of the output is held
element by element to tol sum_j p_j |v_j| (the helper's docstring: tol = max(16 r32, t_op) within [2^-18, 1e-3]).  Every comparison
prints a RATIO line: the kernel's worst ratio, the fp32 reference's, the tolerance and the quotient ratio / tol.

Worst quotient (kernel ratio / tol) per case over its profiles and positions, MI355X (256 CUs; the dense cases ran 25 streams):
  small-c3-d64 0.124;  small-c8-d128 0.098;  small-c8-d32 0.053;  small-c64-d64-ctx 0.180;  small-c64-d64-rope-packed 0.949;
  small-c64-d128-gqa 0.099;  small-c4-ps 0.253;  split-c130-d64-f32 0.095;  split-c130-d64-f32-rope 0.236;
  split-c130-d128-bf16 0.094;  split-c130-d128-bf16-table 0.073;  split-c300-d128-f32 0.094;  split-c300-d128-f32-ropedims 0.200;
  split-c300-d64-bf16-gqa2 0.801;  split-c300-d64-f32-gqa4 0.093;  many-c2048-d64-f32 0.070;  many-c2048-d128-bf16 0.075;
  dense-d64-f32 0.089;  dense-d128-f32 0.504;  dense-d64-bf16 0.076;  dense-d128-bf16 0.061;  ps-c130-d64-f32 0.121;
  ps-c300-d128-bf16-gqa 0.058;  ps-c130-d64-f32-table 0.151;  gemv-c8 0.068;  gemv-c8-b2-ctx3 0.052;  gemv-c2 0.000;
  gemv-c3 0.062;  gemv-c8-randn 0.004;  pf-t1-w31-d64-f32 0.400;  pf-t1-w31-d64-bf16 0.040;  pf-t31-w32-d128-f32 0.318;
  pf-t31-w32-d128-bf16 0.066;  pf-t32-w33-d64-f32 0.189;  pf-t32-w33-d64-bf16 0.078;  pf-t33-w299-d128-f32 0.218;
  pf-t33-w299-d128-bf16 0.100;  pf-t33-w299-d64-f32 0.216;  pf-t33-w299-d64-bf16 0.060;  pf-t70-w69-d64-f32 0.172;
  pf-t70-w69-d64-bf16 0.064;  pf-t33-w140-d128-gqa-f32 0.209;  pf-t33-w140-d128-gqa-bf16 0.049;  pf-t33-w140-d64-gqa4-f32 0.178;
  pf-t33-w140-d64-gqa4-bf16 0.020;  pf-ragged-d64-f32 0.225;  pf-ragged-d64-bf16 0.016;  pf-ragged-d128-f32 0.230;
  pf-ragged-d128-bf16 0.055;  qpre-d64 0.029;  qpre-d128-gqa 0.032;
  (added with tests/test_utterance_attention_bounds_gpu.py: ops.attention(ring=True) past the few-query path, attention_kernel<D> of
  csrc/attention.hip)  walk-c250-d64-t12 0.251;  walk-c70-d128-t40 0.238;  walk-c10-d32-t3 0.149;  walk-c33-d64-t33 0.087.
No launch saw a poisoned slot, none produced a non-finite value, and no kernel was changed.  The two cases near 1 leave through the
packed bf16 hi + lo output, whose own 2^-16 IS their tolerance (t_op); the rotating cases sit at 0.15 - 0.5 of the 2^-18 floor because
the launch's expf frequency differs from the reference's by an ulp (the helper's docstring: why they stay at positions <= 22).  The
bf16 multi-position kernel uses a tenth of its t_op: the hi + lo planes of Q and P are far from their worst case on these operands.

Prefill against single steps (test_prefill_against_single_steps; the stepped route's own worst quotient: 0.24 on fp32 rings, 0.004 on
bf16 rings): worst mutual distance |prefill - steps| / sum_j p_j |v_j| per profile, fp32 rings | bf16 rings (|score| <= 31):
  flat 2.9e-07 | 9.7e-06;  flat/k0 3.4e-07 | 1.5e-05;  peak@oldest 1.8e-07 | 4.6e-06;  peak@own 2.6e-07 | 1.2e-05;
  peak@split_first 3.1e-07 | 7.0e-06;  peak@split_last 3.6e-07 | 9.4e-06;  low 2.8e-05 | 1.1e-05;  high 2.8e-05 | 1.3e-05;
  ramp_up 1.2e-05 | 1.6e-05;  ramp_down 1.5e-05 | 1.5e-05;  ramp_wide 3.0e-05 | 1.6e-05.
On fp32 rings the two routes drift apart with |score| (3e-7 flat, 3e-5 at |score| ~ 90: two fp32 summation orders of a dot product of
that size); on bf16 rings the planes of the multi-position kernel set a level of 1e-5 that does not grow up to |score| = 31."""
import pytest
import torch

from tests.helpers import ring_attention_ref as R
from tests.helpers.gemv_bounds import c_gemv

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _run(c, profile, position, route="entry"):
    b = R.build(c, profile, position)
    got, own = R.device_run(b, DEV, route)
    m = R.measure(b, own=own)
    ok, what, r = R.accept(got, m.ref64, m.tol, b)
    print(f"RATIO {c.name} {profile} pos {position} {route}: kernel {r:.3e} ({what}) fp32 {m.r32:.3e} tol {m.tol:.3e} quotient {r / m.tol:.3f}")
    return b, got, m, ok, r / m.tol


@pytest.mark.parametrize("name", [c.name for c in R.CASES if c.weight == "eye"])
def test_launch_within_bound(name):
    c = R.resolve(R.BY_NAME[name], _cus())
    if R.BY_NAME[name].B == 0:
        assert R.instance(c, _cus()).dense
    missed, worst = [], 0.0
    for position in c.positions:
        for profile in c.profiles:
            b, got, m, ok, q = _run(c, profile, position)
            worst = max(worst, q) if q == q else float("inf")
            if not ok:
                missed.append((profile, position, q))
    print(f"WORST {name}: quotient {worst:.3f}")
    assert not missed, missed


@pytest.mark.parametrize("name", [c.name for c in R.CASES if c.weight != "eye"])
def test_gemv_attn_with_a_randn_out_projection(name):
    """The attention vector through a randn bf16 out-projection: the per-element attention bound carried through |w|, plus the GEMV's
    own term c_gemv(K) 2^-24 sum_k |w_k x_k| (tests/helpers/gemv_bounds.py)."""
    c = R.resolve(R.BY_NAME[name], _cus())
    E = c.H * c.D
    w = (torch.randn(E, E, generator=torch.Generator().manual_seed(E)) / E ** 0.5).bfloat16()
    missed = []
    for position in c.positions:
        for profile in c.profiles:
            b = R.build(c, profile, position)
            b.w = w
            got, own = R.device_run(b, DEV)
            m = R.measure(b, own=own)
            att, den, w64 = m.ref64.out.reshape(c.B, E), m.ref64.den.reshape(c.B, E), w.double()
            y64 = att @ w64.T
            bound = c_gemv(E) * 2.0 ** -24 * (att.abs() @ w64.abs().T) + (m.tol * den) @ w64.abs().T
            y = got.out.reshape(c.B, E).double()
            q = float(((y - y64).abs() / bound).max()) if bool(torch.isfinite(y).all()) else float("nan")
            rr = R.ring_ratio(got.K_after, got.V_after, m.ref64, (b.K, b.V), c, b.pos)
            print(f"RATIO {name} {profile} pos {position}: quotient {q:.3f} ring {rr:.3e} tol {m.tol:.3e}")
            if not (q <= 1.0 and rr <= m.tol):
                missed.append((profile, position, q, rr))
    assert not missed, missed


def _for_steps(c, position):
    """The case a chunk is fed as single ops.lm_attn_decode steps in: itself where the steps' in-launch rotation stays at small positions
    (the helper's docstring), else the same case without rotation."""
    return c if c.rope == "off" or max(R.stream_pos(c, position)) + c.T - 1 <= R.ROPE_POS_LIMIT else R.replace(c, rope="off")


STEP_CASES = [c.name for c in R.CASES if c.entry == "prefill" and c.lengths is None]


@pytest.mark.parametrize("name", STEP_CASES)
def test_prefill_against_single_steps(name):
    """The same chunk as Tc single steps on the same uploaded rings: both routes within their own bound of the same fp64 reference (each
    attending to the rows its route wrote); their mutual distance, in the bound's unit sum_j p_j |v_j|, is printed per profile."""
    c = R.resolve(R.BY_NAME[name], _cus())
    missed = []
    for position in c.positions:
        cs = _for_steps(c, position)
        for profile in c.profiles:
            b, got, m, ok, q = _run(cs, profile, position)
            b2, got2, m2, ok2, q2 = _run(cs, profile, position, "steps")
            d = R.out_ratio(got2.out, R.SimpleNamespace(out=got.out.double(), den=m.ref64.den, scores=m.ref64.scores), c)
            print(f"MUTUAL {name} rope {cs.rope} {profile} pos {position}: prefill / steps distance {d:.3e} (tol {m.tol:.3e} / {m2.tol:.3e})")
            if not (ok and ok2):
                missed.append((profile, position, q, q2))
    assert not missed, missed
