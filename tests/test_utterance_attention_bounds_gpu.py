"""attention_kernel<D, QKV> (csrc/attention.hip) held to fp64 at designed scores: every case of tests/helpers/utterance_attention_ref.py
runs every one of its profiles through its public entry (ops.attention, ops.attention_qkv), one launch on freshly uploaded operands
each, the fused form's operands built from the bytes of the table ops.rope_table returned for that launch.  Every (stream, query, head)
vector is held element by element to tol sum_j p_j |v_j| (the helper's docstring: tol = 16 r32 within [2^-18, 1e-3], t_op = 0).  A case
that does not rotate also sends the same bytes through the other form; the two results must agree within twice the bound.  The ring
walk of the same kernel (the `walk-` cases of tests/helpers/ring_attention_ref.py) runs every profile at every position through
ops.attention(ring=True); every ring byte must be bit-identical afterwards.  Every comparison prints a RATIO line: the kernel's worst
ratio, the fp32 reference's, the tolerance and the quotient ratio / tol.

Worst quotient (kernel ratio / tol) per case over its profiles (and positions), MI355X, 512 comparisons of the whole-utterance forms
and 132 of the ring walk:
  plain-t1-d64 0.000;  fused-t1-d32 0.000;  fused-norope-t1-d128 0.000;  plain-t31-d128 0.070;  fused-t31-d64 0.075;
  plain-t32-d32 0.085;  fused-t32-d128 0.071;  plain-t33-d64 0.075;  fused-t33-d32 0.074;  fused-norope-t33-d64 0.074;
  plain-t161-d64 0.080;  fused-t161-d128 0.070;  plain-t225-d128 0.067;  fused-t225-d32 0.072;  plain-t256-d64 0.069;
  fused-t256-d128 0.082;  plain-t257-d32 0.079;  fused-t257-d64 0.071;  plain-t257-d128 0.065;  plain-t321-d64 0.087;
  fused-t321-d128 0.070;  fused-norope-t321-d32 0.116;  plain-t545-d128 0.072;  fused-t545-d64 0.074;  plain-t700-c250-d64 0.076;
  fused-t700-c250-d64 0.073;  fused-t700-c250-d128 0.066;  plain-t700-c40-d128 0.070;  fused-t700-c40-d32 0.083;
  fused-norope-t700-c40-d64 0.079;  plain-t700-c34-d64 0.070;  fused-t700-c34-d128 0.073;  plain-t700-c33-d32 0.071;
  fused-t700-c33-d64 0.079;  plain-t700-c32-d128 0.069;  fused-t700-c32-d32 0.082;  plain-t700-c1-d64 0.000;  fused-t700-c1-d32 0.000;
  plain-t33-c250-d128 0.070;  fused-t33-c250-d64 0.071;  fused-norope-t33-c250-d32 0.083;
  walk-c250-d64-t12 0.251;  walk-c70-d128-t40 0.238;  walk-c10-d32-t3 0.149;  walk-c33-d64-t33 0.087.
No kernel was changed, no launch produced a non-finite value or saw a poisoned slot, and every ring byte came back as uploaded.  The
whole-utterance forms sit at 1/16 of their tolerance, i.e. at the fp32 reference's own ratio (largest ratio 4.8e-5 against r32 4.9e-5,
plain-t700-c40-d128 at ramp_wide): the kernel is as accurate as an fp32 softmax attention in torch.  A single visible key (T = 1,
context 1) is exact.  Wherever nothing rotates, the plain and the fused form returned the same bytes (distance 0 in all 184 pairs)."""
import pytest
import torch

from tests.helpers import ring_attention_ref as R
from tests.helpers import utterance_attention_ref as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("name", [c.name for c in U.CASES])
def test_launch_within_bound(name):
    c = U.BY_NAME[name]
    other = None if c.rope else "fused" if c.entry == "plain" else "plain"
    table = U.device_table(c, DEV)
    missed, worst = [], 0.0
    for profile in c.profiles:
        b = U.build(c, profile, table=table)
        m = U.measure(b)
        got = U.device_run(b, DEV)
        ok, r = U.accept(got, m.ref64, m.tol)
        print(f"RATIO {name} {profile}: kernel {r:.3e} fp32 {m.r32:.3e} tol {m.tol:.3e} quotient {r / m.tol:.3f}")
        worst = max(worst, r / m.tol) if r == r else float("inf")
        if not ok:
            missed.append((profile, c.entry, r / m.tol))
        if other:
            got2 = U.device_run(b, DEV, form=other)
            ok2, r2 = U.accept(got2, m.ref64, m.tol)
            d = U.out_ratio(got2, U.SimpleNamespace(out=got.double(), den=m.ref64.den))
            print(f"RATIO {name} {profile} as {other}: kernel {r2:.3e} tol {m.tol:.3e} quotient {r2 / m.tol:.3f}; "
                  f"{c.entry} / {other} distance {d:.3e} ({d / m.tol:.3f} tol)")
            if not (ok2 and d <= 2 * m.tol):
                missed.append((profile, other, r2 / m.tol, d / m.tol))
    print(f"WORST {name}: quotient {worst:.3f}")
    assert not missed, missed


@pytest.mark.parametrize("name", R.WALK_CASES)
def test_ring_walk_within_bound(name):
    c = R.BY_NAME[name]
    assert R.instance(c, 256).kernel == f"attention<{c.D}>:ring"
    missed, worst = [], 0.0
    for position in c.positions:
        for profile in c.profiles:
            b = R.build(c, profile, position)
            got, own = R.device_run(b, DEV)
            m = R.measure(b, own=own)
            ok, what, r = R.accept(got, m.ref64, m.tol, b)
            print(f"RATIO {name} {profile} pos {position}: kernel {r:.3e} ({what}) fp32 {m.r32:.3e} tol {m.tol:.3e} quotient {r / m.tol:.3f}")
            worst = max(worst, r / m.tol) if r == r else float("inf")
            same = torch.equal(got.K_after, b.K) and torch.equal(got.V_after, b.V)
            if not (ok and same):
                missed.append((profile, position, what, r / m.tol, same))
    print(f"WORST {name}: quotient {worst:.3f}")
    assert not missed, missed
