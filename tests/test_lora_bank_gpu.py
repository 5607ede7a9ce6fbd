"""ops.lora_bank_shrink / ops.lora_bank_expand (csrc/lm_lora_bank.hip) against fp64, element by element under the bounds of
tests/helpers/lora_bank.py, and the row independence the kernels promise: a row's bits do not depend on the batch it sits in."""
import functools

import pytest
import torch

from rstnet_amd import ops
from tests.helpers import gemv_bounds as GB
from tests.helpers import lora_bank as LB

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_AD = 3
# rows -> (rows_per_id, ids): 0, 1, 2 and -1 mixed (a single row takes adapter 1)
ROWS = {1: (1, [1]), 5: (1, [0, 2, -1, 1, 0]), 67: (1, [(i * 7) % 4 - 1 for i in range(67)]), 12: (3, [2, -1, 0, 1])}


@functools.lru_cache(maxsize=2)
def _banks(K, r, N):
    A, Bm = LB.bank_operands(N_AD, r, K, N, seed=K + r)
    return A, Bm, A.to(DEV), Bm.to(DEV)


def _x(rows, K, prologue):
    g = torch.Generator().manual_seed(rows * 31 + K + prologue)
    x = GB.mixed_rows(rows, 2 * K if prologue == 2 else K, g)
    alpha = 1 + 0.1 * torch.randn(K, generator=g) if prologue == 1 else None
    return x, alpha


SHRINK = [(K, r, p) for K in (64, 520, 1024, 11264) for r in (16, 96) for p in (0, 1, 2) if p != 2 or K in (1024, 11264)]


@pytest.mark.parametrize("K,r,prologue", SHRINK)
def test_shrink_against_fp64(K, r, prologue):
    A, _, A_d, _ = _banks(K, r, 8)
    for rows, (rpi, ids) in ROWS.items():
        x, alpha = _x(rows, K, prologue)
        ids_t = torch.tensor(ids, dtype=torch.int32)
        for ps in (1.0, 0.1875):
            kw = dict(rows_per_id=rpi, prologue=prologue, post_scale=ps)
            a = ops.lora_bank_shrink(x.to(DEV), A_d, ids_t.to(DEV), alpha=None if alpha is None else alpha.to(DEV), eps=GB.EPS_RMS, **kw).cpu()
            a64, bound = LB.shrink_ref(x, A, ids_t, alpha=alpha, **kw)
            worst = LB.worst(a, a64, bound)
            print(f"shrink K={K} r={r} prologue={prologue} rows={rows} post_scale={ps}: worst err / bound = {worst:.3f}")
            assert a.shape == (rows, r) and worst <= 1.0
            base = LB.row_ids(ids_t, rows, rpi) < 0
            assert not a[base].any() and (rows == 1 or a[~base].any())


@pytest.mark.parametrize("N,r,rows", [(50, 16, 1), (50, 96, 5), (50, 16, 67), (50, 96, 12), (3072, 16, 5), (3072, 96, 67), (3072, 96, 12),
                                      (151936, 32, 5)])
def test_expand_against_fp64(N, r, rows):
    _, Bm, _, B_d = _banks(64, r, N)
    rpi, ids = ROWS[rows]
    ids_t = torch.tensor(ids, dtype=torch.int32)
    g = torch.Generator().manual_seed(N + r + rows)
    a = GB.mixed_rows(rows, r, g)
    y = GB.mixed_rows(rows, N, g, -4, 4)                          # the residual the base product left
    y_d = y.to(DEV)
    out = ops.lora_bank_expand(a.to(DEV), B_d, ids_t.to(DEV), y_d, rows_per_id=rpi)
    assert out is y_d                                             # in place
    got = y_d.cpu()
    y64, bound = LB.expand_ref(a, Bm, ids_t, y, rows_per_id=rpi)
    worst = LB.worst(got, y64, bound)
    print(f"expand N={N} r={r} rows={rows}: worst err / bound = {worst:.3f}")
    assert worst <= 1.0
    base = LB.row_ids(ids_t, rows, rpi) < 0
    assert torch.equal(got[base], y[base]) and (rows == 1 or not torch.equal(got[~base], y[~base]))


def test_ids_outside_the_bank_are_base_rows():
    """One unsigned compare: every negative id and every id >= n_adapters reads nothing and changes nothing."""
    A, Bm, A_d, B_d = _banks(64, 16, 50)
    ids = torch.tensor([-1, -7, N_AD, 2 ** 31 - 1, -2 ** 31, 1], dtype=torch.int32)
    x, _ = _x(6, 64, 0)
    a = ops.lora_bank_shrink(x.to(DEV), A_d, ids.to(DEV)).cpu()
    assert not a[:5].any() and a[5].any()
    y = torch.randn(6, 50)
    got = ops.lora_bank_expand(torch.randn(6, 16).to(DEV), B_d, ids.to(DEV), y.to(DEV)).cpu()
    assert torch.equal(got[:5], y[:5]) and not torch.equal(got[5], y[5])


@pytest.mark.parametrize("prologue", [0, 1, 2])
def test_rows_do_not_depend_on_their_batch(prologue):
    """A mixed batch computed whole, permuted, and row by row (rows = 1): bit-identical rows, for both launches."""
    K, r, N, rows = 1024, 96, 3072, 9
    A, Bm, A_d, B_d = _banks(K, r, N)
    x, alpha = _x(rows, K, prologue)
    ids = torch.tensor([0, 2, -1, 1, 0, 1, 2, -1, 0], dtype=torch.int32)
    g = torch.Generator().manual_seed(5)
    y = GB.mixed_rows(rows, N, g, -4, 4)
    al = None if alpha is None else alpha.to(DEV)

    def both(xx, ii, yy):
        a = ops.lora_bank_shrink(xx.to(DEV), A_d, ii.to(DEV), prologue=prologue, alpha=al, eps=GB.EPS_RMS, post_scale=0.1875)
        return a.cpu(), ops.lora_bank_expand(a, B_d, ii.to(DEV), yy.to(DEV)).cpu()

    a_all, y_all = both(x, ids, y)
    perm = torch.randperm(rows, generator=g)
    a_p, y_p = both(x[perm], ids[perm], y[perm])
    assert torch.equal(a_p, a_all[perm]) and torch.equal(y_p, y_all[perm])
    for b in range(rows):
        a_1, y_1 = both(x[b:b + 1], ids[b:b + 1], y[b:b + 1])
        assert torch.equal(a_1[0], a_all[b]) and torch.equal(y_1[0], y_all[b]), b
    # the same rows as T = 3 positions of 3 streams that share an id: rows_per_id changes which id a row reads, nothing else
    ids3 = torch.tensor([0, 2, 1], dtype=torch.int32)
    a3 = ops.lora_bank_shrink(x.to(DEV), A_d, ids3.to(DEV), rows_per_id=3, prologue=prologue, alpha=al, eps=GB.EPS_RMS, post_scale=0.1875).cpu()
    a9 = ops.lora_bank_shrink(x.to(DEV), A_d, ids3.repeat_interleave(3).to(DEV), prologue=prologue, alpha=al, eps=GB.EPS_RMS, post_scale=0.1875).cpu()
    assert torch.equal(a3, a9)


def test_bad_arguments_are_refused_on_the_host():
    A, Bm, A_d, B_d = _banks(64, 16, 50)
    x = torch.zeros(4, 64, device=DEV)
    ids = torch.zeros(4, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="rows_per_id"):
        ops.lora_bank_shrink(x, A_d, ids, rows_per_id=3)
    with pytest.raises(ValueError, match="rows_per_id"):
        ops.lora_bank_expand(torch.zeros(4, 16, device=DEV), B_d, ids[:3], torch.zeros(4, 50, device=DEV))
    with pytest.raises(TypeError):
        ops.lora_bank_shrink(x, A_d, ids.long())
    with pytest.raises(ValueError, match="RMSNorm prologue needs alpha"):
        ops.lora_bank_shrink(x, A_d, ids, prologue=ops.PROLOGUE_RMSNORM)
    with pytest.raises(ValueError, match="K % 8 == 0"):
        ops.lora_bank_shrink(torch.zeros(4, 60, device=DEV), torch.zeros(2, 16, 60, device=DEV, dtype=torch.bfloat16), ids)
    with pytest.raises(ValueError, match="r % 16 == 0"):
        ops.lora_bank_expand(torch.zeros(4, 8, device=DEV), torch.zeros(2, 50, 8, device=DEV, dtype=torch.bfloat16), ids, torch.zeros(4, 50, device=DEV))
