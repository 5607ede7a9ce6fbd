"""The token sampler (csrc/lm_sample.hip, csrc/lm_sample_impl.h behind ops.lm_sample) restated for its readout tests: which kernel
instance rst_launch_lm_sample picks (`route`), the case tables of tests/test_sampler_readout_gpu.py, logits rows, designed noise, the
reference and a torch emulation of the sampler that can carry one defect.  Nothing here needs a GPU; tests/test_sampler_readout_cpu.py
checks the tables against `route`, the conditions under which the designs are valid, and that the defects are caught.

The noise is an input of the sampler, so it is designed instead of drawn:

  * readout: row r has noise 2^-40 at sorted position r and 2^40 everywhere else, so the winner of row r is whatever the sampler put
    at rank r; the rows of one launch share one logits row and read out its ordered candidate list;
  * pair race: noise[r1] = 1, noise[r2] = (p[r2] / p[r1]) * (1 +- 2^-12) (fp64 ratio), 2^40 elsewhere: the winner flips with the
    sign, which pins the race terms (temperature, maximum, exp) that the 2^80 margin of the readout cannot see.

The sampler orders by the scaled logit, the reference by the rounded fp32 probability.  The two orders agree only where distinct scaled
logits have distinct probabilities, so the random rows here have their near-collisions spread to a gap of at least 2^-15 (`spread`):
|l / t - max| reaches 64, where fp32 numbers are 3.8e-6 apart, and closer logits collapse in the subtraction.  ROW (g) keeps such a
collapse on purpose."""
import functools
from collections import namedtuple

import torch

LO, HI = 2.0 ** -40, 2.0 ** 40
EPS_PAIR = 2.0 ** -12
T_READ = 0.8                       # temperature of the readout launches on kinds (a) (b) (c) (f); (d) (e) (g) run at 1.0
PAIR_TEMPS = (0.7, 1.0, 1.3)
T_NUCLEUS = 1.5                    # flat enough that the 300th probability of a 2048-way row stays above the 1e-5 boundary margin
MAX_ELEMS = 1 << 25                # B * V of one launch
MIN_GAP = 2.0 ** -15
SPLIT_CHUNK, SPLIT_CAP, K_STAGE, BIG_K = 10240, 4096, 8192, 1024

S8, S16, S32, SPLIT, BIG, TOP_P = "sample<256,8>", "sample<256,16>", "sample<1024,32>", "split+merge", "big", "top_p"


# ---- the dispatch -----------------------------------------------------------------------------------------------------------------------
def route(V, top_k, *, sampling=True, top_p=0.0, two_level=True):
    """The kernel rst_launch_lm_sample picks (csrc/lm_sample.hip, the launcher at the end of the file) behind ops.lm_sample, which
    hands over the two-level workspace only when `two_level` is set.  Raises ValueError where the launcher refuses."""
    if sampling and top_p > 0.0:
        return TOP_P
    k = top_k if 0 < top_k < V else V
    if sampling and k > K_STAGE:
        raise ValueError(f"top-k {k} exceeds the {K_STAGE} candidate stage")
    if V <= 2048:
        return S8
    if V <= 4096:
        return S16
    if V <= 32768:
        return S32
    if sampling and k > BIG_K:
        raise ValueError(f"top-k {k} > {BIG_K} for a vocabulary of {V}")
    chunks = -(-V // SPLIT_CHUNK)
    return SPLIT if two_level and chunks * (k if sampling else 1) <= SPLIT_CAP else BIG


def live_ids(V, limit):
    return limit if 0 < limit < V else V


def k_eff(V, k, limit):
    return min(k if k > 0 else V, live_ids(V, limit))


# ---- case tables ------------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "inst V k limit")          # k is the top_k argument (0: the whole vocabulary)


def _topk_cases():
    c = [Case(S8, V, k, 0) for V in (1, 2, 50, 2047, 2048) for k in (1, 25, 250, 0)]
    c += [Case(S8, 2048, 250, 2000), Case(S8, 2048, 250, 100)]
    c += [Case(S16, V, k, 0) for V in (2049, 2050, 4096) for k in (1, 250, 0)]
    c += [Case(S16, 2050, 250, 2049), Case(S16, 2050, 200, 2048)]                # the two audio samplers
    c += [Case(S32, V, k, 0) for V in (4097, 32000, 32768) for k in (1, 25, 1000)]
    c += [Case(S32, 4097, 0, 0), Case(S32, 32768, 8192, 0), Case(S32, 32000, 25, 30000)]
    for V in (32769, 40961, 65536, 151936):          # last chunk: 2049 ids | ONE id | full | 8576 ids
        for k in (1, 25, 100) + ((273,) if V == 151936 else ()):                 # 15 * 273 = 4095: the last k on this route
            for limit in (0, 11, 10240, 10241, 20480, 30000):
                if limit != 11 or k <= 11:
                    c.append(Case(SPLIT, V, k, limit))
    c += [Case(BIG, 151936, k, limit) for k in (274, 1000, 1024) for limit in (0, 30000)]
    return c


TOPK_CASES = _topk_cases()
# kinds (d) (e) (f): one (V, k) per kernel instance
EXTRA_CASES = [Case(S8, 2047, 250, 0), Case(S16, 4096, 250, 0), Case(S32, 32000, 1000, 0), Case(SPLIT, 40961, 100, 0), Case(BIG, 151936, 1000, 0)]
COLLAPSED_CASES = [Case(S8, 2048, 8, 0), Case(S8, 2048, 4, 0), Case(SPLIT, 40000, 8, 0), Case(SPLIT, 40000, 4, 0)]
GREEDY_V = sorted({c.V for c in TOPK_CASES})
NucleusCase = namedtuple("NucleusCase", "V m")       # m: the nucleus size aimed at (clipped to the ids that may be drawn)
NUCLEUS_CASES = [NucleusCase(2, 1), NucleusCase(2, 2), NucleusCase(50, 1), NucleusCase(50, 5), NucleusCase(2048, 1), NucleusCase(2048, 7),
                 NucleusCase(2048, 300), NucleusCase(2049, 5), NucleusCase(2049, 300), NucleusCase(32000, 1), NucleusCase(32000, 8),
                 NucleusCase(32000, 300), NucleusCase(151936, 6), NucleusCase(151936, 200)]


def case_id(c):
    return "-".join(f"{f}{v}" for f, v in zip(("", "V", "k", "L"), c)).replace("sample", "s").replace("<", "").replace(">", "").replace(",", "x")


def routes_of(c):
    """(two_level flag, instance) of every launch form a case runs: the split + merge cases run again on the one-workgroup kernel."""
    return [(True, c.inst)] + ([(False, BIG)] if c.inst == SPLIT else [])


# ---- logits rows ------------------------------------------------------------------------------------------------------------------------
def _gen(*key):
    s = 0
    for v in key:
        s = (s * 1000003 + (v if isinstance(v, int) else sum(map(ord, v)))) % (1 << 62)
    return torch.Generator().manual_seed(s)


def spread(l):
    """`l` with every gap between neighbouring values widened to at least MIN_GAP (order, ties aside, kept)."""
    if l.numel() < 2:
        return l
    v, idx = torch.sort(l.double(), stable=True)
    v = torch.cat([v[:1], v[:1] + torch.cumsum(torch.diff(v).clamp_min(MIN_GAP), 0)])
    out = torch.empty_like(l)
    out[idx] = v.float()
    return out


@functools.lru_cache(maxsize=8)
def row_distinct(V, limit=0):
    """(a) 3 * randn.  With a limit the first blanked id holds the row's maximum and the last id the runner-up, so a sampler that
    lets blanked ids race is wrong at rank 0."""
    l = spread(3 * torch.randn(V, generator=_gen("a", V)))
    if 0 < limit < V:
        l[V - 1] = l.max() + 0.25
        l[limit] = l.max() + 0.25
    return l


def tie_targets(n, count):
    """`count` ids below n spread over the row: low, high, middle and the quarters (different lanes, waves and chunks)."""
    want = []
    for t in (1, n - 2, n // 2 + 5, n // 4 + 67, 3 * n // 4 + 133, *range(n)):
        t = min(max(t, 0), n - 1)
        if t not in want:
            want.append(t)
        if len(want) == count:
            break
    return want


def tie_positions(V, k, limit):
    """Sorted positions k-2 .. k+2 among the ids that may be drawn, None when the row has no threshold (k takes them all)."""
    n, ke = live_ids(V, limit), k_eff(V, k, limit)
    return list(range(max(0, ke - 2), min(n - 1, ke + 2) + 1)) if ke < n else None


def row_threshold_tie(V, k, limit):
    """(b) row (a) with the values at sorted positions k-2 .. k+2 replaced by the one at position k and moved to `tie_targets`: the
    top-k takes the two of the five ties with the lowest ids (one of four at k = 1)."""
    l = row_distinct(V, limit).clone()
    pos = tie_positions(V, k, limit)
    if pos is None:
        return None
    n, ke = live_ids(V, limit), k_eff(V, k, limit)
    srt = torch.argsort(l[:n], descending=True, stable=True)
    holders = [int(i) for i in srt[pos]]
    l[holders] = l[srt[ke]].clone()
    want = tie_targets(n, len(pos))
    free = [h for h in holders if h not in want]
    for t in want:
        if t not in holders:
            h = free.pop()
            l[[h, t]] = l[[t, h]]
    return l


@functools.lru_cache(maxsize=8)
def row_plateaus(V):
    """(c) values from {0, 1, 2}."""
    return torch.randint(0, 3, (V,), generator=_gen("c", V)).float()


def row_equal(V):
    return torch.full((V,), 1.5)


def row_few_live(V, m, fill):
    """(d) all but m ids at `fill` (-inf or -3.4e38)."""
    g = _gen("d", V, m)
    l = torch.full((V,), fill)
    m = max(1, min(m, V))
    l[torch.randperm(V, generator=g)[:m]] = spread(3 * torch.randn(m, generator=g))
    return l


def row_zeros(V, leading):
    """(e) +0.0, -0.0 and denormals.  Every probability of these is the same fp32 number, so the reference orders them by id: the values
    descend with the id (positive denormals, a shuffled mix of the two zeros, negative denormals), which makes the order by value the
    same.  `leading`: a few ordinary values are scattered over the row; without them the maximum is the zero plateau, which starts
    with -0.0 at id 0."""
    g = _gen("e", V, int(leading))
    tiny = 2.0 ** -149
    n_pos = V // 4 if leading else 0
    n_neg = V // 4
    n_zero = V - n_pos - n_neg
    zeros = torch.where(torch.rand(n_zero, generator=g) < 0.5, 0.0, -0.0).float()
    if n_zero:
        zeros[0] = -0.0
    if n_zero > 1:
        zeros[1] = 0.0
    pos = torch.arange(n_pos, 0, -1).double() * tiny * 3
    neg = -torch.arange(1, n_neg + 1).double() * tiny * 5
    l = torch.cat([pos.float(), zeros, neg.float()])
    if leading and V >= 16:
        ids = torch.randperm(V, generator=g)[:4]
        l[ids] = torch.tensor([1.0, 0.5, 0.5, -1.0])
    return l


@functools.lru_cache(maxsize=8)
def row_negative(V):
    """(f) -50 + 10 * randn."""
    return spread(-50 + 10 * torch.randn(V, generator=_gen("f", V)))


COLLAPSED_RUN = 8


def row_collapsed(V):
    """(g) eight consecutive fp32 numbers from 0.01 up, increasing with the id, among logits around -20: at temp = 1 their fp32
    probabilities are one number.  Returns (row, the ids of the run in ascending order)."""
    g = _gen("g", V)
    l = -20 + torch.randn(V, generator=g)
    ids = torch.sort(torch.randperm(V, generator=g)[:COLLAPSED_RUN]).values
    v = torch.tensor(0.01)
    for i in ids:
        l[i] = v
        v = torch.nextafter(v, torch.tensor(1.0))
    return l, ids


def kind_rows(c):
    """The readout launches of a top-k case: [(kind, logits row, temp)].  Kind (b) is left out where k takes every id."""
    rows = [("a", row_distinct(c.V, c.limit), T_READ)]
    b = row_threshold_tie(c.V, c.k, c.limit)
    if b is not None:
        rows.append(("b", b, T_READ))
    return rows + [("c3", row_plateaus(c.V), T_READ), ("c1", row_equal(c.V), T_READ)]


def extra_rows(c):
    """Kinds (d) (e) (f) of an EXTRA_CASES entry."""
    m = max(1, k_eff(c.V, c.k, c.limit) // 2)
    return [("d-inf", row_few_live(c.V, m, float("-inf")), 1.0), ("d-3.4e38", row_few_live(c.V, m, -3.4e38), 1.0),
            ("e-lead", row_zeros(c.V, True), 1.0), ("e-zero", row_zeros(c.V, False), 1.0), ("f", row_negative(c.V), T_READ)]


def greedy_rows(V):
    """Every row kind at one V, stacked [rows, V], for the greedy launches."""
    k = min(25, V)
    rows = [row_distinct(V), row_plateaus(V), row_equal(V), row_few_live(V, max(1, k // 2), float("-inf")),
            row_few_live(V, max(1, k // 2), -3.4e38), row_zeros(V, True), row_zeros(V, False), row_negative(V), row_collapsed(V)[0] if V >= 16 else row_equal(V)]
    b = row_threshold_tie(V, 1, 0)       # the tie is for the first place
    return torch.stack(rows + ([b] if b is not None else []))


# ---- reference --------------------------------------------------------------------------------------------------------------------------
Ref = namedtuple("Ref", "probs order p64 scaled")


def reference(l, temp, limit, k):
    """probs = softmax(l / temp) in fp32 over all ids, ids >= limit blanked to 0 afterwards, order = the first min(k, limit or V) ids of
    the stable descending sort.  p64: the same probabilities from an fp64 softmax of the fp32 scaled logits (the noise designs use it)."""
    V = l.numel()
    scaled = l / temp
    probs = torch.softmax(scaled, -1)
    p64 = torch.softmax(scaled.double(), -1)
    n = live_ids(V, limit)
    if n < V:
        probs, p64 = probs.clone(), p64.clone()
        probs[n:] = 0.0
        p64[n:] = 0.0
    order = torch.argsort(probs, descending=True, stable=True)[:k_eff(V, k, limit)]
    return Ref(probs, order, p64, scaled)


def expected(ref, noise):
    """order[argmax(probs[order] / noise)], first maximum, per noise row."""
    return ref.order[(ref.probs[ref.order][None] / noise[:, :ref.order.numel()]).argmax(-1)]


def key_order(ref, limit=0):
    """The order by (scaled logit descending, id ascending) over the ids that may be drawn: what a sampler that compares keys produces."""
    n = live_ids(ref.scaled.numel(), limit)
    return torch.argsort(ref.scaled[:n] + 0.0, descending=True, stable=True)[:ref.order.numel()]


def nucleus_reference(l, temp, limit, top_p):
    """The top_p branch of the oracle's sample_token for one row, with ids >= limit blanked after the softmax.  Returns
    (ps: renormalised survivors' probabilities at their sorted positions, idx: the sorted ids, raw fp64 sorted probabilities)."""
    V = l.numel()
    probs = torch.softmax(l / temp, -1)
    p64 = torch.softmax((l / temp).double(), -1)
    n = live_ids(V, limit)
    if n < V:
        probs, p64 = probs.clone(), p64.clone()
        probs[n:] = 0.0
        p64[n:] = 0.0
    ps, idx = torch.sort(probs, dim=-1, descending=True, stable=True)
    mask = torch.cumsum(ps, -1) - ps > top_p
    ps = ps * (~mask).float()
    return ps / ps.sum(), idx, p64[idx]


def nucleus_expected(ps, idx, noise):
    return idx[(ps[None] / noise).argmax(-1)]


def nucleus_top_p(l, temp, limit, m):
    """(top_p, m): top_p halfway between the fp64 exclusive prefix sums at sorted positions m-1 and m, so that exactly m entries survive
    (m clipped to the ids that may be drawn)."""
    n = live_ids(l.numel(), limit)
    m = min(m, n)
    _, _, p64 = nucleus_reference(l, temp, limit, 1.0)
    excl = torch.cat([torch.zeros(1, dtype=torch.float64), torch.cumsum(p64, 0)])          # excl[j] = sum of the first j
    return float(0.5 * (excl[m - 1] + excl[m])), m


def nucleus_rows(V):
    """(kind, row) of a nucleus case: (a) and its quantised image with plateaus inside the nucleus."""
    a = row_distinct(V)
    return [("a", a), ("q", (2 * a).round() / 2)]


# ---- noise designs ----------------------------------------------------------------------------------------------------------------------
def read_ranks(kk, seed=0):
    """Every rank below kk up to 256; above, ranks 0..7, kk-8..kk-1 and 112 more: 56 evenly strided, 56 seeded-random."""
    if kk <= 256:
        return list(range(kk))
    picked = set(range(8)) | set(range(kk - 8, kk))
    picked |= {8 + (i * (kk - 16)) // 56 for i in range(56)}
    rest = torch.tensor(sorted(set(range(kk)) - picked))
    picked |= {int(r) for r in rest[torch.randperm(rest.numel(), generator=_gen("ranks", kk, seed))[:128 - len(picked)]]}
    return sorted(picked)


def readout_noise(positions, width, device="cpu"):
    """[len(positions), width]: 2^-40 at (row i, positions[i]), 2^40 elsewhere."""
    noise = torch.full((len(positions), width), HI, device=device)
    noise[torch.arange(len(positions), device=device), torch.as_tensor(positions, device=device)] = LO
    return noise


def pair_ranks(ref, seed):
    """(0, 1), (0, k-1), (k/2, k-1) and 5 seeded pairs r1 < r2 among the ranks of positive probability whose first member is within
    2^30 of the largest probability (everything else races with noise 2^40 and has to lose to a term p[r1] / 1)."""
    p = ref.p64[ref.order]
    kk = int((p > 0).sum())
    if kk < 2:
        return []
    pairs = [(0, 1), (0, kk - 1), (kk // 2, kk - 1)]
    near = int((p[:kk] * 2.0 ** 30 > p[0]).sum())
    g = _gen("pairs", kk, seed)
    for _ in range(5):
        r1 = int(torch.randint(0, min(near, kk - 1), (1,), generator=g))
        pairs.append((r1, int(torch.randint(r1 + 1, kk, (1,), generator=g))))
    return [(a, b) for a, b in pairs if a != b]


def pair_noise(ref, pairs):
    """Two rows per pair, (+) then (-): returns (noise [2 * pairs, k], the designed winners)."""
    p = ref.p64[ref.order]
    noise = torch.full((2 * len(pairs), ref.order.numel()), HI)
    win = []
    for i, (r1, r2) in enumerate(pairs):
        for s, sign in enumerate((1.0, -1.0)):
            noise[2 * i + s, r1] = 1.0
            noise[2 * i + s, r2] = float(p[r2] / p[r1]) * (1.0 + sign * EPS_PAIR)
            win.append(int(ref.order[r1 if sign > 0 else r2]))
    return noise, torch.tensor(win)


# ---- a sampler in torch that can carry one defect ---------------------------------------------------------------------------------------
DEFECTS = ("kth_is_next", "swap_last_two", "ties_to_highest_id", "swap_2_3", "no_temperature", "blanked_stay")


def emulate(l, temp, limit, k, noise, defect=None):
    """ops.lm_sample's top-k sampling for one logits row and noise [B, k] in plain torch; `defect` injects one of DEFECTS."""
    V = l.numel()
    probs = torch.softmax(l / (1.0 if defect == "no_temperature" else temp), -1)
    n = live_ids(V, limit)
    if n < V and defect != "blanked_stay":
        probs = probs.clone()
        probs[n:] = 0.0
    kk = k_eff(V, k, limit)
    if defect == "ties_to_highest_id":
        full = V - 1 - torch.argsort(probs.flip(0), descending=True, stable=True)
    else:
        full = torch.argsort(probs, descending=True, stable=True)
    order = full[:kk].clone()
    if defect == "kth_is_next" and kk < V:
        order[kk - 1] = full[kk]
    if defect == "swap_last_two" and kk >= 2:
        order[[kk - 1, kk - 2]] = order[[kk - 2, kk - 1]]
    if defect == "swap_2_3" and kk >= 4:
        order[[2, 3]] = order[[3, 2]]
    return order[(probs[order][None] / noise[:, :kk]).argmax(-1)]
