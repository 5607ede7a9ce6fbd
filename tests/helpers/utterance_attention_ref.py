"""attention_kernel<D, QKV> of csrc/attention.hip (behind ops.attention, ops.attention_qkv and, with a ring, ops.attention(ring=True) past
the few-query path) restated for tests that hold every launch to fp64 at DESIGNED scores: the case table of the whole-utterance forms,
the designed operands and score profiles, a reference of the window definition in fp64 or fp32 that can carry one named defect, the
launcher's geometry (`geometry`) and the acceptance.  Nothing here needs a GPU until `device_run` is called.  The ring walk of the same
kernel is a set of `qpre` cases of tests/helpers/ring_attention_ref.py (`WALK_CASES`): ring map, poison, reference and acceptance are
that helper's, and `reference` here passes them through.  The tolerance constants, the ring map and `tolerance` are imported, not
restated.

Geometry.  One wave per 32-query tile, 32-key tiles staged through LDS, the eight tiles of a 256-query group split over two workgroups
("twins") as {0, 2, 5, 7} and {1, 3, 4, 6}.  A workgroup stages the key tiles s_begin, s_begin + 32, .. <= hi_wg; a wave skips a staged
tile outside its own [lo, hi], takes it whole when it is `interior` (every key visible to every query of the wave's tile) and masks it
per element otherwise.  `kernel_mask` rebuilds the visibility of every (query, key) from that walk; without a defect it must equal the
window definition j <= i, i - j < context (tests/test_utterance_attention_bounds_cpu.py asserts it on every case).

Designed scores.  Per (stream, head) one randn direction u: the ROTATED query of position t is u + 0.05 randn orthogonal to u, the
rotated key j is target_j sqrt(D) u / |u|^2 + 0.05 randn orthogonal to u, so query t scores key j at target_j + O(0.01), the same
for every query.  v is randn.  `plain` takes these rounded to fp32.  `fused` takes them rotated back in fp64 by the exact inverse of the
table's (cos, sin) bytes -- the table ops.rope_table returned for the launch, or `cpu_table`, the same arithmetic in torch -- then
rounded to fp32, in the layout "b t (p h d)"; every head and every third of a row holds values of its own.  The reference always works
from the achieved scores of the fp32 bytes.  Profiles, target_j by key position j (`tile` = j // 32, Wd = context or T):
  flat          0.5 randn
  low / high    every score in [-90, -80] / [80, 90]
  ramp_up       a sawtooth rising by 60 over each period of Wd keys.  The running maximum moves at every key of a period and key
                i + 1 beats key i except across a reset, so a kernel that lets a query see its successor is O(1) off.  In the first
                period (without a context: everywhere) the newest visible key dominates; later the previous period's last key does,
                which is the context edge of the query at the same phase.
  ramp_down     the same falling.  The period's first key dominates every query that sees it: it is the context edge of the
                period's last query, and the key just past the context of the next period's first query.
  ramp_wide     ramp_up over a span of 110: partial sums underflow against the global maximum.
  stairs_first / stairs_last   a background within +-1.5 and a peak on the first / last key of every third key tile, the k-th of
                height 30 + 10 (k mod 8): the running maximum jumps by 10 (30 at the first peak) on a tile's first / last key.

Bound, per (stream, query, head) vector and element: |got_i - ref64_i| <= tol sum_j p_j |v_ji|, p the fp64 probabilities,
tol = max(16 r32, t_op) within [2^-18, 1e-3], r32 the same ratio of the fp32 run of `reference` on the same operands.  t_op = 0 for
every form of this kernel: the scores and the output are fp32 MFMA sums of fp32 products of the stored bytes, the in-load rotation is
the two-product expression the fp32 reference mirrors with the same table bytes, and e^x is v_exp_f32 of x log2 e, about 1e-7
relative on a weight in [0, 1] -- below the 2^-18 floor, and inside 16 r32 wherever |score| is large."""
import math
from dataclasses import dataclass
from functools import lru_cache
from types import SimpleNamespace
from typing import Optional

import torch

from tests.helpers import ring_attention_ref as R
from tests.helpers.depth_frame_ref import TOL_CEIL, TOL_FACTOR, TOL_FLOOR  # noqa: F401  (the bound's constants, used through R.tolerance)

B, H = 2, 2
MAX_PERIOD = 10000.0
TILE, GROUP = 32, 8                          # ATT_GROUP query tiles per group
TWIN_TILES = ((0, 2, 5, 7), (1, 3, 4, 6))    # attention_kernel's wave -> tile map

PROFILES = ("flat", "low", "high", "ramp_up", "ramp_down", "ramp_wide", "stairs_first", "stairs_last")
DEFECTS = ("no_rescale_o", "no_rescale_l", "causal_plus_one", "context_plus_one", "context_minus_one", "diagonal_as_interior",
           "context_edge_as_interior", "stage_one_tile_late", "stage_one_tile_short", "twin_tiles_swapped", "wrong_head_v",
           "table_row_of_tile_start", "q1_slot_visible", "unwritten_slot_visible")
RING_DEFECTS = {"q1_slot_visible": "q1_visible", "unwritten_slot_visible": "end_offset_ignored"}          # R.DEFECTS names
MASK_DEFECTS = ("causal_plus_one", "context_plus_one", "context_minus_one", "diagonal_as_interior", "context_edge_as_interior",
                "stage_one_tile_late", "stage_one_tile_short", "twin_tiles_swapped")


# ---- the case table -----------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    entry: str                      # plain: ops.attention(q, k, v) | fused: ops.attention_qkv(qkv, H)
    D: int
    T: int
    context: Optional[int] = None
    rope: bool = False              # fused: rotate on load
    profiles: tuple = PROFILES


def _cases():
    # (T, context) from the geometry, each with the (entry, D, rope) forms it runs in; every entry reaches every D more than once
    P, F, N = "plain", "fused", "fused-norope"
    table = (
        (1, None, ((P, 64), (F, 32), (N, 128))),              # three waves and the whole twin idle
        (31, None, ((P, 128), (F, 64))),
        (32, None, ((P, 32), (F, 128))),
        (33, None, ((P, 64), (F, 32), (N, 64))),              # the second tile belongs to the twin and holds one query
        (161, None, ((P, 64), (F, 128))),                     # tile 5 (one query) is the twin's last: l_last 4 | 5 apart on tiles 4 / 5
        (225, None, ((P, 128), (F, 32))),                     # tile 7 holds one query
        (256, None, ((P, 64), (F, 128))),
        (257, None, ((P, 32), (F, 64), (P, 128))),            # a second group of one query whose twin has nothing
        (321, None, ((P, 64), (F, 128), (N, 32))),            # a last group where both twins work, l_last 2 | 1
        (545, None, ((P, 128), (F, 64))),                     # three groups
        (700, 250, ((P, 64), (F, 64), (F, 128))),             # the codec's context: s_begin = 256 | 288 in the third group
        (700, 40, ((P, 128), (F, 32), (N, 64))),
        # The tile two before the diagonal, [q0 - 64, q0 - 33], around the context edge.  34: it holds exactly one visible key, for the
        # wave's first query alone.  33: it is skipped by one key, and the tile before the diagonal holds exactly one visible key for
        # the wave's last query.  32: the wave's last query sees nothing of the first tile its wave takes (a lane whose whole tile is
        # masked while its running maximum is still -inf).  1: every query sees only itself, every tile but the diagonal is skipped.
        (700, 34, ((P, 64), (F, 128))),
        (700, 33, ((P, 32), (F, 64))),
        (700, 32, ((P, 128), (F, 32))),
        (700, 1, ((P, 64), (F, 32))),
        (33, 250, ((P, 128), (F, 64), (N, 32))),              # a context longer than the utterance
    )
    out = []
    for T, ctx, forms in table:
        for entry, D in forms:
            name = f"{entry}-t{T}" + (f"-c{ctx}" if ctx else "") + f"-d{D}"
            out.append(Case(name, "plain" if entry == P else "fused", D, T, ctx, rope=entry == F))
    return tuple(out)


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


# ---- the launcher's geometry --------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def geometry(T, context, defect=None):
    """rst_launch_attention's grid and attention_kernel's range arithmetic for a whole-utterance pass (cap = T, pos0 = 0): per
    workgroup `group`, `twin`, `lo_wg`, `s_begin`, `hi_wg`, `l_last`, the `staged` key tiles (their first keys), and per wave `local`,
    `q0`, `has_q`, `lo`, `hi` and the staged tiles it takes as `interior`, `masked` or `skipped`.  ``defect``: one of MASK_DEFECTS that
    changes the walk itself (the per-element ones live in `kernel_mask`)."""
    ctx = context or 0
    cap = T
    wgs = []
    for bx in range(2 * (-(-T // (TILE * GROUP)))):
        grp, twin = bx >> 1, bx & 1
        q_first = grp * TILE * GROUP
        t_last = (T - 1) // TILE - grp * GROUP
        l_last = max([lw for lw in TWIN_TILES[twin] if lw <= t_last], default=-1)
        q_last = q_first + TILE * max(l_last, 0)
        lo_wg, hi_wg = 0, min(cap - 1, q_last + TILE - 1)
        if ctx > 0:
            lo_wg = max(0, q_first + TILE * twin - ctx + 1)
        if l_last < 0:
            hi_wg = -1
        s_begin = lo_wg // TILE * TILE
        staged = list(range(s_begin, hi_wg + 1, TILE))
        if defect == "stage_one_tile_late":
            staged = staged[1:]
        if defect == "stage_one_tile_short":
            staged = staged[:-1]
        waves = []
        for local in TWIN_TILES[twin]:
            if defect == "twin_tiles_swapped" and local in (4, 5):
                local = 9 - local
            q0 = q_first + local * TILE
            has_q = q0 < T
            lo, hi = 0, min(cap - 1, q0 + TILE - 1)
            if ctx > 0:
                lo = max(0, q0 - ctx + 1)
            if not has_q:
                hi = -1
            w = SimpleNamespace(local=local, q0=q0, has_q=has_q, lo=lo, hi=hi, interior=[], masked=[], skipped=[])
            for s0 in staged:
                below = s0 <= q0 if defect == "diagonal_as_interior" else s0 + TILE - 1 <= q0
                inside = ctx <= 0 or q0 + TILE - 1 - s0 < ctx or defect == "context_edge_as_interior"
                if s0 + TILE - 1 < lo or s0 > hi:
                    w.skipped.append(s0)
                elif below and s0 + TILE - 1 < cap and inside:
                    w.interior.append(s0)
                else:
                    w.masked.append(s0)
            waves.append(w)
        wgs.append(SimpleNamespace(group=grp, twin=twin, lo_wg=lo_wg, s_begin=s_begin, hi_wg=hi_wg, l_last=l_last, staged=staged, waves=waves))
    return wgs


@lru_cache(maxsize=None)
def window_mask(T, context):
    """The definition: query i sees key j iff 0 <= i - j (< context)."""
    d = torch.arange(T).view(-1, 1) - torch.arange(T).view(1, -1)
    return (d >= 0) & ((d < context) if context else torch.ones_like(d, dtype=torch.bool))


@lru_cache(maxsize=None)
def kernel_mask(T, context, defect=None):
    """Which (query, key) pairs the kernel's walk lets through ``[T, T]``, rebuilt from `geometry` and the per-element test of a masked
    tile -- with ``defect`` (one of MASK_DEFECTS) as a kernel with that mistake would."""
    ctx = context or 0
    mask = torch.zeros(T, T, dtype=torch.bool)
    for wg in geometry(T, context, defect):
        for w in wg.waves:
            if not w.has_q:
                continue
            q = torch.arange(w.q0, min(w.q0 + TILE, T))
            for s0 in w.interior:
                mask[w.q0:w.q0 + len(q), s0:min(s0 + TILE, T)] = True
            for s0 in w.masked:
                k = torch.arange(s0, min(s0 + TILE, T))
                dlt = q.view(-1, 1) - k.view(1, -1)
                ok = dlt >= (-1 if defect == "causal_plus_one" else 0)
                if ctx > 0:
                    ok &= dlt < ctx + {"context_plus_one": 1, "context_minus_one": -1}.get(defect, 0)
                mask[w.q0:w.q0 + len(q), s0:s0 + len(k)] = ok
    return mask


# ---- rotation ------------------------------------------------------------------------------------------------------------------------------
def cpu_table(T, D):
    """ops.rope_table's arithmetic in torch ``[T, D]`` fp32: (cos, sin) of pair i of position t at [t, 2i], [t, 2i + 1]."""
    fr = torch.exp(torch.arange(D // 2, dtype=torch.float32) * (-math.log(MAX_PERIOD) * 2 / D))
    ang = fr * torch.arange(T, dtype=torch.float32).view(-1, 1)
    return torch.stack([torch.cos(ang), torch.sin(ang)], -1).reshape(T, D)


def rotate(x, table, dtype):
    """x ``[..., T, D]`` (interleaved pairs) by the table's bytes in `dtype`, in the kernel's expressions x0 c - x1 s, x0 s + x1 c."""
    c, s = table.to(dtype)[:, 0::2], table.to(dtype)[:, 1::2]
    a, b = x.to(dtype)[..., 0::2], x.to(dtype)[..., 1::2]
    return torch.stack([a * c - b * s, a * s + b * c], -1).reshape(x.shape)


def _unrotate(y, table):
    """The exact inverse of `rotate` in fp64 (the fp32 (cos, sin) of a row are not of unit length)."""
    c, s = table.double()[:, 0::2], table.double()[:, 1::2]
    n = c * c + s * s
    a, b = y[..., 0::2], y[..., 1::2]
    return torch.stack([(a * c + b * s) / n, (b * c - a * s) / n], -1).reshape(y.shape)


# ---- operands ------------------------------------------------------------------------------------------------------------------------------
def targets(profile, T, context, g):
    """Target score of every key position ``[T]`` fp64."""
    j = torch.arange(T)
    if profile == "flat":
        return 0.5 * torch.randn(T, generator=g, dtype=torch.float64)
    if profile in ("low", "high"):
        t = 89.0 - 8.0 * torch.rand(T, generator=g, dtype=torch.float64)
        return t if profile == "high" else -t
    if profile.startswith("ramp"):
        Wd = context or T
        half = 55.0 if profile == "ramp_wide" else 30.0
        r = -half + 2 * half * (j % Wd).double() / max(Wd - 1, 1)
        return -r if profile == "ramp_down" else r
    at = 0 if profile == "stairs_first" else TILE - 1
    t = (0.5 * torch.randn(T, generator=g, dtype=torch.float64)).clamp(-1.5, 1.5)
    peak = ((j // TILE) % 3 == 0) & (j % TILE == at)
    return torch.where(peak, 30.0 + 10.0 * ((j // TILE // 3) % 8).double(), t)


def build(case, profile, table=None, seed=0):
    """CPU operands of one launch: `q`, `k`, `v` fp32 ``[B, H, T, D]`` as the launch reads them (fused: views of `qkv` ``[B, T, 3 H D]``,
    raw), `table` ``[T, D]`` fp32 where the launch rotates (``table``: the launch's own, else `cpu_table`), and the `targets`."""
    c = case
    T, D = c.T, c.D
    g = torch.Generator().manual_seed(R._seed(c.name, profile, seed))

    def rnd(*shape):
        return torch.randn(*shape, generator=g).double()

    def orth(x, u):
        return x - (x * u).sum(-1, keepdim=True) * u / (u * u).sum(-1, keepdim=True)
    tg = targets(profile, T, c.context, g)
    u = rnd(B, H, 1, D)
    q = u + 0.05 * orth(rnd(B, H, T, D), u)
    k = tg.view(1, 1, T, 1) * math.sqrt(D) * u / (u * u).sum(-1, keepdim=True) + 0.05 * orth(rnd(B, H, T, D), u)
    v = rnd(B, H, T, D)
    out = SimpleNamespace(case=c, profile=profile, targets=tg, table=None, qkv=None)
    if c.entry == "fused":
        if c.rope:
            out.table = (cpu_table(T, D) if table is None else table.detach().cpu().float()).contiguous()
            assert out.table.shape == (T, D)
            q, k = _unrotate(q, out.table), _unrotate(k, out.table)
        out.qkv = torch.stack([q, k, v], 0).permute(1, 3, 0, 2, 4).reshape(B, T, 3 * H * D).float().contiguous()      # "p b h t d -> b t (p h d)"
        out.q, out.k, out.v = out.qkv.view(B, T, 3, H, D).permute(2, 0, 3, 1, 4)
    else:
        out.q, out.k, out.v = q.float().contiguous(), k.float().contiguous(), v.float().contiguous()
    return out


# ---- the reference ------------------------------------------------------------------------------------------------------------------------
def _online(sc, vv, defect):
    """The kernel's online softmax over 32-key tiles (masked scores are -inf) with one of the rescales left out."""
    Bq, Hq, T, _ = sc.shape
    m_run = torch.full((Bq, Hq, T, 1), -math.inf, dtype=sc.dtype)
    l_run = torch.zeros(Bq, Hq, T, 1, dtype=sc.dtype)
    o = torch.zeros(Bq, Hq, T, vv.shape[-1], dtype=sc.dtype)
    for s0 in range(0, sc.shape[-1], TILE):
        s = sc[..., s0:s0 + TILE]
        m_new = torch.maximum(m_run, s.max(-1, keepdim=True).values)
        alpha = torch.where(m_run == -math.inf, torch.ones_like(m_run), torch.exp(m_run - m_new))
        p = torch.where(s == -math.inf, torch.zeros_like(s), torch.exp(s - m_new))
        l_run = l_run * (1.0 if defect == "no_rescale_l" else alpha) + p.sum(-1, keepdim=True)
        o = o * (1.0 if defect == "no_rescale_o" else alpha) + p @ vv[..., s0:s0 + TILE, :]
        m_run = m_new
    return o / l_run


def reference(case, operands, dtype=torch.float64, defect=None):
    """The launch in `dtype` on the operands' fp32 bytes, optionally with one of DEFECTS.  Returns `out` ``[B, T, H, D]``, `den` =
    sum_j p_j |v_j| of the same probabilities, and `scores` ``[B, H, T, T]`` (every pair, masked or not) -- or, for a ring case of
    tests/helpers/ring_attention_ref.py with the operands its `build` made, what that helper's `reference` returns."""
    c, o = case, operands
    if isinstance(c, R.Case):
        return R.reference(c, (o.K, o.V), o.qkv, o.pos, dtype, defect=RING_DEFECTS.get(defect, defect))
    assert defect is None or (defect in DEFECTS and defect not in RING_DEFECTS), defect
    T, D = c.T, c.D
    q, k, v = o.q.to(dtype), o.k.to(dtype), o.v.to(dtype)
    if o.table is not None:
        q = rotate(q, o.table, dtype)
        if defect == "table_row_of_tile_start":
            k = rotate(k, o.table[torch.arange(T) // TILE * TILE], dtype)
        else:
            k = rotate(k, o.table, dtype)
    if defect == "wrong_head_v":
        v = v.roll(1, 1)
    sc = (q @ k.transpose(-1, -2)) * torch.tensor(1.0 / math.sqrt(D), dtype=dtype)          # (fp32: the kernel's rounded 1 / sqrtf(D))
    mask = kernel_mask(T, c.context, defect) if defect in MASK_DEFECTS else window_mask(T, c.context)
    masked = sc.masked_fill(~mask, -math.inf)
    if defect in ("no_rescale_o", "no_rescale_l"):
        out = _online(masked, v, defect)
        p = torch.softmax(masked, -1)
    else:
        p = torch.softmax(masked, -1)
        if defect is not None:
            p = p.nan_to_num(0.0)          # (a query a defect leaves without a key: the launch returns 0)
        out = p @ v
    return SimpleNamespace(out=out.permute(0, 2, 1, 3).contiguous(), den=(p @ v.abs()).permute(0, 2, 1, 3).contiguous(), scores=sc, mask=mask)


# ---- acceptance ---------------------------------------------------------------------------------------------------------------------------
def out_ratio(got_out, ref64):
    """max over every (stream, query, head) vector and element of |got - ref64| / sum_j p_j |v_j|; nan where `got` is not finite."""
    got = got_out.detach().cpu().double().reshape(ref64.out.shape)
    if not bool(torch.isfinite(got).all()):
        return float("nan")
    return float(((got - ref64.out).abs() / ref64.den.clamp_min(1e-300)).max())


def measure(built):
    """The fp64 and fp32 runs of the reference on `built`, r32 and the tolerance (t_op = 0: the module docstring)."""
    ref64 = reference(built.case, built, torch.float64)
    ref32 = reference(built.case, built, torch.float32)
    r32 = out_ratio(ref32.out, ref64)
    return SimpleNamespace(ref64=ref64, ref32=ref32, r32=r32, t_op=0.0, tol=R.tolerance(r32, 0.0))


def accept(got_out, ref64, tol):
    """(within the bound, the worst ratio)."""
    r = out_ratio(got_out, ref64)
    return bool(r <= tol), r


# ---- device side --------------------------------------------------------------------------------------------------------------------------
def device_table(case, dev):
    """The table the fused launch of `case` will read (None: it does not rotate), as CPU bytes for `build`."""
    from rstnet_amd import ops
    return ops.rope_table(case.T, case.D, MAX_PERIOD, dev).cpu() if case.entry == "fused" and case.rope else None


def device_run(built, dev, form=None):
    """One launch of the case's public entry on freshly uploaded operands, each followed by a run of NaN no launch may load.
    ``form``: "plain" / "fused" sends the SAME bytes (a case that does not rotate) through the other entry.  Returns ``[B, T, H, D]``."""
    from rstnet_amd import ops
    c = built.case
    form = form or c.entry
    assert form == c.entry or built.table is None, "the other form reads the same bytes only where nothing rotates"
    if form == "fused":
        qkv = built.qkv if built.qkv is not None else torch.stack([built.q, built.k, built.v], 0).permute(1, 3, 0, 2, 4).reshape(B, c.T, 3 * H * c.D)
        out = ops.attention_qkv(R._guarded(qkv, dev, torch.float32), H, rope=built.table is not None, max_period=MAX_PERIOD, context=c.context)
    else:
        q, k, v = (R._guarded(t.contiguous(), dev, torch.float32) for t in (built.q, built.k, built.v))
        out = ops.attention(q, k, v, context=c.context)
    torch.cuda.synchronize()
    return out.float().cpu().view(B, c.T, H, c.D)
