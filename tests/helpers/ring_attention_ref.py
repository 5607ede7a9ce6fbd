"""The launch-per-op ring attention (csrc/lm_attn.hip behind ops.lm_attn_decode and ops.attention(ring=True), csrc/lm_prefill.hip behind
ops.lm_attn_prefill / ops.lm_ring_append[_ragged], the short-ring prologue of rst_gemv_attn_bf16_f32 behind ops.gemv_attn, and the tile
walk of csrc/attention.hip that ops.attention(ring=True) takes with more than 8 queries or a head dim of 32: the `walk-` cases) restated for
tests that hold every launch to fp64 at DESIGNED scores: the case table, a builder of the ring as that many single steps would have
left it, the score profiles and the poison, a reference of the window definition in any dtype that can carry one named defect, the
launchers' dispatch (`instance`) and the acceptance function.  Nothing here needs a GPU until `device_run` is called;
tests/test_ring_attention_bounds_cpu.py checks the ring map against oracle.lm_oracle.RingKV, the designed scores, that the fp32
reference stands inside its bound, that every defect is rejected by a named (case, profile), and the table's coverage.

The ring is an input (model: tests/helpers/temporal_frame_ref.py, whose slot -> position map is imported, not restated): a case names
the positions it is run at, `pos_dev` is set directly, and every (case, profile, position) is one launch.

Designed scores.  Per stream and KV head one direction u (randn) is the ROTATED query of every query head of the group and of every
chunk row; the raw query is u rotated back in fp64 by the reference's fp32 angle (gemv / q_pre entries take u as it is).  Stored key j
is target_j sqrt(D) u / |u|^2 plus 0.05 randn orthogonal to u, rounded to the ring's dtype; keys that enter through qkv (the step's own,
the chunk's) are rotated back the same way.  The reference always uses the achieved scores of the bytes, never the targets.  Profiles:
  flat             keys 0.5 randn (the distribution of the existing tests)
  peak@oldest|own|split_first|split_last   one visible key 40 above all others (others within +-1.5): at the oldest visible position,
                   at the last query's own key, at the first slot of the last split that has a visible one, at the highest visible
                   slot.  A "split" is what `instance(...).unit` says: `per` slots (split kernels), a pass of 8 slots (short rings),
                   a 32-key tile counted from the last query block's first key (prefill; there split_last is the last key of the
                   first tile, the last key of the last tile being the own key).
  low / high       every score in [-90, -80] / [80, 90]
  ramp_up / ramp_down   monotone over a span of 60 in slot order (prefill: position order): the running maximum changes at every
                   key, or never.  Ring keys are re-assigned by their ACHIEVED score after rounding, so they are exactly monotone;
                   a key that enters through qkv is rounded by the launch and sits within 0.5 of its target.
  ramp_wide        the same over a span of 110: partials underflow against the global maximum.
  flat/k0          flat with the second poison variant.
`Case.smax` shrinks these for prefill_attn_bf16_kernel (see t_op below): |score| <= 31, i.e. peak 30 over others at -11.5, low / high
[-30, -22] / [22, 30], ramp_wide a span of 62 -- there it cannot underflow, which the f32 prefill cases and the split kernels cover.

Poison (always finite) sits in every slot or row no query of the launch may see: positions outside every window, slots at or beyond
end_offset, the Q1 slot (end_offset % cap counts as the future), the step's own stale slot, chunk rows at or past a ragged length:
V = +-2^14 and a key along u whose score would be 40 above the visible maximum (`dominant`: a kernel that sees it returns ~2^14
instead of ~1), or K = 0 (`k0`, as tests/test_temporal_frame_steps_gpu.py).  The other KV heads of a grouped layout hold their own
group's rows: independent randn values, an O(1) error for a query head that reads them (defect `kv_head_h`).

Bound, per (stream, query, head) vector and element: |got_i - ref64_i| <= tol sum_j p_j |v_ji|, p the fp64 probabilities.
tol = max(16 r32, t_op) within [2^-18, 1e-3]; r32 the same ratio of the fp32 run of `reference` on the same operands.  t_op, from the
code:
  * attn_small / attn_decode / attn_decode_dense / prefill_attn_f32 / gemv prologue / attention_kernel's ring walk: fp32 FMAs (fp32
    MFMAs) on the stored bytes: 0.
  * packed output (store_packed8): the result leaves as bf16 hi + lo, |x - hi - lo| <= 2^-16 |x| (lm_common.h): 2^-16.
  * prefill_attn_bf16_kernel: Q enters the score MFMA as hi + lo planes, so score j is off by at most 2^-16 sum_i |q_i k_ji| / sqrt(D)
    =: e_j; a weight exp(s_j - M) / L moves by e_j in the numerator and max e in L: 2 max_j e_j relative.  The probabilities enter the
    second MFMA as hi + lo: 2^-16 more.  t_op = 2 * 2^-16 * max_j sum_i |q_i k_ji| / sqrt(D) + 2^-16.  It reaches the 1e-3 ceiling at
    |score| ~ 32, hence smax = 31 for that kernel.
In-launch rotation (attn_small / attn_decode with rope): the launch's frequency is expf(i * coef), the reference's torch.exp of the same
fp32 argument; they may differ by an ulp, which the position multiplies (lm_prefill.hip's stage_kernel records 1.9e-4 at position 3000
and takes a frequency table for that reason).  An ulp of a frequency near 1 turns a pair by pos * 2^-23 rad, i.e. moves a stored key
by up to pos * 2^-23 * sqrt(2) of the row's largest element; that stays under the 2^-18 floor of the tolerance up to position 22
(ROPE_POS_LIMIT), so cases with in-launch or table rotation stay at positions <= 22 and the wrapped long rings run without rotation.
Prefill takes the reference's frequency table and rotates at any position; against single steps it is compared with rotation only
where the steps stay under that limit, and without rotation everywhere else."""
import math
from dataclasses import dataclass, replace
from functools import lru_cache
from types import SimpleNamespace
from typing import Optional

import torch

from tests.helpers.depth_frame_ref import TOL_CEIL, TOL_FACTOR, TOL_FLOOR
from tests.helpers.temporal_frame_ref import half_ulp_bf16, slot_position, visible_slots

MAX_PERIOD = 10000.0
POISON = 2.0 ** 14
MARGIN = 40.0
ROPE_POS_LIMIT = 22          # in-launch / table rotation: see the module docstring
LM_ATTN_MAX_SPLITS = 16      # ops.LM_ATTN_MAX_SPLITS

PROFILES = ("flat", "peak@oldest", "peak@own", "peak@split_first", "peak@split_last", "low", "high", "ramp_up", "ramp_down", "ramp_wide",
            "flat/k0")
PEAKS = tuple(p for p in PROFILES if p.startswith("peak"))


# ---- the case table -----------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    entry: str                      # decode: ops.lm_attn_decode | gemv: ops.gemv_attn | prefill: ops.lm_attn_prefill + append | qpre: ops.attention
    B: int                          # 0: the fewest streams the dense kernel takes on this device (`resolve`)
    H: int
    G: int
    D: int
    cap: int
    context: Optional[int]          # decode / gemv / qpre: the context (None: the whole ring); prefill: the window
    kv: str                         # "f32" | "bf16" rings
    positions: tuple                # each an int (one position for all streams) or a tuple of B ints (per-stream positions)
    rope: str = "off"               # "off" | "launch" (computed by the launch) | "table" (ops.lm_rope_table; prefill: its frequency table)
    rope_dims: int = 0              # leading head dims that rotate (0: all)
    T: int = 1                      # chunk rows (prefill: Tc) / queries (qpre)
    lengths: Optional[tuple] = None  # prefill: ragged lengths of the append
    packed: bool = False            # decode: out_packed, read back through tests/helpers/lm_operands.py
    weight: str = "eye"             # gemv: the out-projection
    smax: float = 100.0             # largest designed |score| (31: shrunk for prefill_attn_bf16_kernel)
    profiles: tuple = PROFILES


def _pf(name, B, H, G, D, cap, W, T, positions, rope="table", lengths=None):
    """A prefill case for both ring dtypes: prefill_attn_f32_kernel and prefill_attn_bf16_kernel (|score| <= 31, see t_op)."""
    return (Case(f"pf-{name}-f32", "prefill", B, H, G, D, cap, W, "f32", positions, rope, 0, T, lengths),
            Case(f"pf-{name}-bf16", "prefill", B, H, G, D, cap, W, "bf16", positions, rope, 0, T, lengths, smax=31.0))


CASES = (
    # -- ops.lm_attn_decode, short rings (attn_small_kernel): one pass of 3 slots, one full pass, eight passes
    Case("small-c3-d64", "decode", 2, 2, 2, 64, 3, None, "f32", (0, 1, 2, 3, 7, 11), "launch"),
    Case("small-c8-d128", "decode", 2, 4, 4, 128, 8, None, "f32", (0, 5, 7, 8, 20), "off"),
    Case("small-c8-d32", "decode", 2, 2, 2, 32, 8, 5, "f32", (3, 7, 8, 21), "launch"),
    Case("small-c64-d64-ctx", "decode", 2, 2, 2, 64, 64, 40, "f32", (10, 63, 64, 150), "off"),
    Case("small-c64-d64-rope-packed", "decode", 2, 2, 2, 64, 64, None, "f32", (9, 22), "launch", packed=True),
    Case("small-c64-d128-gqa", "decode", 2, 4, 2, 128, 64, None, "f32", (63, 200), "off"),
    Case("small-c4-ps", "decode", 4, 2, 2, 64, 4, None, "f32", ((2, 3, 4, 19), 2, 3, 4, 19), "launch"),
    # -- the split kernel with one split (cap 130) and two (cap 300), fp32 and bf16 rings, in-launch / table rotation while the ring fills
    Case("split-c130-d64-f32", "decode", 2, 2, 2, 64, 130, None, "f32", (63, 64, 128, 129, 130, 397), "off"),
    Case("split-c130-d64-f32-rope", "decode", 2, 2, 2, 64, 130, None, "f32", (0, 15, 22), "launch"),
    Case("split-c130-d128-bf16", "decode", 2, 2, 2, 128, 130, 100, "bf16", (5, 129, 130, 397), "off"),
    Case("split-c130-d128-bf16-table", "decode", 2, 2, 2, 128, 130, None, "bf16", (0, 22), "table"),
    Case("split-c300-d128-f32", "decode", 2, 2, 2, 128, 300, None, "f32", (100, 299, 300, 907), "off"),
    Case("split-c300-d128-f32-ropedims", "decode", 2, 2, 2, 128, 300, None, "f32", (22,), "table", rope_dims=64),
    Case("split-c300-d64-bf16-gqa2", "decode", 2, 4, 2, 64, 300, 200, "bf16", (150, 299, 300, 907), "off", packed=True),
    Case("split-c300-d64-f32-gqa4", "decode", 1, 8, 2, 64, 300, None, "f32", (299, 641), "off"),
    # -- more than eight active splits (the combine reads eight at a time): 10 at pos 600, 16 on the full and the wrapped ring
    Case("many-c2048-d64-f32", "decode", 1, 2, 2, 64, 2048, None, "f32", (600, 2047, 2048, 6151), "off"),
    Case("many-c2048-d128-bf16", "decode", 1, 2, 2, 128, 2048, 1500, "bf16", (575, 576, 6151), "off"),
    # -- the dense kernel: B * 32 heads > 3 x CUs workgroups of one split
    Case("dense-d64-f32", "decode", 0, 32, 8, 64, 70, None, "f32", (69, 70, 217), "off"),
    Case("dense-d128-f32", "decode", 0, 32, 8, 128, 70, 15, "f32", (22,), "launch"),
    Case("dense-d64-bf16", "decode", 0, 32, 16, 64, 70, None, "bf16", (70, 217), "off"),
    Case("dense-d128-bf16", "decode", 0, 32, 8, 128, 70, None, "bf16", (69, 217), "off"),
    # -- per-stream positions in four phases at once (not full, cap - 1, cap, 3 cap + 7), then the shared launch at each of them
    Case("ps-c130-d64-f32", "decode", 4, 2, 2, 64, 130, None, "f32", ((57, 129, 130, 397), 57, 129, 130, 397), "off"),
    Case("ps-c300-d128-bf16-gqa", "decode", 4, 4, 2, 128, 300, 250, "bf16", ((100, 299, 300, 907), 100, 299, 300, 907), "off"),
    Case("ps-c130-d64-f32-table", "decode", 4, 2, 2, 64, 130, None, "f32", ((0, 7, 15, 22),), "table"),
    # -- ops.gemv_attn: the depth transformer's 16 x 64 on a ring of 8, wrapped rings of 2 and 3, a context shorter than the ring
    Case("gemv-c8", "gemv", 1, 16, 16, 64, 8, None, "f32", (0, 3, 7, 8, 21)),
    Case("gemv-c8-b2-ctx3", "gemv", 2, 16, 16, 64, 8, 3, "f32", (1, 7, 8, 21)),
    Case("gemv-c2", "gemv", 2, 16, 16, 64, 2, None, "f32", (1, 2, 3, 4, 5)),
    Case("gemv-c3", "gemv", 1, 16, 16, 64, 3, None, "f32", (2, 3, 4, 7)),
    Case("gemv-c8-randn", "gemv", 2, 16, 16, 64, 8, None, "f32", (5, 21), weight="randn", profiles=("flat", "peak@oldest", "high", "ramp_up")),
    # -- ops.lm_attn_prefill + ops.lm_ring_append: Tc 1 / 31 / 32 / 33 around the 32-query tile, windows 31 / 32 / 33 around the 32-key tile
    *_pf("t1-w31-d64", 2, 2, 2, 64, 70, 31, 1, (0, 20, 69, 100)),
    *_pf("t31-w32-d128", 2, 2, 2, 128, 70, 32, 31, (0, 9, 50, 139)),
    *_pf("t32-w33-d64", 2, 2, 2, 64, 70, 33, 32, (0, 60)),
    # ten key tiles (four waves taking every fourth), an empty ring, a window across the wrap, a wrapped ring
    *_pf("t33-w299-d128", 1, 2, 2, 128, 300, 299, 33, (0, 280, 650)),
    *_pf("t33-w299-d64", 2, 2, 2, 64, 300, 299, 33, (7, 290)),
    # Tc = cap: every slot is appended; the last queries no longer see the first chunk rows
    *_pf("t70-w69-d64", 1, 2, 2, 64, 70, 69, 70, (0, 35, 200), rope="off"),
    *_pf("t33-w140-d128-gqa", 2, 4, 2, 128, 300, 140, 33, (8, 290)),
    *_pf("t33-w140-d64-gqa4", 1, 8, 2, 64, 300, 140, 33, (290,), rope="off"),
    # per-stream positions with ragged lengths: nothing, all of the chunk, a few rows, all but one
    *_pf("ragged-d64", 4, 2, 2, 64, 130, 129, 32, ((0, 100, 129, 397),), lengths=(0, 32, 5, 31)),
    *_pf("ragged-d128", 4, 2, 2, 128, 130, 100, 33, ((3, 120, 130, 300), 120), lengths=(33, 0, 1, 32)),
    # -- ops.attention(ring=True) with T > 1 (`lm/stack.py`): queries already rotated, keys already in the ring
    Case("qpre-d64", "qpre", 2, 2, 2, 64, 130, None, "f32", (0, 50, 127, 300), T=3, profiles=("flat",) + PEAKS),
    Case("qpre-d128-gqa", "qpre", 2, 4, 2, 128, 300, 100, "f32", (40, 298, 905), T=2, profiles=("flat",) + PEAKS),
    # -- the same entry past the few-query path (T > 8, or D = 32 at any T): attention_kernel<D> of csrc/attention.hip walks the ring in
    # 32-slot tiles.  An empty ring, a filling one, a chunk across the wrap, a ring wrapped twice; T = cap, where slot end_offset % cap
    # is the FIRST query's own key and counts as the future (that query sees nothing: the launch returns 0 for it)
    Case("walk-c250-d64-t12", "qpre", 2, 2, 2, 64, 250, 250, "f32", (0, 100, 245, 738), T=12),
    Case("walk-c70-d128-t40", "qpre", 2, 2, 2, 128, 70, None, "f32", (0, 50, 200), T=40),
    Case("walk-c10-d32-t3", "qpre", 2, 2, 2, 32, 10, 7, "f32", (0, 8, 25), T=3),
    Case("walk-c33-d64-t33", "qpre", 2, 2, 2, 64, 33, None, "f32", (0, 40), T=33),
)
WALK_CASES = tuple(c.name for c in CASES if c.name.startswith("walk-"))
BY_NAME = {c.name: c for c in CASES}

# Every kernel instance (template arguments) the three launchers reach, plus the run-time forms the issue names
REACHABLE = frozenset(
    [f"attn_small<{D}>" for D in (32, 64, 128)] +
    [f"{k}<{D},{kv}>" for k in ("attn_decode", "attn_decode_dense") for D in (64, 128) for kv in ("f32", "bf16")] +
    [f"prefill_attn_{kv}<{D}>" for kv in ("f32", "bf16") for D in (64, 128)] + ["stage<f32>", "stage<bf16>", "stage<f32>:ring", "stage<bf16>:ring"] +
    ["gemv_attn<1>", "gemv_attn<2>", "q_pre:T>1<64>", "q_pre:T>1<128>", "splits>8", "splits=1", "splits=2", "per_stream", "rope_table", "packed",
     "gqa2", "gqa4", "ragged", "rope_dims<D"] + [f"attention<{D}>:ring" for D in (32, 64, 128)])


def resolve(case, cus):
    """The dense cases sized from the device's CU count: the fewest streams with B * H * splits > 3 x CUs."""
    if case.B:
        return case
    return replace(case, B=3 * cus // (case.H * lm_attn_splits(case.cap, 1)) + 1)


def lm_attn_splits(cap, pairs):
    """ops.lm_attn_splits."""
    return max(1, min(LM_ATTN_MAX_SPLITS, cap // 128, 1024 // max(1, pairs)))


def instance(case, cus, pos=None):
    """Which kernel rst_launch_lm_attn / rst_launch_lm_attn_prefill / rst_launch_gemv dispatch `case` to on a device of `cus` CUs, with
    how many splits, and (with `pos`, the launch's first new position) how many of them are active and how many slots each takes.
    `unit`: what the peak@split_* profiles call a split.  `names`: the members of REACHABLE the case stands for."""
    c = resolve(case, cus)
    kv = c.kv
    names = set()
    out = SimpleNamespace(case=c, splits=1, active=1, per=c.cap, unit=8, dense=False)
    if c.entry == "gemv":
        out.kernel = f"gemv_attn<{c.B}>"
    elif c.entry == "prefill":
        out.kernel = f"prefill_attn_{kv}<{c.D}>"
        out.unit = 32
        names |= {f"stage<{kv}>", f"stage<{kv}>:ring"}
        if c.lengths:
            names.add("ragged")
    else:
        T = c.T if c.entry == "qpre" else 1
        walk = False
        if c.entry == "qpre":          # ops.attention: the few-query ring path, else the tile walk of attention_kernel<D>
            walk = not ((T <= 8 or c.G != c.H) and c.D in (64, 128))
            assert not walk or c.G == c.H, "grouped key/value heads are served by the few-query path only"
            out.splits = 1 if walk else max(1, min(4, c.cap // 64, 1024 // max(1, c.B * T * c.H)))
        else:
            out.splits = 1 if c.cap <= 64 else lm_attn_splits(c.cap, c.B * c.H)
        if walk:
            out.kernel = f"attention<{c.D}>:ring"
            out.unit = 32
        elif c.entry == "decode" and c.cap <= 64 and out.splits == 1:
            assert kv == "f32", "bf16 rings are served by the long-ring form only"
            out.kernel = f"attn_small<{c.D}>"
        else:
            out.dense = out.splits * c.H * c.B * T > 3 * cus
            out.kernel = f"{'attn_decode_dense' if out.dense else 'attn_decode'}<{c.D},{kv}>"
            out.unit = None
            if c.entry == "qpre":
                names.add(f"q_pre:T>1<{c.D}>")
            if pos is not None:
                n_used = min(c.cap, pos + T)
                out.active = max(1, min(out.splits, -(-n_used // 64)))
                out.per = out.unit = -(-n_used // out.active)
                names.add("splits>8" if out.active > 8 else f"splits={out.active}")
    names.add(out.kernel)
    if any(isinstance(p, tuple) for p in c.positions):
        names.add("per_stream")
    if c.rope == "table" and c.entry == "decode":
        names.add("rope_table")
    if c.packed:
        names.add("packed")
    if c.H != c.G:
        names.add(f"gqa{c.H // c.G}")
    if c.rope_dims and c.rope_dims < c.D:
        names.add("rope_dims<D")
    out.names = frozenset(names)
    return out


def case_names(case, cus):
    """Every member of REACHABLE `case` stands for over all its positions."""
    out = set()
    for position in case.positions:
        for p in set(stream_pos(resolve(case, cus), position)):
            out |= instance(case, cus, p).names
    return frozenset(out) & REACHABLE


def stream_pos(case, position):
    return list(position) if isinstance(position, tuple) else [position] * case.B


def ring_dtype(case):
    return torch.bfloat16 if case.kv == "bf16" else torch.float32


def round_to_ring(t, case):
    return t.float().to(ring_dtype(case)).to(t.dtype)


# ---- the ring map --------------------------------------------------------------------------------------------------------------------------
def held(slot, n, cap):
    """The position ring slot `slot` physically holds after `n` single steps (None: unwritten) -- `slot_position` without its relabelling
    of slot n % cap as the future."""
    p = slot_position(slot, n - 1, cap)
    return p - cap if p == n else p


@lru_cache(maxsize=None)
def queries(case, P):
    """Per query t of a stream whose launch starts at position P: the keys it sees as (kind, index, position) in the launch's order --
    ("ring", slot, p) read from the ring, ("new", row, p) taken from the launch's own qkv rows."""
    cap, ctx, T = case.cap, case.context, case.T
    out = []
    if case.entry in ("decode", "gemv"):
        out.append([("new", 0, P) if s == P % cap else ("ring", s, slot_position(s, P, cap)) for s in visible_slots(P, cap, ctx)])
    elif case.entry == "qpre":          # RingKVCache.complete after all T appends; query t at P + t
        for t in range(T):
            row = []
            for s in range(cap):
                p = slot_position(s, P + T - 1, cap)
                if p is not None and 0 <= P + t - p and (not ctx or P + t - p < ctx):
                    row.append(("ring", s, p))
            out.append(row)
    else:                               # the window definition of lm_prefill.hip: positions max(0, p - W + 1) .. p
        for t in range(T):
            out.append([("ring", j % cap, j) if j < P else ("new", j - P, j) for j in range(max(0, P + t - ctx + 1), P + t + 1)])
    return out


def live_queries(case, b):
    """Queries of stream b whose result counts: all, or those below the ragged length."""
    return range(case.T if case.lengths is None else min(case.T, case.lengths[b]))


# ---- rotation ------------------------------------------------------------------------------------------------------------------------------
def angles(case, pos):
    """The reference's fp32 angles of one position ``[D/2]`` (modules/rope.py: fp32 frequency table times the fp32 position), 0 where
    nothing rotates."""
    a = torch.zeros(case.D // 2, dtype=torch.float32)
    if case.rope != "off":
        n = case.rope_dims or case.D
        fr = torch.exp(torch.arange(n // 2, dtype=torch.float32) * (-math.log(MAX_PERIOD) * 2 / n))
        a[:n // 2] = fr * torch.tensor([pos]).float()
    return a


def rotate(x, ang, dtype, inverse=False):
    """x ``[..., D]`` (interleaved pairs) by the angles ``[D/2]``, cos / sin and the arithmetic in `dtype`."""
    ang = ang.to(dtype)
    c, s = torch.cos(ang), torch.sin(-ang if inverse else ang)
    a, b = x.to(dtype)[..., 0::2], x.to(dtype)[..., 1::2]
    return torch.stack([a * c - b * s, a * s + b * c], -1).reshape(x.shape)


# ---- operands ------------------------------------------------------------------------------------------------------------------------------
def _seed(*parts):
    s = 0
    for ch in "|".join(str(p) for p in parts):
        s = (s * 1000003 + ord(ch)) % (1 << 62)
    return s


def _targets(profile, n, smax, g):
    """Target scores of n keys in ramp order (None: undesigned `flat` keys)."""
    kind = profile.split("/")[0]
    if kind == "flat":
        return None
    if kind.startswith("peak"):
        lo = min(0.0, smax - 1.0 - MARGIN - 1.5)
        return lo + (0.5 * torch.randn(n, generator=g, dtype=torch.float64)).clamp(-1.5, 1.5)          # the peak is set by the caller
    if kind in ("low", "high"):
        e = min(90.0, smax)
        t = e - 1.0 - 8.0 * torch.rand(n, generator=g, dtype=torch.float64)
        return t if kind == "high" else -t
    half = {"ramp_up": 30.0, "ramp_down": 30.0, "ramp_wide": min(55.0, smax)}[kind]
    r = torch.linspace(-half, half, n, dtype=torch.float64) if n > 1 else torch.zeros(1, dtype=torch.float64)
    return r.flip(0) if kind == "ramp_down" else r


def _peak_index(profile, case, keys, P, inst, own):
    """Index into `keys` (ramp order) of the peak key of a peak@... profile; `own`: the position of the last live query."""
    where = profile.split("@")[1]
    if where == "oldest":
        return min(range(len(keys)), key=lambda i: keys[i][2])
    if where == "own":
        return next(i for i, k in enumerate(keys) if k[2] == own)
    if case.entry == "prefill":
        t0 = 32 * ((case.T - 1) // 32)
        u_lo = max(t0 - case.context + 1, -min(P, case.cap))
        coord = [k[2] - P - u_lo for k in keys]
        cand = [i for i, c in enumerate(coord) if c >= 0 and keys[i][2] != own]
        if where == "split_last":
            first = [i for i in cand if coord[i] < 32]
            return max(first or cand, key=lambda i: coord[i]) if cand else 0
    else:
        coord = [k[2] % case.cap for k in keys]
        cand = [i for i, k in enumerate(keys) if k[2] != own]
        if where == "split_last":
            return max(cand, key=lambda i: coord[i]) if cand else 0
    unit = inst.unit or case.cap
    firsts = [i for i in cand if coord[i] % unit == 0]
    if firsts:
        return max(firsts, key=lambda i: coord[i])
    return min(cand, key=lambda i: (coord[i] % unit, -coord[i])) if cand else 0


def build(case, profile, position, seed=0):
    """CPU operands of one launch: `qkv` fp32 ``[B, T, (H + 2G) D]`` (qpre: the rotated queries ``[B, H, T, D]``), the rings `K`, `V` fp32
    ``[B, G, cap, D]`` (numbers the ring's dtype holds) as `pos[b]` single steps would have left them with poison wherever no query of
    the launch may look, and what was designed: `u`, per stream the key list in ramp order, its targets and the peak's key."""
    c = case
    assert c.B, "resolve() the case first"
    kind, variant = (profile.split("/") + ["dominant"])[:2]
    g = torch.Generator().manual_seed(_seed(c.name, profile, position, seed))
    B, H, G, D, cap, T = c.B, c.H, c.G, c.D, c.cap, c.T
    pos = stream_pos(c, position)
    n_new = 0 if c.entry == "qpre" else T

    def rnd(*shape):
        return torch.randn(*shape, generator=g, dtype=torch.float64)
    u = rnd(B, G, D)
    u = u * (math.sqrt(D) / u.norm(dim=-1, keepdim=True))                           # |u|^2 = D: key j = target_j u / sqrt(D) + orthogonal part
    K, V = torch.zeros(B, G, cap, D, dtype=torch.float64), (0.5 * rnd(B, G, cap, D))
    k_new, v_new = torch.zeros(B, G, max(n_new, 1), D, dtype=torch.float64), 0.5 * rnd(B, G, max(n_new, 1), D)
    sign = torch.where(torch.rand(B, G, cap + max(n_new, 1), D, generator=g) < 0.5, -1.0, 1.0).double()
    designed = []
    for b in range(B):
        P = pos[b]
        inst = instance(c, 256, P)
        qs = queries(c, P)
        seen = {}
        for t in live_queries(c, b):
            for k in qs[t]:
                seen[k[:2]] = k
        order = (lambda k: k[2]) if c.entry == "prefill" else (lambda k: (k[2] % cap, k[2]))
        keys = sorted(seen.values(), key=order)
        n = len(keys)
        tg = _targets(profile, n, c.smax, g) if n else None
        peak = None
        if kind.startswith("peak") and n:
            peak = _peak_index(profile, c, keys, P, inst, P + max(live_queries(c, b)))
            if n > 1:
                tg[peak] = float(torch.cat([tg[:peak], tg[peak + 1:]]).max()) + MARGIN
        top = float(tg.max()) if tg is not None and n else 2.0
        for gi in range(G):
            ug = u[b, gi]
            orth = rnd(n, D)
            orth = orth - (orth @ ug).unsqueeze(1) * ug / D
            rows = 0.5 * rnd(n, D) if tg is None else tg.unsqueeze(1) * ug / math.sqrt(D) + 0.05 * orth
            ring_i = [i for i, k in enumerate(keys) if k[0] == "ring"]
            if ring_i:
                ri = torch.tensor(ring_i)
                stored = round_to_ring(rows[ri], c)
                if kind.startswith("ramp"):          # exactly monotone in the achieved scores of the rounded bytes
                    by = torch.argsort(stored @ ug, descending=kind == "ramp_down")
                    stored = stored[by]
                K[b, gi, torch.tensor([keys[i][1] for i in ring_i])] = stored
            for i, k in enumerate(keys):
                if k[0] == "new":
                    k_new[b, gi, k[1]] = rows[i]
            pk = (0.0 if variant == "k0" else top + MARGIN + 1.0) * ug / math.sqrt(D)
            hidden = torch.tensor([("ring", s) not in seen for s in range(cap)])
            K[b, gi, hidden] = pk
            V[b, gi, hidden] = POISON * sign[b, gi, :cap][hidden]
            for t in range(n_new):
                if ("new", t) not in seen:
                    k_new[b, gi, t] = pk
                    v_new[b, gi, t] = POISON * sign[b, gi, cap + t]
        designed.append(SimpleNamespace(keys=keys, targets=tg, peak=None if peak is None else keys[peak]))
    K, V = round_to_ring(K, c).float(), round_to_ring(V, c).float()
    if c.entry == "qpre":
        qkv = u.float()[:, torch.arange(H) // (H // G)].unsqueeze(2).expand(B, H, T, D).contiguous()
    else:
        qkv = torch.zeros(B, T, (H + 2 * G) * D)
        for b in range(B):
            for t in range(T):
                ang = angles(c, pos[b] + t)
                q = rotate(u[b], ang, torch.float64, inverse=True)[torch.arange(H) // (H // G)]
                k = rotate(k_new[b, :, t], ang, torch.float64, inverse=True)
                qkv[b, t] = torch.cat([q.reshape(-1), k.reshape(-1), v_new[b, :, t].reshape(-1)]).float()
    return SimpleNamespace(case=c, profile=profile, position=position, pos=pos, qkv=qkv, K=K, V=V, u=u, designed=designed)


# ---- the reference ------------------------------------------------------------------------------------------------------------------------
DEFECTS = ("window_wide_old", "window_narrow_old", "own_hidden", "q1_visible", "end_offset_ignored", "own_stale", "no_rescale",
           "combine_unscaled", "max_not_subtracted", "q_lo_dropped", "p_lo_dropped", "kv_head_h", "shared_pos", "ragged_row_appended",
           "rope_pos_not_t", "own_unrounded")


def _planes(x, lo=True):
    """split_hi_lo8 of fp32 values (lm_common.h): the truncated bf16 hi plus (``lo``) the residual rounded half-up to bf16, as fp64."""
    x = x.float().contiguous()
    hi = (x.view(torch.int32) & -65536).view(torch.float32)
    if not lo:
        return hi.double()
    r = (x - hi).contiguous()
    return hi.double() + ((r.view(torch.int32) + 0x8000) & -65536).view(torch.float32).double()


def _entries(case, P, t, rows, defect):
    """The key list of query t with the visibility defects applied."""
    cap, T = case.cap, case.T
    rows = list(rows)
    end = P + (T if case.entry == "qpre" else 1 if case.entry != "prefill" else 0)          # appends the ring has seen when it is read
    if defect == "window_wide_old" and rows:
        j = min(r[2] for r in rows) - 1
        n_ring = P if case.entry != "qpre" else P + T
        if j >= 0 and j >= n_ring - cap and not (case.entry in ("decode", "gemv") and j % cap == P % cap):
            rows.append(("ring", j % cap, j))
    if defect == "window_narrow_old" and len(rows) > 1:
        rows.remove(min(rows, key=lambda r: r[2]))
    if defect == "own_hidden":
        rows = [r for r in rows if r[2] != P + t]
    if defect == "q1_visible" and case.entry != "prefill" and end >= cap:
        rows.append(("ring", end % cap, end - cap))
    if defect == "end_offset_ignored" and P < cap:
        if case.entry == "prefill":          # the -pos clamp: keys before position 0 read from the slots they would have
            rows += [("ring", j % cap, j) for j in range(max(P + t - case.context + 1, P - cap), 0)]
        elif end < cap:
            rows += [("ring", s, None) for s in range(end, cap)]
    return rows


def _groups(case, P, t, rows):
    """The partial each key of a query falls into: the split of its slot (split kernels), the wave of its key tile (bf16 prefill), the
    lane of its key (fp32 prefill); one partial elsewhere."""
    inst = instance(case, 256, P)
    if case.entry == "prefill":
        t0 = 32 * (t // 32) if case.kv == "bf16" else t
        u_lo = max(t0 - case.context + 1, -min(P, case.cap))
        if case.kv == "bf16":
            return [((r[2] - P - u_lo) // 32) % 4 if r[2] is not None else 0 for r in rows]
        return [(r[2] - P - u_lo) % 64 if r[2] is not None else 0 for r in rows]
    if inst.unit is None or inst.kernel.startswith(("attn_small", "gemv")):
        return [0] * len(rows)
    return [(r[1] if r[0] == "ring" else P % case.cap) // inst.per for r in rows]


def reference(case, rings, qkv, pos, dtype=torch.float64, defect=None, own=None, planes=False):
    """The launch in `dtype`: `rings` = (K, V) fp32 ``[B, G, cap, D]`` before it, `qkv` as `build` lays it out, `pos` the B first
    positions.  ``own`` = (k, v) ``[B, G, T, D]``: the rows a launch wrote for its new positions -- teacher forcing, the reference attends
    to exactly those bytes -- or None: its own rotated keys / values rounded to the ring's dtype.  ``planes``: Q and the probabilities
    pass through bf16 hi + lo as in prefill_attn_bf16_kernel.  Returns `out` ``[B, T, H, D]``, `den` = sum_j p_j |v_j| of the fp64
    probabilities' kind, `k_new` / `v_new` (unrounded) and `k_row` / `v_row` (as attended) ``[B, G, T, D]``, `K_after` / `V_after` and
    `written` ``[B, T]``, and per (b, t) the achieved scores ``[H, n]`` with their key list."""
    c = case
    B, H, G, D, cap, T = c.B, c.H, c.G, c.D, c.cap, c.T
    K0, V0 = rings
    qpk = H // G
    kvmap = (torch.arange(H) % G) if defect == "kv_head_h" else torch.arange(H) // qpk
    planes = planes or defect in ("q_lo_dropped", "p_lo_dropped")
    out, den = torch.zeros(B, T, H, D, dtype=dtype), torch.zeros(B, T, H, D, dtype=dtype)
    n_new = 0 if c.entry == "qpre" else T
    k_new, v_new = torch.zeros(B, G, max(n_new, 1), D, dtype=dtype), torch.zeros(B, G, max(n_new, 1), D, dtype=dtype)
    k_row, v_row = k_new.clone(), v_new.clone()
    K_after, V_after = K0.clone(), V0.clone()
    written = torch.zeros(B, T, dtype=torch.bool)
    scores, qrot = {}, {}
    for b in range(B):
        P = pos[0] if defect == "shared_pos" else pos[b]
        qs = queries(c, P)
        if c.entry == "qpre":
            q_rot = qkv[b].to(dtype)                                            # [H, T, D]
            Kb, Vb = K0[b].to(dtype), V0[b].to(dtype)
        else:
            raw = qkv[b].view(T, H + 2 * G, D)
            for t in range(T):
                ang = angles(c, P + (0 if defect == "rope_pos_not_t" else t))
                k_new[b, :, t] = rotate(raw[t, H:H + G], ang, dtype)
                v_new[b, :, t] = raw[t, H + G:].to(dtype)
            q_rot = torch.stack([rotate(raw[t, :H], angles(c, P + (0 if defect == "rope_pos_not_t" else t)), dtype) for t in range(T)], 1)
            if own is not None:
                k_row[b], v_row[b] = own[0][b].to(dtype), own[1][b].to(dtype)
            else:
                k_row[b], v_row[b] = round_to_ring(k_new[b], c), round_to_ring(v_new[b], c)
            if defect == "own_unrounded":
                k_row[b], v_row[b] = k_new[b], v_new[b]
            if defect == "own_stale":
                for t in range(T):
                    k_row[b, :, t], v_row[b, :, t] = K0[b, :, (P + t) % cap].to(dtype), V0[b, :, (P + t) % cap].to(dtype)
            Kb, Vb = torch.cat([K0[b].to(dtype), k_row[b]], 1), torch.cat([V0[b].to(dtype), v_row[b]], 1)
            n_app = T if c.lengths is None else min(T, max(0, c.lengths[b] + (1 if defect == "ragged_row_appended" else 0)))
            for t in range(n_app):
                K_after[b, :, (P + t) % cap] = round_to_ring(k_row[b, :, t], c).float()
                V_after[b, :, (P + t) % cap] = round_to_ring(v_row[b, :, t], c).float()
                written[b, t] = True
        qrot[b] = q_rot
        KH, VH = Kb[kvmap], Vb[kvmap]                                          # [H, cap (+ T), D]
        for t in range(T):
            rows = _entries(c, P, t, qs[t], defect)
            if not rows:
                continue
            idx = torch.tensor([r[1] if r[0] == "ring" else cap + r[1] for r in rows])
            qv = q_rot[:, t]
            if planes:
                qv = _planes(qv, lo=defect != "q_lo_dropped").to(dtype)
            sc = torch.einsum("hd,hnd->hn", qv, KH[:, idx]) / math.sqrt(D)
            Vv = VH[:, idx]
            M = sc.max(-1, keepdim=True).values
            p = torch.softmax(sc, -1)
            if defect == "max_not_subtracted":
                e = torch.exp(sc.float())
                o = (torch.einsum("hn,hnd->hd", e, Vv.float()) / e.sum(-1, keepdim=True)).to(dtype)
            elif defect == "no_rescale":          # weights as they were when added, the accumulator never scaled down to the later maximum
                m_run = torch.cummax(sc, -1).values
                w = torch.exp(sc - m_run)
                o = torch.einsum("hn,hnd->hd", w, Vv) / (w * torch.exp(m_run - M)).sum(-1, keepdim=True)
            elif defect == "combine_unscaled":
                grp = torch.tensor(_groups(c, P, t, rows))
                num, l = torch.zeros(H, D, dtype=dtype), torch.zeros(H, 1, dtype=dtype)
                for gidx in grp.unique():
                    sel = grp == gidx
                    w = torch.exp(sc[:, sel] - sc[:, sel].max(-1, keepdim=True).values)
                    num += torch.einsum("hn,hnd->hd", w, Vv[:, sel])
                    l += w.sum(-1, keepdim=True)
                o = num / l
            elif planes:
                e = torch.exp(sc - M)
                o = torch.einsum("hn,hnd->hd", _planes(e, lo=defect != "p_lo_dropped").to(dtype), Vv) / e.sum(-1, keepdim=True)
            else:
                o = torch.einsum("hn,hnd->hd", p, Vv)
            out[b, t] = o
            den[b, t] = torch.einsum("hn,hnd->hd", p, Vv.abs())
            scores[b, t] = (sc, rows, torch.einsum("hd,hnd->hn", qv.abs(), KH[:, idx].abs()).max() / math.sqrt(D))
    return SimpleNamespace(out=out, den=den, k_new=k_new, v_new=v_new, k_row=k_row, v_row=v_row, K_after=K_after, V_after=V_after,
                           written=written, scores=scores, qrot=qrot)


# ---- acceptance ---------------------------------------------------------------------------------------------------------------------------
def out_ratio(got_out, ref64, case):
    """max over the live (stream, query, head) vectors and their elements of |got - ref64| / sum_j p_j |v_j|; nan where `got` is not
    finite (rows at or past a ragged length included: those only have to be finite)."""
    got = got_out.detach().cpu().double()
    if not bool(torch.isfinite(got).all()):
        return float("nan")
    worst = 0.0
    for b in range(case.B):
        for t in live_queries(case, b):
            if (b, t) in ref64.scores:
                worst = max(worst, float(((got[b, t] - ref64.out[b, t]).abs() / ref64.den[b, t].clamp_min(1e-300)).max()))
            else:
                worst = max(worst, float(got[b, t].abs().max()))
    return worst


def t_op(case, ref64):
    """The operand term of the kernel's own schedule (module docstring)."""
    t = 0.0
    if case.entry == "prefill" and case.kv == "bf16":
        e = max((float(s[2]) for (b, tq), s in ref64.scores.items() if tq in live_queries(case, b)), default=0.0)
        t = 2 * 2.0 ** -16 * e + 2.0 ** -16
    if case.packed:
        t += 2.0 ** -16
    return t


def tolerance(r32, top):
    return min(max(TOL_FACTOR * r32, top, TOL_FLOOR), TOL_CEIL)


def ring_ratio(got_K, got_V, ref64, before, case, pos):
    """The rings after the launch: inf unless every slot the launch does not append is bit-identical to `before`; else the worst
    written row against the reference's unrounded key / value: (|row - new| - half a bf16 ulp on bf16 rings) / max |new|."""
    c = case
    if c.entry == "qpre":
        return 0.0 if torch.equal(got_K, before[0]) and torch.equal(got_V, before[1]) else float("inf")
    keep = torch.ones(c.B, c.cap, dtype=torch.bool)
    for b in range(c.B):
        for t in range(c.T):
            if ref64.written[b, t]:
                keep[b, (pos[b] + t) % c.cap] = False
    mask = keep.view(c.B, 1, c.cap, 1).expand_as(got_K)
    if not (torch.equal(got_K[mask], before[0][mask]) and torch.equal(got_V[mask], before[1][mask])):
        return float("inf")
    worst = 0.0
    for b in range(c.B):
        for t in range(c.T):
            if not ref64.written[b, t]:
                continue
            s = (pos[b] + t) % c.cap
            for row, new in ((got_K[b, :, s], ref64.k_new[b, :, t]), (got_V[b, :, s], ref64.v_new[b, :, t])):
                row, new = row.double(), new.double()
                if not bool(torch.isfinite(row).all()):
                    return float("nan")
                slack = half_ulp_bf16(new) if c.kv == "bf16" else torch.zeros_like(new)
                r = ((row - new).abs() - slack).amax(-1) / new.abs().amax(-1).clamp_min(1e-300)
                worst = max(worst, float(r.max()))
    return worst


def accept(got, ref64, tol, built):
    """(within the bound, what was worst, its ratio): `got` has `out` ``[B, T, H, D]`` and the rings after the launch `K_after`, `V_after`."""
    c = built.case
    ro = out_ratio(got.out, ref64, c)
    rr = ring_ratio(got.K_after, got.V_after, ref64, (built.K, built.V), c, built.pos)
    name, r = ("out", ro) if (ro != ro or (rr == rr and ro >= rr)) else ("ring", rr)
    return bool(ro <= tol and rr <= tol), name, r


def measure(built, got_out=None, own=None):
    """The fp64 and fp32 runs of the reference on `built` (attending to ``own`` if given), r32, t_op and the tolerance."""
    c = built.case
    ref64 = reference(c, (built.K, built.V), built.qkv, built.pos, torch.float64, own=own)
    ref32 = reference(c, (built.K, built.V), built.qkv, built.pos, torch.float32, own=own)
    r32 = out_ratio(ref32.out, ref64, c)
    top = t_op(c, ref64)
    return SimpleNamespace(ref64=ref64, ref32=ref32, r32=r32, t_op=top, tol=tolerance(r32, top))


# ---- device side --------------------------------------------------------------------------------------------------------------------------
def _guarded(t, dev, dtype):
    """`t` on the device followed by a run of NaN: bytes no launch may load."""
    flat = torch.full((t.numel() + 4096,), float("nan"), device=dev, dtype=dtype)
    flat[:t.numel()] = t.reshape(-1).to(dev, dtype)
    return flat[:t.numel()].view(t.shape)


def device_run(built, dev, route="entry"):
    """One launch of the case's public entry point on freshly uploaded rings (``route="steps"``: a prefill chunk as Tc single
    ops.lm_attn_decode steps instead).  Returns `out` ``[B, T, H, D]``, the rings after it as fp32 CPU tensors and `own`, the rows the
    launch wrote for its new positions ``[B, G, T, D]`` (prefill: by an un-ragged append on a second ring copy, so rows past a ragged
    length are there as well)."""
    from rstnet_amd import ops
    from tests.helpers.lm_operands import decode_packed
    c = built.case
    B, H, G, D, cap, T = c.B, c.H, c.G, c.D, c.cap, c.T
    dt = ring_dtype(c)
    kc, vc = _guarded(built.K, dev, dt), _guarded(built.V, dev, dt)
    qkv = _guarded(built.qkv, dev, torch.float32)
    shared = len(set(built.pos)) == 1 and not isinstance(built.position, tuple)
    pos_dev = torch.tensor(built.pos[:1] if shared else built.pos, dtype=torch.int64, device=dev)
    heads = H if G != H else None
    rope = c.rope != "off"
    own = None

    def rows_of(k, v):
        sl = torch.tensor([[(built.pos[b] + t) % cap for t in range(T)] for b in range(B)], device=dev)
        ix = sl.view(B, 1, T, 1).expand(B, G, T, D)
        return k.gather(2, ix).float().cpu(), v.gather(2, ix).float().cpu()

    def decode(q, k, v, p):
        table = ops.lm_rope_table(p, D, rope_dims=c.rope_dims) if c.rope == "table" else None
        o = ops.lm_attn_decode(q, k, v, p, rope=rope, context=c.context, heads=heads, rope_dims=c.rope_dims, packed=c.packed, rope_table=table)
        if c.packed:
            assert isinstance(o, ops.PackedAct)
            hi, lo = o.xp.view(2, -1)[0], o.xp.view(2, -1)[1]
            o = (decode_packed(hi, H * D).float() + decode_packed(lo, H * D).float())[:B]
        return o
    if c.entry == "decode":
        out = decode(qkv[:, 0], kc, vc, pos_dev).view(B, 1, H, D)
        own = rows_of(kc, vc)
    elif c.entry == "gemv":
        E = H * D
        w = built.w.to(dev) if getattr(built, "w", None) is not None else torch.eye(E, device=dev, dtype=torch.bfloat16)
        out = ops.gemv_attn(qkv[:, 0], kc, vc, pos_dev, w, context=c.context, res=torch.zeros(B, w.shape[0], device=dev)).view(B, 1, H, D)
        own = rows_of(kc, vc)
    elif c.entry == "qpre":
        out = ops.attention(qkv, kc, vc, pos_dev=pos_dev, ring=True, context=c.context).view(B, T, H, D)
    elif route == "steps":
        p = pos_dev.clone()
        outs = []
        for t in range(T):
            outs.append(decode(qkv[:, t].contiguous(), kc, vc, p))
            p.add_(1)
        out = torch.stack(outs, 1).view(B, T, H, D)
        own = rows_of(kc, vc)
    else:
        k2, v2 = kc.clone(), vc.clone()
        ops.lm_ring_append(qkv, k2, v2, pos_dev, rope=rope, max_period=MAX_PERIOD, heads=heads)
        own = rows_of(k2, v2)
        before = (kc.clone(), vc.clone())
        out = ops.lm_attn_prefill(qkv, kc, vc, pos_dev, window=c.context, rope=rope, max_period=MAX_PERIOD, heads=heads).view(B, T, H, D)
        assert torch.equal(kc, before[0]) and torch.equal(vc, before[1]), "the attention launch must not touch the ring"
        if c.lengths is None:
            ops.lm_ring_append(qkv, kc, vc, pos_dev, rope=rope, max_period=MAX_PERIOD, heads=heads)
        else:
            ops.lm_ring_append_ragged(qkv, kc, vc, pos_dev, rope=rope, max_period=MAX_PERIOD, heads=heads,
                                      lengths=torch.tensor(c.lengths, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    return SimpleNamespace(out=out.float().cpu(), K_after=kc.float().cpu(), V_after=vc.float().cpu()), own
