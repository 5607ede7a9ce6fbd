"""The persistent temporal-frame launch (csrc/lm_temporal.hip behind ops.temporal_decode_frame) restated for its step-by-step tests:
the case table with the positions / contexts each case is run at, CPU operands and poisoned rings, a reference of ONE step of all
layers in any dtype (fp64 for the bound, fp32 for the tolerance) that takes the ring as an input and can carry one named defect, the
launcher's grid and loop bounds (`grid`), the readout of the hand-off workspace and the acceptance function.  Nothing here needs a GPU
until `device_case` is called; tests/test_temporal_frame_steps_cpu.py checks the table's coverage, the ring map against a brute-force
write history and RingKV.complete, the reference against oracle/lm_oracle.py and that every defect is rejected.

Why the ring is an input: the launch reads cap - 1 old rows per head and writes one, so a test that chooses `pos`, `context` and the
ring contents freely reaches every split / block / wrap geometry in one launch each.  Every slot the step must NOT see -- its own
stale row included -- holds K = 0, V = +-2^14: score 0 gives a wrongly admitted slot a softmax weight of at least
exp(-max visible score) / n_visible, an error of order 10^3 instead of one that shows by luck.

Why prefixes: the hand-off workspace keeps the last layer's vectors; a launch over the first l layers (same weights, same rings --
re-appending the step's row is idempotent) ends in layer l's residual stream."""
import math
from collections import namedtuple
from types import SimpleNamespace

import torch

from tests.helpers.depth_frame_ref import TOL_CEIL, TOL_FACTOR, TOL_FLOOR, ratio, worst

TF_WW, TF_MAX_SPLITS, TF_TAB_MAX, TF_HDR, TF_MAX_L = 4, 8, 48, 64, 40          # csrc/lm_temporal.hip
K_PIECE, K_BLOCK = 512, 4096                                                   # k per 16-byte piece of a wave, k per block of 8 pieces
LDS_LIMIT = 150 * 1024
EPS = 1e-5
POISON = 2.0 ** 14

# ---- the case table -----------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name E H Hd cap kv L")          # kv: "f32" | "bf16" rings
Step = namedtuple("Step", "pos context rope")

CASES = (
    # G 64, S 8, U 64: past 512 slots per > 64 and some waves walk two ring blocks; the rescale across blocks and across 8 splits
    Case("d128-f32", 256, 2, 264, 530, "f32", 2),
    # U 256: two ring blocks per wave past 2048 slots
    Case("d64-bf16", 256, 4, 264, 2100, "bf16", 2),
    # the fourth kernel variant; one and two splits
    Case("d64-f32", 256, 4, 264, 140, "f32", 2),
    # the third kernel variant
    Case("d128-bf16", 256, 2, 264, 140, "bf16", 2),
    # 55 - 57 blocks per layer and wave > TF_TAB_MAX: the persistent launch decodes as it goes; four k blocks for the FFN out, the last
    # with 8 live columns; 106 KB of LDS
    Case("tab-off", 256, 4, 12296, 70, "f32", 2),
    # E = 2 x 512 + 64: a clamped third piece; 4 or 3 in-projection rows and 2 or 1 out rows per wave; an odd head count
    Case("e1088", 1088, 17, 520, 70, "bf16", 2),
    # every wave owns two out-projection rows; gate rows 2 or 1 per wave
    Case("rows", 2048, 16, 1032, 70, "f32", 2),
    # S = 6; workgroups 240 - 255 serve no head; two splits past 256 slots
    Case("s6", 2560, 40, 264, 300, "bf16", 2),
    # Hd = 7 x 512 + 264: eight pieces, the eighth partial -- not the whole block whose loads go unclamped (the last row's would run past
    # the matrix, into the NaN row `device_case` puts behind every weight matrix)
    Case("hd3848", 256, 4, 3848, 70, "f32", 2),
)
BY_NAME = {c.name: c for c in CASES}
RING_CASES = ("d128-f32", "d64-bf16", "d64-f32", "d128-bf16")
SHAPE_CASES = ("tab-off", "e1088", "rows", "s6", "hd3848")
CONTEXT_CASES = ("d128-f32", "d64-bf16")
STREAM_CASES = ("d64-f32", "d128-bf16")
STREAM_STEPS = 6          # from pos = cap - 3: across end % cap == 0 and the first wrap

FLAGS = ("f32_d128", "bf16_d64", "f32_d64", "bf16_d128", "tab_off", "kv_blocks_2", "splits_1", "splits_2", "splits_8", "S_lt_8",
         "wg_without_head", "wave_without_slot", "E_tail", "Hd_tail", "Hd_k_blocks", "rows_pair_ragged", "rows2_out",
         "ctx_split_invisible", "ctx_1", "ctx_over_wrap", "wrap_end0", "no_rope", "k_block_partial8")


def kv_geometry(case):
    """TfKv: slots per block of one wave (SPB) and per block round of a workgroup (U = 4 SPB)."""
    D = case.E // case.H
    row_bytes = D * (2 if case.kv == "bf16" else 4)
    SPB = 8 * (64 // (row_bytes // 16))
    return SimpleNamespace(D=D, SPB=SPB, U=TF_WW * SPB)


def positions(case):
    """The positions a ring-geometry case is run at with no context and the product's rope table."""
    g, cap = kv_geometry(case), case.cap
    ps = [0, g.SPB - 1, g.SPB, g.U - 1, g.U]
    if 8 * g.U < cap:
        ps += [8 * g.U - 1, 8 * g.U]
    ps += [cap - 2, cap - 1, cap, cap + 1, 2 * cap - 1, 2 * cap + 3]
    return ps


def context_steps(case):
    """An unwrapped ring (all eight splits walk) and a wrapped one under every kind of context, plus a window that straddles the wrap."""
    g, cap = kv_geometry(case), case.cap
    out = []
    for pos in (8 * g.U + 5, cap + 7):
        out += [Step(pos, ctx, True) for ctx in (1, 5, g.U + 3, cap - 1, cap, cap + 50)]
    return out + [Step(cap + 2, 9, True)]


def steps(case):
    """Every (pos, context, rope) of the position test of a case."""
    cap = case.cap
    if case.name in RING_CASES:
        out = [Step(p, None, True) for p in positions(case)]
        if case.name in CONTEXT_CASES:
            out += context_steps(case)
    else:          # an empty ring, a half-full ring, a wrapped ring
        out = [Step(0, None, True), Step(cap // 2, None, True), Step(cap + 5, None, True)]
    return out + [Step(cap // 2 + 1, None, False)]


def repair_steps():
    """(case, step) of the repair-launch test."""
    a, u = BY_NAME["d128-f32"], kv_geometry(BY_NAME["d128-f32"]).U
    return [("d128-f32", Step(8 * u, None, True)), ("d128-f32", Step(a.cap, None, True)), ("d64-f32", Step(BY_NAME["d64-f32"].cap + 1, None, True)),
            ("e1088", Step(40, None, True)), ("tab-off", Step(75, 5, True))]


# ---- the ring map --------------------------------------------------------------------------------------------------------------------------
def slot_position(slot, pos, cap):
    """The position ring slot `slot` counts as right after the append of position `pos` (end = pos + 1 steps made), None when it is
    unwritten: the latest p <= pos with p = slot (mod cap) -- except that the slot the NEXT append will take, end % cap, counts as
    position `end` (RingKVCache.complete's `delta <= 0` branch at delta = 0), which lies in the future."""
    end = pos + 1
    if slot >= end or slot >= cap:
        return None
    if slot == end % cap:
        return end
    return pos - (pos - slot) % cap


def visible(slot, pos, cap, context):
    p = slot_position(slot, pos, cap)
    return p is not None and 0 <= pos - p and (not context or pos - p < context)


def visible_slots(pos, cap, context):
    return [s for s in range(cap) if visible(s, pos, cap, context)]


# ---- the launcher's geometry --------------------------------------------------------------------------------------------------------------
def lds_bytes(case):
    """tf_lds_bytes."""
    D = case.E // case.H
    EP, HdP = -(-case.E // K_BLOCK) * K_BLOCK, -(-case.Hd // K_BLOCK) * K_BLOCK
    return (TF_HDR + 2 * EP + HdP + 2 * case.E + 3 * D + TF_WW * D + TF_WW * TF_TAB_MAX * 8) * 4


def split_of(geo, slot):
    """(split, block round, wave) that walks `slot` of a head's ring in the persistent launch."""
    split = slot // geo.per
    off = slot - split * geo.per
    return split, off // geo.U, (off // geo.SPB) % TF_WW


def grid(case, cus, step=None):
    """rst_temporal_frame_grid, tf_lds_bytes and the loop bounds of temporal_frame_kernel: G, W = 4 G, splits per head S, whether the
    launcher serves the shape (`ok`) and the set of paths taken (`flags`) -- those of the shape alone, or with `step` also those of
    the ring geometry at that (pos, context): active splits, slots per split `per`, ring blocks per wave, blocks per layer and wave."""
    c = case
    E, H, Hd, cap = c.E, c.H, c.Hd, c.cap
    D = E // H
    kg = kv_geometry(c)
    ok = E > 0 and E % 8 == 0 and E <= 4096 and Hd > 0 and Hd % 8 == 0 and H > 0 and D in (64, 128) and H * D == E and 1 <= c.L <= TF_MAX_L and cap >= 1
    lds = lds_bytes(c)
    G = min(cus, E // TF_WW)
    ok = bool(ok and lds <= LDS_LIMIT and G >= 1 and H <= G)
    W = G * TF_WW
    S = min(TF_MAX_SPLITS, G // H) if ok else 0
    f = {f"{c.kv}_d{D}"}
    if S < TF_MAX_SPLITS:
        f.add("S_lt_8")
    if G > H * S:
        f.add("wg_without_head")
    if E > K_PIECE and E % K_PIECE:
        f.add("E_tail")
    if Hd > K_BLOCK:
        f.add("Hd_k_blocks")
        if Hd % K_BLOCK:
            f.add("Hd_tail")
    if any(K % K_BLOCK > K_BLOCK - K_PIECE for K in (E, Hd)):          # eight pieces, but not a whole block
        f.add("k_block_partial8")
    if any(N > W and N % W for N in (3 * E, E)):
        f.add("rows_pair_ragged")
    if E > W:
        f.add("rows2_out")
    out = SimpleNamespace(G=G, W=W, S=S, lds=lds, ok=ok, D=D, SPB=kg.SPB, U=kg.U)
    if step is not None and ok:
        pos, ctx = step.pos, step.context
        n_used = min(cap, pos + 1)
        active = max(1, min(S, -(-n_used // kg.U)))
        per = -(-n_used // active)
        out.n_used, out.active, out.per = n_used, active, per
        KBd = -(-Hd // K_BLOCK)

        def rows_of(N, gw):
            return -(-(N - gw) // W) if gw < N else 0
        kvb = {}
        for split in range(S):
            for w in range(TF_WW):
                s_lo = split * per
                span = min(n_used, s_lo + per) - s_lo - w * kg.SPB
                kvb[split, w] = -(-span // kg.U) if split < active and span > 0 else 0
        n_layer = []
        for gw in range(W):
            wg, w = divmod(gw, TF_WW)
            nB = (rows_of(E, gw) + 1) // 2
            kv = kvb[wg % S, w] if wg // S < H else 0
            n_layer.append((rows_of(3 * E, gw) + 1) // 2 + kv + nB + rows_of(Hd, gw) + nB * KBd)
        out.blocks_per_layer = (min(n_layer), max(n_layer))
        if min(n_layer) > TF_TAB_MAX:
            f.add("tab_off")
        if max(kvb.values()) >= 2:
            f.add("kv_blocks_2")
        if active in (1, 2, 8):
            f.add(f"splits_{active}")
        if any(kvb[s, w] == 0 for s in range(active) for w in range(TF_WW)):
            f.add("wave_without_slot")
        vis = visible_slots(pos, cap, ctx)
        if ctx:
            if active > 1 and {s // per for s in vis} != set(range(active)):
                f.add("ctx_split_invisible")
            if ctx == 1:
                f.add("ctx_1")
            if ctx < cap - 1 and vis and min(vis) == 0 and max(vis) == cap - 1:
                f.add("ctx_over_wrap")
        if (pos + 1) % cap == 0:
            f.add("wrap_end0")
        if not step.rope:
            f.add("no_rope")
    out.flags = frozenset(f)
    return out


def case_flags(case, cus):
    """Every path the position test of `case` takes on a device of `cus` CUs."""
    f = set()
    for st in steps(case):
        f |= grid(case, cus, st).flags
    return frozenset(f)


# ---- operands ------------------------------------------------------------------------------------------------------------------------------
def _seed(name, seed):
    s = seed
    for ch in name:
        s = (s * 1000003 + ord(ch)) % (1 << 62)
    return s


def ring_dtype(case):
    return torch.bfloat16 if case.kv == "bf16" else torch.float32


def make_case(case, seed=0):
    """CPU operands: bf16 weights of randn / sqrt(K), fp32 norm gains and input, and per layer the ring's base contents (0.5 randn at
    the ring's precision, kept as fp32) with the signs of its poison."""
    c = case
    g = torch.Generator().manual_seed(_seed(c.name, seed))
    E, Hd, H, D = c.E, c.Hd, c.H, c.E // c.H

    def w(rows, cols):
        return (torch.randn(rows, cols, generator=g) / math.sqrt(cols)).bfloat16()
    o = SimpleNamespace(case=c, eps=float(torch.tensor(EPS, dtype=torch.float32)))
    o.in_proj = [w(3 * E, E) for _ in range(c.L)]
    o.out_proj = [w(E, E) for _ in range(c.L)]
    o.gate_in = [w(2 * Hd, E) for _ in range(c.L)]
    o.gate_out = [w(E, Hd) for _ in range(c.L)]
    o.norm1 = [1 + 0.1 * torch.randn(E, generator=g) for _ in range(c.L)]
    o.norm2 = [1 + 0.1 * torch.randn(E, generator=g) for _ in range(c.L)]
    o.x = torch.randn(E, generator=g)
    o.ring_base = [tuple((0.5 * torch.randn(H, c.cap, D, generator=g)).to(ring_dtype(c)).float() for _ in range(2)) for _ in range(c.L)]
    o.poison_sign = [torch.where(torch.rand(H, c.cap, D, generator=g) < 0.5, -1.0, 1.0) for _ in range(c.L)]
    return o


def make_rings(co, step):
    """Per layer (K, V) fp32 ``[H, cap, D]`` before the step: the base contents where the step sees them, K = 0 and V = +-2^14 in every
    other slot, the step's own slot included."""
    return poison(co, [(K.clone(), V.clone()) for K, V in co.ring_base], step)


def poison(co, rings, step):
    """K = 0, V = +-2^14 (in place) in every slot of `rings` that the step must not see."""
    c = co.case
    hidden = torch.tensor([not visible(s, step.pos, c.cap, step.context) or s == step.pos % c.cap for s in range(c.cap)])
    for l, (K, V) in enumerate(rings):
        K[:, hidden] = 0.0
        V[:, hidden] = (POISON * co.poison_sign[l])[:, hidden]
    return rings


def rope_table(pos, D, max_period=10000.0):
    """``[D/2, 2]`` (cos, sin) of one step in fp32, the arithmetic of the oracle's rope_interleaved_1 (for the tests without a GPU; the
    GPU tests hand the reference the table the product built)."""
    ds = torch.arange(D // 2, dtype=torch.float32)
    ang = torch.exp(ds * (-math.log(max_period) * 2 / D)) * torch.tensor([pos]).float()
    return torch.stack([torch.cos(ang), torch.sin(ang)], -1)


# ---- the reference ------------------------------------------------------------------------------------------------------------------------
# xs [L, E]: every layer's output | qkv [3E], att [E], hid [Hd]: the last layer's hand-off vectors (qkv before the rotation) |
# k_new, v_new [L, H, D]: the step's key (rotated) and value before they are rounded to the ring | k_row, v_row [L, H, D]: the row of
# the step's slot as attended to and written | gx [E]: the last layer's output as the hand-off workspace holds it (launches only)
Ref = namedtuple("Ref", "xs qkv att hid k_new v_new k_row v_row gx", defaults=(None,))
DEFECTS = ("ctx_ignored", "oldest_slot_visible", "own_slot_stale", "own_kv_unrounded", "k_unrotated", "last_slot_dropped",
           "last_split_dropped", "second_kv_block_dropped", "wave1_slots_dropped", "merge_unscaled", "rotate_half_instead_of_pairs",
           "k_tail_E", "k_tail_Hd", "second_row_dropped", "norm2_on_layer_input")


def round_to_ring(t, case):
    return t.float().to(ring_dtype(case)).to(t.dtype)


def reference(co, step, rings, table, own=None, dtype=torch.float64, defect=None, x=None):
    """One step at ``step.pos`` through all layers in ``dtype``.  ``rings``: per layer (K, V) ``[H, cap, D]`` before the step;
    ``table``: ``[D/2, 2]`` (cos, sin) or None; ``own``: per layer (k, v) ``[H, D]`` the row a launch wrote for the step's slot --
    teacher forcing, the reference then attends to exactly that row -- or None: its own key / value rounded to the ring's precision."""
    c = co.case
    E, H, Hd, L, cap = c.E, c.H, c.Hd, c.L, c.cap
    D = E // H
    pos, context = step.pos, step.context
    eps = torch.tensor(co.eps, dtype=torch.float32).to(dtype)
    geo = grid(c, 256, step)
    W = geo.W
    kE = (E // K_PIECE) * K_PIECE if defect == "k_tail_E" and E > K_PIECE else E
    kH = (Hd // K_BLOCK) * K_BLOCK if defect == "k_tail_Hd" and Hd > K_BLOCK else Hd
    slot_cur = pos % cap
    vis = visible_slots(pos, cap, None if defect == "ctx_ignored" else context)
    if defect == "oldest_slot_visible" and pos + 1 >= cap and (not context or cap - 1 < context) and (pos + 1) % cap not in vis:
        vis = sorted(vis + [(pos + 1) % cap])          # the write history says it holds position pos + 1 - cap
    if defect == "last_slot_dropped":
        vis = vis[:-1]
    if defect == "last_split_dropped" and geo.active > 1:
        vis = [s for s in vis if split_of(geo, s)[0] != geo.active - 1]
    if defect == "second_kv_block_dropped":
        vis = [s for s in vis if split_of(geo, s)[1] == 0]
    if defect == "wave1_slots_dropped":
        vis = [s for s in vis if split_of(geo, s)[2] != 1]
    idx = torch.tensor(vis, dtype=torch.long)

    def lin(v, wt, K, pairs):
        y = wt[:, :K].to(dtype) @ v[:K]
        if defect == "second_row_dropped" and pairs:          # row r0 + W of a block of two rows
            y[(torch.arange(y.numel()) // W) % 2 == 1] = 0
        return y

    def norm(v, alpha):
        return v * (alpha.to(dtype) / torch.sqrt(eps + (v * v).mean()))

    def rotate(v):          # [H, D]
        if table is None:
            return v
        cs, sn = table[:, 0].to(dtype), table[:, 1].to(dtype)
        if defect == "rotate_half_instead_of_pairs":
            a, b = v[:, :D // 2], v[:, D // 2:]
            return torch.cat([a * cs - b * sn, a * sn + b * cs], -1)
        a, b = v[:, 0::2], v[:, 1::2]
        return torch.stack([a * cs - b * sn, a * sn + b * cs], -1).reshape(H, D)

    def attend(q, K, V):
        if not vis:
            return torch.zeros(H, D, dtype=dtype)
        sc = torch.einsum("hd,hsd->hs", q, K[:, idx]) / math.sqrt(D)
        if defect != "merge_unscaled":
            return torch.einsum("hs,hsd->hd", torch.softmax(sc, -1), V[:, idx])
        num, den = torch.zeros(H, D, dtype=dtype), torch.zeros(H, 1, dtype=dtype)
        for split in sorted({split_of(geo, s)[0] for s in vis}):          # partials added without exp(m_s - M)
            sel = torch.tensor([i for i, s in enumerate(vis) if split_of(geo, s)[0] == split])
            p = torch.exp(sc[:, sel] - sc[:, sel].max(-1, keepdim=True).values)
            num += torch.einsum("hs,hsd->hd", p, V[:, idx[sel]])
            den += p.sum(-1, keepdim=True)
        return num / den
    x = (co.x if x is None else x).to(dtype)
    xs, k_new, v_new, k_row, v_row = [], [], [], [], []
    for l in range(L):
        qkv = lin(norm(x, co.norm1[l]), co.in_proj[l], kE, True)
        q, k, v = qkv.view(3, H, D).unbind(0)
        q = rotate(q)
        if defect != "k_unrotated":
            k = rotate(k)
        if own is not None:
            kr, vr = own[l][0].to(dtype), own[l][1].to(dtype)
        else:
            kr, vr = round_to_ring(k, c), round_to_ring(v, c)
        K, V = rings[l][0].to(dtype).clone(), rings[l][1].to(dtype).clone()
        if defect != "own_slot_stale":
            K[:, slot_cur], V[:, slot_cur] = (k, v) if defect == "own_kv_unrounded" else (kr, vr)
        att = attend(q, K, V).reshape(E)
        x1 = x + lin(att, co.out_proj[l], kE, True)
        uv = lin(norm(x if defect == "norm2_on_layer_input" else x1, co.norm2[l]), co.gate_in[l], kE, False)
        hid = torch.nn.functional.silu(uv[:Hd]) * uv[Hd:]
        x = x1 + lin(hid, co.gate_out[l], kH, True)
        xs.append(x)
        k_new.append(k), v_new.append(v), k_row.append(kr), v_row.append(vr)
    return Ref(torch.stack(xs), qkv, att, hid, torch.stack(k_new), torch.stack(v_new), torch.stack(k_row), torch.stack(v_row))


def rows_of(ref):
    """The rows a run wrote, in the form `reference(own=...)` takes."""
    return [(ref.k_row[l], ref.v_row[l]) for l in range(ref.k_row.shape[0])]


def append(rings, step, ref, case):
    """The rings after the step: the row of `ref` in slot pos % cap of every layer (streaming on the CPU)."""
    for l, (K, V) in enumerate(rings):
        K[:, step.pos % case.cap], V[:, step.pos % case.cap] = ref.k_row[l].float(), ref.v_row[l].float()
    return rings


# ---- acceptance ---------------------------------------------------------------------------------------------------------------------------
def half_ulp_bf16(a):
    """Half a bf16 unit in the last place of |a| (0 at 0), as fp64."""
    a = a.double().abs()
    _, ex = torch.frexp(a)          # a = m 2^ex, m in [0.5, 1): an ulp of 8 significand bits is 2^(ex - 8)
    return torch.where(a > 0, torch.ldexp(torch.ones_like(a), ex.clamp_min(-125) - 9), torch.zeros_like(a))


def row_ratio(row, new, case):
    """A written head row ``[D]`` against the reference's unrounded key / value: max over the elements of (|row - new| - r) /
    max |new|, r = half a bf16 ulp of |new| on bf16 rings and 0 on fp32 rings -- held to the same `tol` as every vector."""
    row, new = row.detach().cpu().double(), new.detach().cpu().double()
    if not bool(torch.isfinite(row).all()):
        return float("nan")
    slack = half_ulp_bf16(new) if case.kv == "bf16" else torch.zeros_like(new)
    return float((((row - new).abs() - slack).max() / new.abs().max().clamp_min(1e-300)).clamp_min(0.0))


def ratios(got, ref, case, rows=True):
    """The ratio (max |got - ref| / max |ref|) of every vector the tests bound: every layer's output, the last layer's qkv / gated
    activation / x hand-offs where `got` has them, the attention output per head, and (``rows``) the written row per layer and head."""
    H, D = case.H, case.E // case.H
    out = {f"x[layer {l}]": ratio(got.xs[l], ref.xs[l]) for l in range(ref.xs.shape[0])}
    if got.qkv is not None:
        out["qkv"] = ratio(got.qkv, ref.qkv)
    if got.hid is not None:
        out["hid"] = ratio(got.hid, ref.hid)
    if got.gx is not None:
        out["x[hand-off]"] = ratio(got.gx, ref.xs[-1])
    if got.att is not None:
        ga, ra = got.att.reshape(H, D), ref.att.reshape(H, D)
        for h in range(H):
            out[f"att[head {h}]"] = ratio(ga[h], ra[h]) if float(ra[h].abs().max()) > 0 else float(ga[h].abs().max())
    if rows:
        for l in range(ref.k_new.shape[0]):
            for h in range(H):
                out[f"k_row[layer {l}, head {h}]"] = row_ratio(got.k_row[l, h], ref.k_new[l, h], case)
                out[f"v_row[layer {l}, head {h}]"] = row_ratio(got.v_row[l, h], ref.v_new[l, h], case)
    return out


def tolerance(ref32, ref64, case):
    """depth_frame_ref.tolerance's rule: 16 x the worst ratio of the fp32 run of the reference against its fp64 run (both attending
    to the same written row), within [2^-18, 1e-3]."""
    return min(max(TOL_FACTOR * worst(ratios(ref32, ref64, case, rows=False))[1], TOL_FLOOR), TOL_CEIL)


def accept(got, ref64, tol, case):
    """(every vector and written row within tol, name of the worst, its ratio)."""
    rs = ratios(got, ref64, case)
    name, r = worst(rs)
    return all(v <= tol for v in rs.values()), name, r


# ---- the hand-off workspace ---------------------------------------------------------------------------------------------------------------
def workspace(ops, case):
    """The eager workspace ops.temporal_decode_frame launched a shape on (int64 granules)."""
    return ops.frame_workspace("temporal_frame", (case.E, case.Hd, case.H))


def read_handoff(ws, case, solo=False):
    """The fp32 value (low word) and the epoch tag (high word) of every {tag, value} granule of gX [E] | gQKV [3E] | gATT [E] | gH [Hd]
    (csrc/lm_temporal.hip: rst_temporal_frame_workspace_granules) as CPU tensors X, QKV, ATT, H and X_tag, ...  ``solo``: the repair
    launch's own set, one such set (the head partials included) further on."""
    E, Hd, H, D = case.E, case.Hd, case.H, case.E // case.H
    n = 5 * E + Hd + H * TF_MAX_SPLITS * (D + 2)
    words = ws[n if solo else 0:2 * n if solo else n].view(torch.int32).view(-1, 2).cpu()
    out, off = {}, 0
    for name, width in (("X", E), ("QKV", 3 * E), ("ATT", E), ("H", Hd)):
        out[name] = words[off:off + width, 0].contiguous().view(torch.float32)
        out[name + "_tag"] = words[off:off + width, 1].contiguous()
        off += width
    return SimpleNamespace(**out)


# ---- device side --------------------------------------------------------------------------------------------------------------------------
def device_case(co, dev):
    """The operands on the device, rings of the case's capacity and precision, and ``ops.TemporalFrameTables`` over the first
    1 .. L layers (``tables[l - 1]``: l layers; they share the weight and ring tensors).  Every weight matrix is followed by one row of
    NaN and every ring by one head of NaN: a load past the last row / head that is multiplied by a padding zero or a zero softmax
    weight still turns its sum into NaN, which no bound accepts."""
    from rstnet_amd import ops
    c = co.case
    D = c.E // c.H

    def guarded(w):
        buf = torch.full((w.shape[0] + 1, w.shape[1]), float("nan"), device=dev, dtype=w.dtype)
        buf[:-1] = w.to(dev)
        return buf[:-1]

    def ring():
        return torch.full((1, c.H + 1, c.cap, D), float("nan"), device=dev, dtype=ring_dtype(c))[:, :c.H]
    layers = []
    for l in range(c.L):
        layers.append(dict(in_proj=guarded(co.in_proj[l]), out_proj=guarded(co.out_proj[l]), gate_in=guarded(co.gate_in[l]),
                           gate_out=guarded(co.gate_out[l]), norm1=co.norm1[l].to(dev), norm2=co.norm2[l].to(dev), k_cache=ring(), v_cache=ring()))
    tables = [ops.TemporalFrameTables(layers[:l], H=c.H, context=None, eps=co.eps) for l in range(1, c.L + 1)]
    return SimpleNamespace(case=c, co=co, dev=dev, layers=layers, tables=tables, x=co.x.to(dev).view(1, c.E).contiguous())


def upload_rings(d, rings):
    for ly, (K, V) in zip(d.layers, rings):
        ly["k_cache"][0].copy_(K.to(ly["k_cache"].dtype))
        ly["v_cache"][0].copy_(V.to(ly["v_cache"].dtype))


def download_rings(d):
    return [(ly["k_cache"][0].float().cpu(), ly["v_cache"][0].float().cpu()) for ly in d.layers]


def launch(d, step, *, status_code=0):
    """One step on the rings as they are on the device: the launch over all layers, then over the first L - 1 .. 1 layers (each
    layer's output).  ``status_code``: planted in status[0] of every table first, so that the repair launch behind each persistent one
    recomputes the step (the readout is then the repair launch's granule set).  Returns (what the launches left as a `Ref` with the
    written rows, the status words of every table -- full launch last --, the tags of the read granule set, the rope table on the CPU,
    the rings after the launches)."""
    from rstnet_amd import ops
    c = d.case
    pos_dev = torch.tensor([step.pos], dtype=torch.int64, device=d.dev)
    table = ops.lm_rope_table(pos_dev, c.E // c.H) if step.rope else None
    ys, hand = [None] * c.L, None
    for t in reversed(d.tables):
        t.context = step.context
        if status_code:
            t.status[0] = status_code
        ys[t.L - 1] = ops.temporal_decode_frame(t, d.x, pos_dev, table)
        torch.cuda.synchronize()
        if t.L == c.L:
            hand = read_handoff(workspace(ops, c), c, solo=bool(status_code))
    after = download_rings(d)
    slot = step.pos % c.cap
    got = Ref(torch.stack([y[0].cpu() for y in ys]), hand.QKV, hand.ATT, hand.H, None, None,
              torch.stack([K[:, slot] for K, _ in after]), torch.stack([V[:, slot] for _, V in after]), hand.X)
    tags = {n: getattr(hand, n + "_tag") for n in ("X", "QKV", "ATT", "H")}
    return got, [t.status.tolist() for t in d.tables], tags, None if table is None else table.cpu(), after
