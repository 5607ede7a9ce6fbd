"""The persistent codec-transformer launch (csrc/codec_tr.hip behind ops.codec_transformer_frame) restated for its step-by-step tests:
the case table with the steps (pos, context, rope, T) each case is run at, CPU operands and poisoned rings, a reference of ONE step
of all layers in any dtype (fp64 for the bound, fp32 for the tolerance) that takes the rings as an input and can carry one named
defect, the launcher's grid and loop bounds (`grid`), the granule layout of the hand-off workspace and the acceptance function.
Nothing here needs a GPU until `device_case` is called; tests/test_codec_frame_steps_cpu.py checks the table's coverage, the ring map
against a brute-force write history, the reference against oracle/mimi_oracle.py and that every defect is rejected.

Why the rings are an input: a step reads up to cap old rows per (stream, head) and writes T, so a test that chooses `pos`, `context`,
T and the ring contents freely reaches every batch / wrap / window geometry in one launch each.  Every slot the step must NOT see --
masked by the context for every query, older than the ring map admits, never written, the new positions' own stale rows -- holds
K = 0, V = +-2^14: score 0 gives a wrongly admitted slot a softmax weight of at least exp(-max visible score) / n_visible, an error
of order 10^3 instead of one that hides under LayerScale.

Why prefixes: the hand-off workspace keeps the last layer's vectors; a launch over the first l layers (same weights, same rings --
re-appending the step's rows is idempotent) ends in layer l's residual stream."""
import math
from collections import namedtuple
from types import SimpleNamespace

import torch

from tests.helpers.depth_frame_ref import TOL_CEIL, TOL_FACTOR, TOL_FLOOR, ratio, worst

DF_WAVES, DF_THREADS, DF_HDR_FLOATS, MAX_L = 4, 256, 512, 8          # csrc/persist.h, RST_CTR_MAX_L
K_CHUNK, K_BLOCK2 = 512, 2048          # k per chunk of a wave (8 floats per lane); k per block of linear2 (four chunks)
LN_REG = 1024                          # columns of a row ct_layernorm keeps in registers; the rest goes through its tail loops
JB = 16                                # ring slots per slot class and batch
LDS_LIMIT = 150 * 1024
EPS = 1e-5
MAX_PERIOD = 10000.0
POISON = 2.0 ** 14

# ---- the case table -----------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name E H F L cap B scale")          # scale: LayerScale's mean value, None: no LayerScale (null ls1 / ls2)
Step = namedtuple("Step", "pos context rope T")                # context None: the ring map alone

CASES = (
    # 64 slot classes, 1024 slots per batch: a second batch past 1024 used slots; G = 16 > B H = 4: workgroups without a head
    Case("d16", 64, 4, 64, 2, 1100, 1, 0.3),
    # W = 64: 384 in-projection rows in three rounds of two, 128 out-projection rows in two rounds, linear1's second row masked
    Case("d32", 128, 4, 64, 2, 37, 1, 0.3),
    # Mimi's layer shape at four rows (two streams x two positions); 256 slots per batch
    Case("d64", 512, 8, 2048, 2, 250, 2, 0.3),
    # 128 slots per batch: two batches
    Case("d128", 512, 4, 1024, 2, 150, 1, 0.3),
    # 64 slots per batch: three batches; a whole wave per ring row
    Case("d256", 512, 2, 512, 2, 150, 2, 0.3),
    # E = 512 + 16: a second k chunk with 16 live columns (lanes 0 and 1); 33 heads
    Case("e528", 528, 33, 136, 2, 20, 1, 0.3),
    # E = 2 x 512 + 64: the LayerNorm's tail loops past 1024 columns, a third k chunk with 64 live columns; 17 heads
    Case("e1088", 1088, 17, 128, 2, 20, 1, 0.3),
    # F = 2048 + 8: linear2's second k block with 8 live columns (lane 0 of its first chunk)
    Case("f2056", 64, 4, 2056, 2, 20, 1, 0.3),
    # four streams of one position: B H = 16 = G, every workgroup owns a head
    Case("rows4", 64, 4, 64, 2, 20, 4, 0.3),
    # a ring barely longer than / as long as a step: a step's later rows overwrite slots its earlier queries would have seen
    Case("short", 64, 4, 64, 2, 5, 1, 0.3),
    Case("short4", 64, 4, 64, 2, 4, 1, 0.3),
    # null ls1 / ls2
    Case("noscale", 64, 4, 64, 2, 20, 1, None),
)
BY_NAME = {c.name: c for c in CASES}
# new positions per step of each case (each B * T = R in 1 .. 4 is a kernel instance of its own)
TS = {"d16": (1, 2), "d32": (3, 4), "d64": (2,), "d128": (4,), "d256": (1,), "e528": (2,), "e1088": (1,), "f2056": (3,), "rows4": (1,),
      "short": (4,), "short4": (4,), "noscale": (2,)}
RING_CASES = ("d16", "d32", "d64", "d128", "d256")
SHAPE_CASES = ("e528", "e1088", "f2056", "rows4", "short", "short4", "noscale")
STREAM_CASES = ("d64", "short")
STREAM_CUTS = (1, 2, 4, 2, 1, 4)          # from pos = cap - 3: T of consecutive steps (d64 has two streams: T <= 2 there, see stream_cuts)

FLAGS = ("d16", "d32", "d64", "d128", "d256", "R1", "R2", "R3", "R4", "T3", "T4", "slot_batches_2", "slot_batches_3", "wg_without_head",
         "BH_eq_G", "inproj_rounds_3", "outproj_rounds_2", "lin1_row_masked", "k_chunk_2", "k_chunk_3", "k_chunk_partial", "ln_tail",
         "lin2_k_block_2", "lin2_k_block_partial8", "odd_heads", "short_ring", "cap_eq_T", "no_scale", "ring_empty", "unwritten_slots",
         "step_wraps", "wrap_end0", "empty_row", "ctx_none", "ctx_1", "ctx_lt_T", "ctx_masks_old", "ctx_over_wrap", "ctx_gt_cap", "no_rope")


def kv_geometry(case):
    """Thread (dq, cls) of the ring sweeps: GS lanes per ring row, NC slot classes, SPB slots per batch, capS score columns."""
    D = case.E // case.H
    NC = 1024 // D
    return SimpleNamespace(D=D, GS=D // 4, NC=NC, SPB=JB * NC, capS=case.cap + JB * NC)


def stream_cuts(case):
    return tuple(min(t, 4 // case.B) for t in STREAM_CUTS)


def positions(case, T):
    """The positions a ring-geometry case is run at with the product's context (= cap) and rope."""
    g, cap = kv_geometry(case), case.cap
    ps = [0, g.SPB - T, g.SPB - 1, g.SPB, cap - T, cap - 1, cap, cap + 1, 2 * cap + 3]
    out = []
    for p in ps:
        if p >= 0 and p not in out:
            out.append(p)
    return out


def context_steps(case, T):
    """Every kind of context on an unwrapped (nearly full) and on a wrapped ring, plus a window that straddles the wrap."""
    g, cap = kv_geometry(case), case.cap
    ctxs = []
    for ctx in (1, 2, T, g.SPB + 3, cap - 1, cap, cap + 50):
        if ctx not in ctxs:
            ctxs.append(ctx)
    return [Step(pos, ctx, True, T) for pos in (cap - T - 2, cap + 7) for ctx in ctxs] + [Step(cap + 2, 9, True, T)]


def steps(case):
    """Every (pos, context, rope, T) of the position test of a case."""
    cap, ts = case.cap, TS[case.name]
    if case.name in RING_CASES:
        out = [Step(p, cap, True, T) for T in ts for p in positions(case, T)]
        out += context_steps(case, ts[-1])
    else:          # an empty ring, a half-full ring, a step that wraps inside itself, a wrapped ring
        T = ts[-1]
        out = [Step(0, cap, True, T), Step(cap // 2, cap, True, T), Step(cap - 1, cap, True, T), Step(cap + 3, cap, True, T)]
    return out + [Step(cap // 2 + 1, None, False, ts[-1])]


def repair_steps():
    """(case, step) of the repair-launch test."""
    a, b = BY_NAME["d16"], BY_NAME["d64"]
    return [("d16", Step(1030, a.cap, True, 2)), ("d64", Step(b.cap + 1, b.cap, True, 2)), ("e1088", Step(12, 20, True, 1)),
            ("rows4", Step(21, 7, True, 1))]


# ---- the ring map --------------------------------------------------------------------------------------------------------------------------
def slot_position(slot, end, cap):
    """The position ring slot `slot` counts as once `end` positions have been appended (RingKVCache.complete, ring_visible_at in
    csrc/lm_common.h), None when it was never written: the latest p < end with p = slot (mod cap) -- except that the slot the NEXT
    append will take, end % cap, counts as position `end` (the `delta <= 0` branch at delta = 0), which lies in every query's future."""
    if slot >= end or slot >= cap:
        return None
    delta = slot - end % cap
    return end + delta if delta <= 0 else end + delta - cap


def visible(slot, qpos, end, cap, context):
    """Whether the query at position `qpos` sees `slot` of a ring that holds `end` positions."""
    p = slot_position(slot, end, cap)
    return p is not None and 0 <= qpos - p and (not context or qpos - p < context)


def visible_slots(qpos, end, cap, context):
    return [s for s in range(cap) if visible(s, qpos, end, cap, context)]


def new_slots(step, cap):
    return [(step.pos + t) % cap for t in range(step.T)]


def step_mask(step, cap, defect=None):
    """bool [T, cap]: slot s is attended to by query t (all T rows appended before any query reads)."""
    pos, T, ctx = step.pos, step.T, step.context
    g_end = pos if defect == "end_offset_is_pos" else pos + T
    if ctx and defect == "window_wide":
        ctx += 1
    if ctx and defect == "window_narrow":
        ctx = max(1, ctx - 1)
    m = torch.zeros(T, cap, dtype=torch.bool)
    for t in range(T):
        end = pos + t + 1 if defect == "append_per_query" else g_end
        for s in range(cap):
            m[t, s] = visible(s, pos + t, end, cap, ctx)
        if defect == "own_hidden":
            m[t, (pos + t) % cap] = False
        if defect == "unused_slot_read" and pos + T < cap:
            m[t, pos + T] = True
    return m


# ---- the launcher's geometry --------------------------------------------------------------------------------------------------------------
def lds_bytes(case, T):
    """ct_lds_bytes: header | xs [R][max(E, F)] | xres [R][E] | qh [T][3][D] | sraw, pB [R][capS] | opart [1024][R] | wred [2][4][R]."""
    R, D = case.B * T, case.E // case.H
    return (DF_HDR_FLOATS + R * max(case.E, case.F) + R * case.E + T * 3 * D + 2 * R * (case.cap + 16384 // D) + (1024 + 2 * DF_WAVES) * R) * 4


def row_rounds(N, K, RU, CU, W):
    """One `df_rows<R>` instance (persist.h, `DfPre<true, RU, CU, false>`) over an [N, K] matrix: (row rounds of the wave that owns row 0, k blocks per round)."""
    return -(-N // (RU * W)), -(-K // (CU * K_CHUNK))


def grid(case, T, cus, step=None):
    """rst_codec_tr_grid, ct_lds_bytes and the loop bounds of codec_tr_kernel: G, W = 4 G, whether the launcher serves the shape (`ok`)
    and the set of paths taken (`flags`) -- those of the shape alone, or with `step` also those of the ring geometry at that step."""
    c = case
    E, H, F, cap, B = c.E, c.H, c.F, c.cap, c.B
    R = B * T
    ok = B >= 1 and 1 <= T <= DF_WAVES and R <= 4 and E > 0 and E % 8 == 0 and F > 0 and F % 8 == 0 and H > 0 and E % H == 0 and \
        1 <= c.L <= MAX_L and cap >= T
    D = E // H if ok else 0
    ok = ok and D in (16, 32, 64, 128, 256)
    lds = lds_bytes(c, T) if ok else 0
    G = min(cus, max(1, -(-min(3 * E, F) // DF_WAVES)))
    ok = bool(ok and lds <= LDS_LIMIT and B * H <= G)
    W = G * DF_WAVES
    out = SimpleNamespace(G=G, W=W, ok=ok, lds=lds, D=D, R=R)
    if not ok:
        out.flags = frozenset()
        return out
    kg = kv_geometry(c)
    out.SPB, out.NC, out.capS = kg.SPB, kg.NC, kg.capS
    out.rounds = {"in_proj": row_rounds(3 * E, E, 2, 1, W), "out_proj": row_rounds(E, E, 1, 1, W), "linear1": row_rounds(F, E, 2, 1, W),
                  "linear2": row_rounds(E, F, 1, 4, W)}
    f = {f"d{D}", f"R{R}"}
    if T >= 3:
        f.add(f"T{T}")
    if G > B * H:
        f.add("wg_without_head")
    if G == B * H:
        f.add("BH_eq_G")
    if out.rounds["in_proj"][0] >= 3:
        f.add("inproj_rounds_3")
    if out.rounds["out_proj"][0] >= 2:
        f.add("outproj_rounds_2")
    if 0 < F % (2 * W) <= W:          # the waves of the last round own one live row; the second, r + W >= F, is masked
        f.add("lin1_row_masked")
    if E > K_CHUNK:
        f.add("k_chunk_2")
        if E % K_CHUNK:
            f.add("k_chunk_partial")
    if E > 2 * K_CHUNK:
        f.add("k_chunk_3")
    if E > LN_REG:
        f.add("ln_tail")
    if F > K_BLOCK2:
        f.add("lin2_k_block_2")
        if F % K_BLOCK2 == 8:
            f.add("lin2_k_block_partial8")
    if H % 2:
        f.add("odd_heads")
    if cap < 2 * T:
        f.add("short_ring")
    if cap == T:
        f.add("cap_eq_T")
    if c.scale is None:
        f.add("no_scale")
    if step is not None:
        pos, ctx = step.pos, step.context
        end = pos + T
        n_used = min(cap, end)
        nb = -(-n_used // kg.SPB)
        out.n_used, out.nb = n_used, nb
        assert nb * kg.SPB <= kg.capS          # the score rows hold every batch the sweeps touch
        if nb in (2, 3):
            f.add(f"slot_batches_{nb}")
        if pos == 0:
            f.add("ring_empty")
        if end < cap:
            f.add("unwritten_slots")
        if pos % cap + T > cap:
            f.add("step_wraps")
        if end % cap == 0:
            f.add("wrap_end0")
        vis = [visible_slots(pos + t, end, cap, ctx) for t in range(T)]
        if any(not v for v in vis):
            f.add("empty_row")
        if not ctx:
            f.add("ctx_none")
        else:
            if ctx == 1:
                f.add("ctx_1")
            if ctx < T:
                f.add("ctx_lt_T")
            if ctx > cap:
                f.add("ctx_gt_cap")
            if any(len(v) < len(visible_slots(pos + t, end, cap, None)) for t, v in enumerate(vis)):
                f.add("ctx_masks_old")
            if any(ctx < cap - 1 and v and v[0] == 0 and v[-1] == cap - 1 for v in vis):
                f.add("ctx_over_wrap")
        if not step.rope:
            f.add("no_rope")
    out.flags = frozenset(f)
    return out


def case_flags(case, cus):
    """Every path the position test of `case` takes on a device of `cus` CUs."""
    f = set()
    for st in steps(case):
        f |= grid(case, st.T, cus, st).flags
    return frozenset(f)


# ---- operands ------------------------------------------------------------------------------------------------------------------------------
def _seed(name, seed):
    s = seed
    for ch in name:
        s = (s * 1000003 + ord(ch)) % (1 << 62)
    return s


def make_case(case, seed=0):
    """CPU operands, all fp32: weights of randn / sqrt(K), LayerNorm gains 1 + 0.1 randn and biases 0.1 randn, LayerScale vectors
    scale x (0.75 .. 1.25) or None, the input of four positions per stream (a step of T takes the first T), and per layer the
    rings' base contents (0.5 randn) with the signs of their poison."""
    c = case
    g = torch.Generator().manual_seed(_seed(c.name, seed))
    E, F, H, D, B = c.E, c.F, c.H, c.E // c.H, c.B

    def w(rows, cols):
        return torch.randn(rows, cols, generator=g) / math.sqrt(cols)

    def vec(mean, spread):
        return mean + spread * torch.randn(E, generator=g)
    o = SimpleNamespace(case=c, eps=float(torch.tensor(EPS, dtype=torch.float32)))
    o.in_proj = [w(3 * E, E) for _ in range(c.L)]
    o.out_proj = [w(E, E) for _ in range(c.L)]
    o.linear1 = [w(F, E) for _ in range(c.L)]
    o.linear2 = [w(E, F) for _ in range(c.L)]
    o.norm1_w, o.norm1_b = [vec(1.0, 0.1) for _ in range(c.L)], [vec(0.0, 0.1) for _ in range(c.L)]
    o.norm2_w, o.norm2_b = [vec(1.0, 0.1) for _ in range(c.L)], [vec(0.0, 0.1) for _ in range(c.L)]
    for n in ("scale1", "scale2"):
        setattr(o, n, [None if c.scale is None else c.scale * (0.75 + 0.5 * torch.rand(E, generator=g)) for _ in range(c.L)])
    o.x = torch.randn(B, 4, E, generator=g)
    o.ring_base = [tuple(0.5 * torch.randn(B, H, c.cap, D, generator=g) for _ in range(2)) for _ in range(c.L)]
    o.poison_sign = [torch.where(torch.rand(B, H, c.cap, D, generator=g) < 0.5, -1.0, 1.0) for _ in range(c.L)]
    return o


def make_rings(co, step):
    """Per layer (K, V) fp32 ``[B, H, cap, D]`` before the step: the base contents where a query of the step may look, K = 0 and
    V = +-2^14 in every other slot, the new positions' own slots included."""
    return poison(co, [(K.clone(), V.clone()) for K, V in co.ring_base], step)


def poison(co, rings, step):
    """K = 0, V = +-2^14 (in place) in every slot of `rings` that no query of the step may see."""
    cap = co.case.cap
    hidden = ~step_mask(step, cap).any(0)
    hidden[new_slots(step, cap)] = True
    for l, (K, V) in enumerate(rings):
        K[:, :, hidden] = 0.0
        V[:, :, hidden] = (POISON * co.poison_sign[l])[:, :, hidden]
    return rings


# ---- the reference ------------------------------------------------------------------------------------------------------------------------
# xs [L, B, T, E]: every layer's output | the last layer's qkv [B, T, 3E] (before the rotation), att [B, T, E], hid [B, T, F] (after the
# GELU), x1 [B, T, E] (the residual stream between attention and FFN) | k_new, v_new [L, B, H, T, D]: the step's keys (rotated) and
# values as computed | k_row, v_row: the rows attended to and written | gx [B, T, E]: the last layer's output as the hand-off
# workspace holds it (launches only)
Ref = namedtuple("Ref", "xs qkv att hid x1 k_new v_new k_row v_row gx", defaults=(None,))
DEFECTS = ("window_wide", "window_narrow", "own_hidden", "end_offset_is_pos", "append_per_query", "rope_pos_ignores_t", "unused_slot_read",
           "k_tail_dropped", "ln_tail_dropped", "ln_unbiased", "scale_skipped", "second_batch_dropped", "head_of_other_stream")


def rope_coef(D):
    from rstnet_amd import ops
    return ops.rope_coef(MAX_PERIOD, D)


def reference(co, step, rings, dtype=torch.float64, defect=None, own=None):
    """One step of ``step.T`` positions from ``step.pos`` through all layers in ``dtype``.  ``rings``: per layer (K, V)
    ``[B, H, cap, D]`` before the step; ``own``: per layer (k, v) ``[B, H, T, D]`` the rows a launch wrote for the new positions --
    teacher forcing, the reference then attends to exactly those rows -- or None: its own keys / values."""
    c = co.case
    E, H, F, L, cap, B = c.E, c.H, c.F, c.L, c.cap, c.B
    D, T, pos = E // H, step.T, step.pos
    eps = torch.tensor(co.eps, dtype=torch.float32).to(dtype)
    SPB = kv_geometry(c).SPB
    mask = step_mask(step, cap, defect)
    if defect == "second_batch_dropped":
        mask[:, SPB:] = False
    slots = torch.tensor(new_slots(step, cap))

    def lin(v, wt, block=K_CHUNK):
        K = wt.shape[1]
        if defect == "k_tail_dropped" and K > block:
            K = (K // block) * block
        return v[..., :K] @ wt[:, :K].to(dtype).T

    def norm(v, gamma, beta):
        s = v[..., :LN_REG] if defect == "ln_tail_dropped" else v
        mean = s.mean(-1, keepdim=True)
        var = ((s - mean) ** 2).sum(-1, keepdim=True) / (s.shape[-1] - (1 if defect == "ln_unbiased" else 0))
        return (v - mean) / torch.sqrt(var + eps) * gamma.to(dtype) + beta.to(dtype)

    def rotate(v):          # [B, H, T, D], interleaved (real, imaginary) pairs at position pos + t
        if not step.rope:
            return v
        freqs = torch.exp(torch.arange(D // 2, dtype=dtype) * rope_coef(D))
        ts = torch.tensor([float(pos)], dtype=dtype) + (0 if defect == "rope_pos_ignores_t" else torch.arange(T, dtype=dtype))
        ang = freqs * ts.view(-1, 1)
        cs, sn = torch.cos(ang), torch.sin(ang)
        a, b = v[..., 0::2], v[..., 1::2]
        return torch.stack([a * cs - b * sn, a * sn + b * cs], -1).reshape(B, H, T, D)

    def scaled(u, s):
        return u if s is None or defect == "scale_skipped" else u * s.to(dtype)

    x = co.x[:, :T].to(dtype)
    xs, k_new, v_new, k_row, v_row = [], [], [], [], []
    for l in range(L):
        qkv = lin(norm(x, co.norm1_w[l], co.norm1_b[l]), co.in_proj[l])
        q, k, v = qkv.view(B, T, 3, H, D).permute(2, 0, 3, 1, 4)
        q, k = rotate(q), rotate(k)
        kr, vr = (own[l][0].to(dtype), own[l][1].to(dtype)) if own is not None else (k, v)
        K0, V0 = rings[l][0].to(dtype), rings[l][1].to(dtype)
        K, V = K0.clone(), V0.clone()
        K[:, :, slots], V[:, :, slots] = kr, vr
        att = torch.zeros(B, H, T, D, dtype=dtype)
        for t in range(T):
            Kt, Vt = K, V
            if defect == "append_per_query":          # the rows of the later positions are not in the ring yet
                Kt, Vt = K0.clone(), V0.clone()
                Kt[:, :, slots[:t + 1]], Vt[:, :, slots[:t + 1]] = kr[:, :, :t + 1], vr[:, :, :t + 1]
            if defect == "head_of_other_stream" and B > 1:
                Kt, Vt = torch.cat([Kt[:1], Kt[:-1]]), torch.cat([Vt[:1], Vt[:-1]])
            idx = mask[t].nonzero().view(-1)
            if idx.numel():
                sc = torch.einsum("bhd,bhsd->bhs", q[:, :, t], Kt[:, :, idx]) / math.sqrt(D)
                att[:, :, t] = torch.einsum("bhs,bhsd->bhd", torch.softmax(sc, -1), Vt[:, :, idx])
        att = att.permute(0, 2, 1, 3).reshape(B, T, E)
        x1 = x + scaled(lin(att, co.out_proj[l]), co.scale1[l])
        hid = torch.nn.functional.gelu(lin(norm(x1, co.norm2_w[l], co.norm2_b[l]), co.linear1[l]))
        x = x1 + scaled(lin(hid, co.linear2[l], K_BLOCK2), co.scale2[l])
        xs.append(x)
        k_new.append(k), v_new.append(v), k_row.append(kr), v_row.append(vr)
    return Ref(torch.stack(xs), qkv, att, hid, x1, torch.stack(k_new), torch.stack(v_new), torch.stack(k_row), torch.stack(v_row))


def rows_of(ref):
    """The rows a run wrote, in the form `reference(own=...)` takes."""
    return [(ref.k_row[l], ref.v_row[l]) for l in range(ref.k_row.shape[0])]


def append(rings, step, ref, case):
    """The rings after the step: the rows of `ref` in the new positions' slots of every layer (streaming on the CPU)."""
    slots = torch.tensor(new_slots(step, case.cap))
    for l, (K, V) in enumerate(rings):
        K[:, :, slots], V[:, :, slots] = ref.k_row[l].float(), ref.v_row[l].float()
    return rings


# ---- acceptance ---------------------------------------------------------------------------------------------------------------------------
def _ratio0(got, ref):
    """`ratio`, or max |got| where the reference vector is all zero (a query that sees no slot)."""
    return ratio(got, ref) if float(ref.abs().max()) > 0 else ratio(got + 1.0, ref + 1.0)


def ratios(got, ref, case, rows="written"):
    """The ratio (max |got - ref| / max |ref|) of every vector the tests bound, per row (stream, position): every layer's output, the
    last layer's qkv / GELU activation / residual hand-offs where `got` has them, the attention output per row and head, and per
    layer, row and head the key and value against the reference's own: ``rows`` "written": the rows `got` left in the rings,
    "computed": the keys / values `got` computed itself (a teacher-forced run of the reference attends to given rows, its own
    rotation and projection error shows only here)."""
    H, D = case.H, case.E // case.H
    L, B, T, _ = ref.xs.shape
    out = {}
    for b in range(B):
        for t in range(T):
            at = f"stream {b}, t {t}"
            for l in range(L):
                out[f"x[layer {l}, {at}]"] = ratio(got.xs[l, b, t], ref.xs[l, b, t])
            for name, mine, theirs in (("qkv", got.qkv, ref.qkv), ("hid", got.hid, ref.hid), ("x1", got.x1, ref.x1), ("x[hand-off]", got.gx, ref.xs[-1])):
                if mine is not None:
                    out[f"{name}[{at}]"] = ratio(mine[b, t], theirs[b, t])
            if got.att is not None:
                for h in range(H):
                    out[f"att[{at}, head {h}]"] = _ratio0(got.att[b, t].reshape(H, D)[h], ref.att[b, t].reshape(H, D)[h])
            gk, gv = (got.k_row, got.v_row) if rows == "written" else (got.k_new, got.v_new)
            for l in range(L):
                for h in range(H):
                    out[f"k_row[layer {l}, {at}, head {h}]"] = ratio(gk[l, b, h, t], ref.k_new[l, b, h, t])
                    out[f"v_row[layer {l}, {at}, head {h}]"] = ratio(gv[l, b, h, t], ref.v_new[l, b, h, t])
    return out


def reference_error(ref32, ref64, case):
    """(name, ratio) of the worst vector of the fp32 run of the reference against its fp64 run, both attending to the same written
    rows: every vector `accept` bounds, the keys and values as each run computed them (rotated at its own precision)."""
    return worst(ratios(ref32, ref64, case, rows="computed"))


def tolerance(ref32, ref64, case):
    """depth_frame_ref.tolerance's rule: TOL_FACTOR x the worst ratio of the fp32 run of the reference against its fp64 run, within
    [TOL_FLOOR, TOL_CEIL]."""
    return min(max(TOL_FACTOR * reference_error(ref32, ref64, case)[1], TOL_FLOOR), TOL_CEIL)


def accept(got, ref64, tol, case):
    """(every vector and written row within tol, name of the worst, its ratio)."""
    rs = ratios(got, ref64, case)
    name, r = worst(rs)
    return all(v <= tol for v in rs.values()), name, r


# ---- the hand-off workspace ---------------------------------------------------------------------------------------------------------------
def granules(case, T):
    """rst_codec_tr_workspace_granules: one set; the workspace holds the persistent launch's, then the repair launch's."""
    return case.B * T * (5 * case.E + case.F)


def layout(case, T):
    """(name, first granule, rows, width) of X [R][E] | QKV [R][3E] | ATT [R][E] | H [R][F] within a set; row = stream * T + t."""
    R, out, off = case.B * T, [], 0
    for name, width in (("X", case.E), ("QKV", 3 * case.E), ("ATT", case.E), ("H", case.F)):
        out.append((name, off, R, width))
        off += R * width
    return out


def epochs(L):
    """The tag of every granule array after a launch over L layers: each op publishes once per layer, X twice."""
    return {"X": 2 * L, "QKV": L, "ATT": L, "H": L}


def read_handoff(ws, case, T, solo=False):
    """The fp32 value (low word) and the epoch tag (high word) of every {tag, value} granule of one set as CPU tensors X, QKV, ATT, H
    ``[B, T, width]`` and X_tag, ...  ``solo``: the repair launch's own set."""
    n = granules(case, T)
    words = ws[n if solo else 0:2 * n if solo else n].view(torch.int32).view(-1, 2).cpu()
    out = {}
    for name, off, rows, width in layout(case, T):
        out[name] = words[off:off + rows * width, 0].contiguous().view(torch.float32).view(case.B, T, width)
        out[name + "_tag"] = words[off:off + rows * width, 1].contiguous().view(case.B, T, width)
    return SimpleNamespace(**out)


# ---- device side --------------------------------------------------------------------------------------------------------------------------
def device_case(co, dev):
    """The operands on the device in the form ops.codec_transformer_frame takes, rings of the case's capacity.  Every weight matrix and
    every gamma / beta / scale vector is followed by one row of NaN and every ring by one head of NaN: a load past the operand that is
    multiplied by a padding zero or a zero softmax weight still turns its sum into NaN, which no bound accepts."""
    c = co.case
    D = c.E // c.H

    def guarded(w):
        w2 = w.view(1, -1) if w.dim() == 1 else w
        buf = torch.full((w2.shape[0] + 1, w2.shape[1]), float("nan"), device=dev, dtype=torch.float32)
        buf[:-1] = w2.to(dev)
        return buf[:-1].view(w.shape)

    def ring():
        return torch.full((c.B * c.H + 1, c.cap, D), float("nan"), device=dev, dtype=torch.float32)[:c.B * c.H].view(c.B, c.H, c.cap, D)
    layers = []
    for l in range(c.L):
        ly = {n: guarded(getattr(co, n)[l]) for n in ("in_proj", "out_proj", "linear1", "linear2", "norm1_w", "norm1_b", "norm2_w", "norm2_b")}
        ly["scale1"] = None if co.scale1[l] is None else guarded(co.scale1[l])
        ly["scale2"] = None if co.scale2[l] is None else guarded(co.scale2[l])
        ly["k_cache"], ly["v_cache"] = ring(), ring()
        layers.append(ly)
    return SimpleNamespace(case=c, co=co, dev=dev, layers=layers, x=co.x.to(dev))


def upload_rings(d, rings):
    for ly, (K, V) in zip(d.layers, rings):
        ly["k_cache"].copy_(K)
        ly["v_cache"].copy_(V)


def download_rings(d):
    return [(ly["k_cache"].cpu(), ly["v_cache"].cpu()) for ly in d.layers]


def launch(d, step, status_code=0):
    """One step on the rings as they are on the device: the launch over all layers, then over the first L - 1 .. 1 layers (each
    layer's output).  ``status_code``: planted in the device's status[0] before every launch (the other words zeroed), so that the
    repair launch behind each persistent one recomputes the step; the readout is then the repair launch's granule set.  Returns (what
    the launches left as a `Ref` with the written rows, the status words after every launch -- full launch first --, the tags of the
    read granule set, the input as it is after the launches, the rings after the launches)."""
    from rstnet_amd import ops
    c, T = d.case, step.T
    pos_dev = torch.tensor([step.pos], dtype=torch.int64, device=d.dev)
    x = d.x[:, :T].contiguous()
    status = ops.codec_transformer_status(torch.device(d.dev))
    ys, hand, words = [None] * c.L, None, []
    for l in range(c.L, 0, -1):
        if status_code:
            status.zero_()
            status[0] = status_code
        ys[l - 1] = ops.codec_transformer_frame(x, d.layers[:l], pos_dev, H=c.H, context=step.context, rope=step.rope, max_period=MAX_PERIOD,
                                                eps=d.co.eps)
        torch.cuda.synchronize()
        words.append(status.tolist())
        if l == c.L:
            hand = read_handoff(ops.frame_workspace("codec_transformer", (c.B * T, c.E, c.F), d.dev), c, T, solo=bool(status_code))
    after = download_rings(d)
    slots = torch.tensor(new_slots(step, c.cap))
    got = Ref(torch.stack([y.cpu() for y in ys]), hand.QKV, hand.ATT, hand.H, None, None, None,
              torch.stack([K[:, :, slots] for K, _ in after]), torch.stack([V[:, :, slots] for _, V in after]), hand.X)
    tags = {n: getattr(hand, n + "_tag") for n in ("X", "QKV", "ATT", "H")}
    return got, words, tags, x.cpu(), after
