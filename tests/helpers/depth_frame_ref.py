"""The persistent depth-frame launch (csrc/lm_depth.hip behind ops.depth_decode_frame) restated for its step-by-step tests: the case
table, CPU operands, a teacher-forced reference of the depth phase in any dtype (fp64 for the bound, fp32 for the tolerance) that can
carry one named defect, the launcher's grid and loop bounds (`grid`), the readout of the hand-off workspace, pointer tables for the
first q' steps of a frame, the designed noise / limits of the sampler readout and the acceptance function.  Nothing here needs a GPU
until `device_tables` is called; tests/test_depth_frame_steps_cpu.py checks the table's coverage, the reference against
oracle/lm_oracle.py, the ring map against RingKV.complete and that every defect is rejected.

Why prefixes: the launch keeps one step's logits at a time (the hand-off buffer gLOG is overwritten by the next step), but steps
0 .. q'-1 of a launch over the first q' steps' weights, with the ring capacity of the full frame, are the same computation as in the
full launch, so the last-step logits of prefix q' are the full frame's step q'-1 logits."""
import ctypes as C
import functools
import math
from collections import namedtuple
from types import SimpleNamespace

import torch

DF_WAVES, DF_THREADS, DF_NORM_J, DF_HDR_FLOATS = 4, 256, 8, 512          # csrc/persist.h, csrc/lm_depth.hip
MAX_Q = MAX_L = 8                                                         # RST_DEPTH_MAX_Q / _L
K_CHUNK_E, K_CHUNK_HD = 2 * 512, 6 * 512                                  # k covered by one pass of df_rows' kb loop (CU 2 / CU 6)
LDS_LIMIT, LDS_CLASS = 150 * 1024, 64 * 1024
LO, HI = 2.0 ** -40, 2.0 ** 40
EPS = 1e-5

# ---- the case table -----------------------------------------------------------------------------------------------------------------------
# text: what column 0 of the token matrix holds per batch row -- "ok" a valid id, "neg1" the id -1 (zero embedding), "big" an id past the
# text table (clamped to its last row)
Case = namedtuple("Case", "name B E H Hd card Q L top_k ring_cap context bias text")


def _both(name, text1, text2, **kw):
    return [Case(name=f"{name}-B1", B=1, text=(text1,), **kw), Case(name=f"{name}-B2", B=2, text=text2, **kw)]


CASES = (
    # G 10, W 40: a ragged second row block in the in-projection (192 rows, RU 3), the gate pairs (176, RU 3) and the E-row ops (64, RU 1)
    _both("rows", "neg1", ("big", "ok"), E=64, H=2, Hd=176, card=37, Q=3, L=2, top_k=50, ring_cap=3, context=None, bias=True)
    # G 10, W 40: the head's second row block (100 rows, RU 2); a ring one slot longer than the frame
    + _both("headrows", "big", ("ok", "neg1"), E=64, H=4, Hd=40, card=100, Q=4, L=1, top_k=25, ring_cap=5, context=None, bias=False)
    # G 88, W 352 > E: waves without a row in the out-projection and the FFN out; D 8
    + _both("idle", "ok", ("neg1", "big"), E=128, H=16, Hd=352, card=2048, Q=2, L=2, top_k=250, ring_cap=2, context=None, bias=False)
    # G 16 = H: every workgroup owns a head; the longest frame the launch takes
    + _both("heads16", "neg1", ("ok", "big"), E=128, H=16, Hd=64, card=64, Q=8, L=8, top_k=25, ring_cap=8, context=3, bias=True)
    # D 24: lanes 24 .. 63 of the attention wave idle; sample_row<256, 16> one id past its threshold
    + _both("d24", "big", ("neg1", "ok"), E=96, H=4, Hd=104, card=2049, Q=4, L=1, top_k=250, ring_cap=5, context=2, bias=True)
    # D 192: three passes of the attention's dd loops; a one-step frame
    + _both("d192", "ok", ("big", "neg1"), E=384, H=2, Hd=200, card=300, Q=1, L=2, top_k=25, ring_cap=2, context=None, bias=False)
    # E 1088: a second pass of the kb loop with 64 of its 1024 columns live
    + _both("e1088", "neg1", ("ok", "big"), E=1088, H=17, Hd=264, card=300, Q=2, L=1, top_k=25, ring_cap=2, context=None, bias=True)
    # Hd 3080: a second pass of the FFN out's kb loop with 8 of its 3072 columns live
    + _both("hd3080", "big", ("neg1", "ok"), E=64, H=2, Hd=3080, card=40, Q=2, L=1, top_k=8, ring_cap=3, context=None, bias=False)
    # E 2304: the norm's tail loop, D 128, a third pass of the kb loop, sample_row<256, 16> at its largest row; > 64 KB of LDS at batch 2
    + _both("wide", "ok", ("big", "neg1"), E=2304, H=18, Hd=512, card=4096, Q=2, L=1, top_k=250, ring_cap=2, context=None, bias=True)
    # Hd 16392: > 64 KB of LDS at batch 1 (xs [B][Hd]); six passes of the FFN out's kb loop
    + [Case(name="hd16392-B1", B=1, text=("ok",), E=64, H=2, Hd=16392, card=40, Q=2, L=1, top_k=8, ring_cap=2, context=None, bias=True)]
)
CASES = tuple(CASES)
BY_NAME = {c.name: c for c in CASES}
# the repair launch: the two smallest cases, a second kb pass, and 16 heads walked by the one workgroup
REPAIR_CASES = ("rows-B1", "headrows-B2", "e1088-B2", "heads16-B1")

FLAGS = ("rows2_in", "rows2_gate", "rows2_out", "rows2_head", "idle_waves", "k_partial", "k2_E", "k2_Hd", "norm_tail", "lds_big",
         "D8", "D24", "D128", "D192", "H_eq_G", "H_lt_G", "s8", "s16", "card37", "card2048", "card2049", "card4096", "topk_ge_card",
         "Q1", "Q8L8", "L1", "ring_eq_Q", "ring_Q_plus_1", "ctx2", "ctx3", "tok_neg1", "tok_big", "rows_differ", "bias", "no_bias")


def emb_rows(case):
    """Rows of step k's embedding table: a short text table, then audio tables that alternate between card + 1 rows and half the
    card, so that the tokens the launch draws itself are clamped at the even steps."""
    return [11] + [case.card + 1 if k % 2 else max(2, case.card // 2) for k in range(1, case.Q)]


def lds_bytes(case):
    """df_lds_bytes."""
    B, E, Hd, D = case.B, case.E, case.Hd, case.E // case.H
    fl = DF_HDR_FLOATS + B * max(E, Hd) + B * E + B * case.card + B * 3 * D + case.L * case.Q * B * 2 * D
    fl += fl & 1
    k = case.top_k if 0 < case.top_k < case.card else case.card
    return fl * 4 + ((k + 7) & ~7) * 8


def grid(case, cus):
    """rst_depth_frame_grid / df_grid_for_rows and the loop bounds of df_rows, df_rmsnorm, the attention and the sampler dispatch:
    G, W = 4 G, the LDS footprint, whether the launcher serves the shape (`ok`) and the set of paths the case takes (`flags`)."""
    c = case
    E, Hd, card, H = c.E, c.Hd, c.card, c.H
    D = E // H
    ok = (1 <= c.B <= 2 and E > 0 and E % 8 == 0 and Hd > 0 and Hd % 8 == 0 and H > 0 and H * D == E and 0 < card <= 16 * DF_THREADS
          and 1 <= c.Q <= MAX_Q and 1 <= c.L <= MAX_L and c.ring_cap >= c.Q)
    lds = lds_bytes(c)
    ok = ok and lds <= LDS_LIMIT
    g = -(-min(3 * E, Hd, card) // DF_WAVES)
    G = max(g, 1) if g < cus else cus
    ok = ok and H <= G
    W = G * DF_WAVES
    f = set()

    def second_block(rows, RU):
        return rows > RU * W and rows % W != 0
    if second_block(3 * E, 3):
        f.add("rows2_in")
    if second_block(Hd, 3):
        f.add("rows2_gate")
    if second_block(E, 1):
        f.add("rows2_out")
    if second_block(card, 2):
        f.add("rows2_head")
    if E < W:
        f.add("idle_waves")
    if any(K < 512 and K % 512 for K in (E, Hd)):
        f.add("k_partial")
    if E > K_CHUNK_E and E % K_CHUNK_E:
        f.add("k2_E")
    if Hd > K_CHUNK_HD and Hd % K_CHUNK_HD:
        f.add("k2_Hd")
    if E > DF_NORM_J * DF_THREADS:
        f.add("norm_tail")
    if lds > LDS_CLASS:
        f.add("lds_big")
    if D in (8, 24, 128, 192):
        f.add(f"D{D}")
    f.add("H_eq_G" if H == G else "H_lt_G")
    f.add("s8" if card <= 8 * DF_THREADS else "s16")
    if card in (37, 2048, 2049, 4096):
        f.add(f"card{card}")
    if not 0 < c.top_k < card:
        f.add("topk_ge_card")
    if c.Q == 1:
        f.add("Q1")
    if c.Q == 8 and c.L == 8:
        f.add("Q8L8")
    if c.L == 1:
        f.add("L1")
    if c.ring_cap == c.Q and c.Q >= 2:
        f.add("ring_eq_Q")
    if c.ring_cap == c.Q + 1:
        f.add("ring_Q_plus_1")
    if c.context in (2, 3) and c.Q >= 4:
        f.add(f"ctx{c.context}")
    if "neg1" in c.text:
        f.add("tok_neg1")
    if "big" in c.text:
        f.add("tok_big")
    if len(set(emb_rows(c))) > 1:
        f.add("rows_differ")
    f.add("bias" if c.bias else "no_bias")
    return SimpleNamespace(G=G, W=W, lds=lds, ok=bool(ok), flags=frozenset(f))


# ---- operands ------------------------------------------------------------------------------------------------------------------------------
def _seed(name, seed):
    s = seed
    for ch in name:
        s = (s * 1000003 + ord(ch)) % (1 << 62)
    return s


def text_tokens(case):
    rows0 = emb_rows(case)[0]
    return torch.tensor([{"ok": 3 + b, "neg1": -1, "big": rows0 + 5}[kind] for b, kind in enumerate(case.text)], dtype=torch.long)


def make_case(case, seed=0, limits=None):
    """The operands of a case on the CPU, fp32 numbers that bf16 holds exactly (norm gains, bias and h_all are fp32 in the product).
    ``limits``: the per-step id limits of the sampler readout -- the step's head bias (created when the case has none) gets +8 at the
    first blanked id."""
    c = case
    g = torch.Generator().manual_seed(_seed(c.name.split("-")[0], seed))          # the batch sizes of a shape share their weights
    E, Hd, Q, L = c.E, c.Hd, c.Q, c.L

    def w(rows, cols, fan_in=None):
        return (torch.randn(rows, cols, generator=g) / math.sqrt(fan_in or cols)).bfloat16().float()
    o = SimpleNamespace(case=c, eps=float(torch.tensor(EPS, dtype=torch.float32)), ring_cap=c.ring_cap, context=c.context)
    o.in_proj = [w(Q * 3 * E, E) for _ in range(L)]
    o.out_proj = [w(Q * E, E) for _ in range(L)]
    o.norm1 = [1 + 0.1 * torch.randn(E, generator=g) for _ in range(L)]
    o.norm2 = [1 + 0.1 * torch.randn(E, generator=g) for _ in range(L)]
    o.gate_in = [[w(2 * Hd, E) for _ in range(Q)] for _ in range(L)]
    o.gate_out = [[w(E, Hd) for _ in range(Q)] for _ in range(L)]
    o.heads = [w(c.card, E) for _ in range(Q)]
    o.head_bias = [0.5 * torch.randn(c.card, generator=g) if c.bias else None for _ in range(Q)]
    o.emb = [w(r, E, fan_in=1) for r in emb_rows(c)]
    o.h_all = torch.randn(2, Q * E, generator=g)[:c.B].contiguous()
    o.text = text_tokens(c)
    if limits is not None:
        for k, lim in enumerate(limits):
            if o.head_bias[k] is None:
                o.head_bias[k] = torch.zeros(c.card)
            if 0 < lim < c.card:
                o.head_bias[k][lim] += 8.0
    return o


# ---- the reference ------------------------------------------------------------------------------------------------------------------------
Ref = namedtuple("Ref", "logits qkv att hid x")          # [Q, B, card] | the hand-off vectors of the last (step, layer): [B, 3E], [B, E], [B, Hd], [B, E]
DEFECTS = ("last_row_block", "k_tail_E", "k_tail_Hd", "norm_tail", "head_dims", "hidden_slot", "context_ignored", "ring_cap_as_Q",
           "bias_ignored", "neg1_not_zeroed", "unclamped_row0")
SAMPLER_DEFECTS = ("noise_step0", "limit_step0", "noise_row0")


def ring_visible(slot, pos, cap, context, end_offset):
    """Whether ring slot `slot` is seen by the query at position `pos` right after the append that made `end_offset` steps: the slot ->
    position map of RingKVCache.complete with the mask of the streaming attention (position known, not in the future, within the
    context)."""
    end_index = end_offset % cap
    delta = slot - end_index
    pk = end_offset + delta if delta <= 0 else end_offset + delta - cap
    if slot >= end_offset:
        pk = -1
    ok = slot < cap and pk >= 0 and pos - pk >= 0
    if context:
        ok = ok and pos - pk < context
    return ok


def visible_steps(k, Q, cap, context, defect=None):
    """The earlier steps (= ring slots: a frame never wraps its ring) that step k of a frame attends to."""
    if defect == "context_ignored":
        context = None
    if defect == "ring_cap_as_Q":
        cap = Q
    if defect == "hidden_slot":          # positions taken as the slots themselves: plain causal attention
        return [s for s in range(k + 1) if not context or k - s < context]
    return [s for s in range(k + 1) if ring_visible(s, k, cap, context, k + 1)]


def reference(co, tokens, dtype=torch.float64, defect=None):
    """The depth phase teacher-forced with ``tokens`` int64 ``[B, >= Q]`` (column k is the input of step k) in ``dtype``."""
    c = co.case
    B, E, H, Hd, Q, L = c.B, c.E, c.H, c.Hd, c.Q, c.L
    D = E // H
    eps = torch.tensor(co.eps, dtype=torch.float32).to(dtype)
    W = grid(c, 256).W
    kE = (E // K_CHUNK_E) * K_CHUNK_E if defect == "k_tail_E" and E > K_CHUNK_E else E
    kH = (Hd // K_CHUNK_HD) * K_CHUNK_HD if defect == "k_tail_Hd" and Hd > K_CHUNK_HD else Hd

    def lin(x, wt, K, RU):
        y = x[:, :K] @ wt[:, :K].to(dtype).T
        span = RU * W
        if defect == "last_row_block" and y.shape[1] > span:
            y[:, ((y.shape[1] - 1) // span) * span:] = 0
        return y

    def norm(x, alpha):
        y = x * (alpha.to(dtype) / torch.sqrt(eps + (x * x).mean(-1, keepdim=True)))
        if defect == "norm_tail":
            y[:, DF_NORM_J * DF_THREADS:] = x[:, DF_NORM_J * DF_THREADS:]
        return y
    keys = torch.zeros(L, Q, B, H, D, dtype=dtype)
    vals = torch.zeros(L, Q, B, H, D, dtype=dtype)
    dl = min(D, 64) if defect == "head_dims" else D
    logits, last = [], None
    for k in range(Q):
        tok, rows = tokens[:, k], co.emb[k].shape[0]
        zero = tok == -1 if defect != "neg1_not_zeroed" else torch.zeros_like(tok, dtype=torch.bool)
        idx = tok.clamp(0, rows - 1)
        if defect == "unclamped_row0":
            idx = torch.where(tok >= rows, torch.zeros_like(idx), idx)
        e = co.emb[k][idx].to(dtype)
        x = co.h_all[:, k * E:(k + 1) * E].to(dtype) + torch.where(zero[:, None], torch.zeros_like(e), e)
        for l in range(L):
            qkv = lin(norm(x, co.norm1[l]), co.in_proj[l][k * 3 * E:(k + 1) * 3 * E], kE, 3)
            q, kk, v = qkv.view(B, 3, H, D).unbind(1)
            keys[l, k], vals[l, k] = kk, v
            vis = visible_steps(k, Q, co.ring_cap, co.context, defect)
            sc = torch.einsum("bhd,sbhd->bhs", q[..., :dl], keys[l, vis][..., :dl]) / math.sqrt(D)
            att = torch.einsum("bhs,sbhd->bhd", torch.softmax(sc, -1), vals[l, vis])
            if dl < D:
                att[..., dl:] = 0
            att = att.reshape(B, E)
            x = x + lin(att, co.out_proj[l][k * E:(k + 1) * E], kE, 1)
            uv = torch.cat([lin(norm(x, co.norm2[l]), half, kE, 3) for half in co.gate_in[l][k].view(2, Hd, E)], 1)
            hid = torch.nn.functional.silu(uv[:, :Hd]) * uv[:, Hd:]
            x = x + lin(hid, co.gate_out[l][k], kH, 1)
        lg = lin(x, co.heads[k], kE, 2)
        if co.head_bias[k] is not None and defect != "bias_ignored":
            lg = lg + co.head_bias[k].to(dtype)
        logits.append(lg)
        last = (qkv, att, hid, x)
    return Ref(torch.stack(logits), *last)


# ---- acceptance ---------------------------------------------------------------------------------------------------------------------------
TOL_FACTOR, TOL_FLOOR, TOL_CEIL = 16.0, 2.0 ** -18, 1e-3


def ratio(got, ref):
    """max |got - ref| / max |ref| of one vector; nan (compares false with every bound) where `got` is not finite."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    if not bool(torch.isfinite(got).all()):
        return float("nan")
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def ratios(got, ref, H):
    """The ratio of every vector the tests bound: each (step, row) of the logits `got` has, and per row of the hand-off vectors it
    has (None: not read) -- per head for the attention output."""
    out = {}
    for k in range(got.logits.shape[0]):
        for b in range(ref.logits.shape[1]):
            out[f"logits[step {k}, row {b}]"] = ratio(got.logits[k, b], ref.logits[k, b])
    for name in ("qkv", "hid", "x"):
        if getattr(got, name) is not None:
            for b in range(ref.x.shape[0]):
                out[f"{name}[row {b}]"] = ratio(getattr(got, name)[b], getattr(ref, name)[b])
    if got.att is not None:
        B, E = ref.att.shape
        ga, ra = got.att.reshape(B, H, E // H), ref.att.reshape(B, H, E // H)
        for b in range(B):
            for h in range(H):
                out[f"att[row {b}, head {h}]"] = ratio(ga[b, h], ra[b, h])
    return out


def worst(rs):
    name = max(rs, key=lambda n: float("inf") if rs[n] != rs[n] else rs[n])
    return name, rs[name]


def tolerance(ref32, ref64, H):
    """16 x the worst ratio of the fp32 run of the reference against its fp64 run, within [2^-18, 1e-3].  16: what legitimately
    differs from aten's fp32 (per-lane strided k order + wave reduction, four-partial norm sums, expf, 1 / sqrtf); the ceiling is
    the bound the real-shape test holds 8 steps x 6 layers to; the floor is 64 fp32 unit roundoffs."""
    return min(max(TOL_FACTOR * worst(ratios(ref32, ref64, H))[1], TOL_FLOOR), TOL_CEIL)


def accept(got, ref64, tol, H):
    """(every vector within tol, name of the worst vector, its ratio)."""
    rs = ratios(got, ref64, H)
    name, r = worst(rs)
    return all(v <= tol for v in rs.values()), name, r


# ---- the sampler readout: designed limits and noise --------------------------------------------------------------------------------------
def k_eff(card, top_k, limit):
    live = limit if 0 < limit < card else card
    return min(top_k if top_k > 0 else card, live)


def design_limits(case):
    return [(0, case.card - 1, case.card // 2)[k % 3] for k in range(case.Q)]


def read_rank(b, k, ke):
    return (3 * k + 5 * b + 1) % ke


def design_noise(case, limits, extra=0):
    """``[B, Q * top_k + extra]``: for row b and step k, 2^-40 at column k * top_k + read_rank(b, k) and 2^40 elsewhere."""
    noise = torch.full((case.B, case.Q * case.top_k + extra), HI)
    for b in range(case.B):
        for k in range(case.Q):
            noise[b, k * case.top_k + read_rank(b, k, k_eff(case.card, case.top_k, limits[k]))] = LO
    return noise


def ordered_ids(row, limit):
    """The ids below the limit by (logit descending, id ascending): the sampler's order at temperature 1."""
    live = limit if 0 < limit < row.numel() else row.numel()
    return torch.argsort(row[:live] + 0.0, descending=True, stable=True)


def expected_tokens(logits, case, limits):
    """``[B, Q]``: the read_rank(b, k)-th id of step k's logits among the ids below the step's limit, and the distance of its logit
    from the row maximum (the design is valid within 50: exp(-50) > 2^-80)."""
    tok = torch.zeros(case.B, case.Q, dtype=torch.long)
    gap = torch.zeros(case.B, case.Q)
    for b in range(case.B):
        for k in range(case.Q):
            row = logits[k, b].float()
            t = ordered_ids(row, limits[k])[read_rank(b, k, k_eff(case.card, case.top_k, limits[k]))]
            tok[b, k], gap[b, k] = t, row.max() - row[t]
    return tok, gap


def emulate_sampler(logits, noise, limits, case, defect=None):
    """The launch's use of its sampler in torch, per (row, step): noise columns k * top_k .., the row of b, the limit of step k; the
    winner is the first maximum of p / noise over the top-k of the ids below the limit.  `defect`: one of SAMPLER_DEFECTS."""
    tok = torch.zeros(case.B, case.Q, dtype=torch.long)
    for b in range(case.B):
        for k in range(case.Q):
            kn = 0 if defect == "noise_step0" else k
            bn = 0 if defect == "noise_row0" else b
            lim = limits[0 if defect == "limit_step0" else k]
            row = logits[k, b].float()
            order = ordered_ids(row, lim)[:k_eff(case.card, case.top_k, lim)]
            p = torch.softmax(row.double(), -1)[order]
            nz = noise[bn, kn * case.top_k:kn * case.top_k + order.numel()].double()
            tok[b, k] = order[(p / nz).argmax()]
    return tok


# ---- the hand-off workspace ---------------------------------------------------------------------------------------------------------------
def workspace(ops, B, E, Hd, card):
    """The eager workspace ops.depth_decode_frame launched a shape on (int64 granules)."""
    return ops.frame_workspace("depth_frame", (B, E, Hd, card))


def read_handoff(ws, case, B, solo=False):
    """The fp32 value (low word) of every {tag, value} granule of gX | gQKV | gATT | gH | gLOG | gTOK (csrc/lm_depth.hip) as CPU tensors
    ``X [B, E], QKV [B, 3E], ATT [B, E], H [B, Hd], LOG [B, card]`` and ``TOK [B]`` (int32: the token's bits ride in the value word).
    ``case``: anything with E, Hd, card.  ``solo``: the repair launch's own set, behind the persistent launch's."""
    E, Hd, card = case.E, case.Hd, case.card
    n = B * (5 * E + Hd + card + 1)
    low = ws[n if solo else 0:(2 * n if solo else n)].view(torch.int32).view(-1, 2)[:, 0].contiguous().cpu()
    out, off = {}, 0
    for name, width in (("X", E), ("QKV", 3 * E), ("ATT", E), ("H", Hd), ("LOG", card)):
        out[name] = low[off:off + B * width].view(torch.float32).view(B, width)
        off += B * width
    out["TOK"] = low[off:off + B]
    return SimpleNamespace(**out)


# ---- device side: pointer tables ----------------------------------------------------------------------------------------------------------
def device_tables(co, dev):
    """The operands on the device (bf16 weights, fp32 gains / bias / h_all) and the ``DepthFrameTables`` of the full frame, built by the
    product's own class from a stand-in for the per-step-weights transformer."""
    from rstnet_amd.lm.depth_frame import DepthFrameTables
    c = co.case

    def bf(t):
        return t.to(dev, torch.bfloat16).contiguous()

    def f32(t):
        return None if t is None else t.to(dev, torch.float32).contiguous()

    def norm(a):
        a = f32(a)
        return SimpleNamespace(alpha_f32=lambda: a, eps=co.eps)
    layers = []
    for l in range(c.L):
        gating = [SimpleNamespace(linear_in=SimpleNamespace(weight=bf(co.gate_in[l][k])), linear_out=SimpleNamespace(weight=bf(co.gate_out[l][k])))
                  for k in range(c.Q)]
        layers.append(SimpleNamespace(self_attn=SimpleNamespace(in_proj_weight=bf(co.in_proj[l]), out_proj=SimpleNamespace(weight=bf(co.out_proj[l]))),
                                      norm1=norm(co.norm1[l]), norm2=norm(co.norm2[l]), gating=gating))
    dep = SimpleNamespace(layers=layers, weights_per_step=c.Q, d_model=c.E, num_heads=c.H, context=c.context)
    d = SimpleNamespace(case=c, co=co, dep=dep, heads=[bf(h) for h in co.heads], head_bias=[f32(b) for b in co.head_bias],
                        emb=[bf(e) for e in co.emb], h_all=f32(co.h_all), text=co.text.to(dev))
    d.full = DepthFrameTables(dep, d.heads, d.head_bias, d.emb)
    return d


class PrefixTables:
    """Pointer tables of the first q steps of ``d.full``'s frame: the in / out projections keep their base pointers (their layout is
    step-major), the gating tables are re-flattened as l * q + k, heads / bias / embeddings are cut to q; a status tensor of its own."""

    def __init__(self, d, q):
        from rstnet_amd import ops
        t, c = d.full, d.case
        assert 1 <= q <= c.Q
        self.L, self.dep_q, self.E, self.H, self.Hd, self.card = t.L, q, t.E, t.H, t.Hd, t.card
        self.in_proj, self.out_proj, self.norm1, self.norm2 = t.in_proj, t.out_proj, t.norm1, t.norm2

        def cut(arr, index):
            return (C.c_void_p * len(index))(*[arr[i] for i in index])
        gates = [l * c.Q + k for l in range(c.L) for k in range(q)]
        self.gate_in, self.gate_out = cut(t.gate_in, gates), cut(t.gate_out, gates)
        self.heads, self.emb = cut(t.heads, range(q)), cut(t.emb, range(q))
        self.head_bias = None if t.head_bias is None else cut(t.head_bias, range(q))
        self.emb_rows = (C.c_int * q)(*list(t.emb_rows)[:q])
        self.eps, self.context = t.eps, t.context
        self.status = ops.new_persistent_status(d.h_all.device)
        self._keep = d


def prefix_tables(d, q):
    return PrefixTables(d, q)


def launch(d, tables, *, noise=None, limits=None, tok_pad=0, status_code=0):
    """One frame through ops.depth_decode_frame on fresh tokens ``[B, dep_q + 1 + tok_pad]`` (column 0: the text token; -7 elsewhere), with
    the ring capacity of the full case; sampling at temperature 1 when ``noise`` is given.  ``status_code``: planted in status[0]
    first, so that the repair launch behind the persistent one recomputes the frame.  Returns the token matrix on the CPU."""
    from rstnet_amd import ops
    c, q = d.case, tables.dep_q
    tokens = torch.full((c.B, q + 1 + tok_pad), -7, dtype=torch.long, device=d.h_all.device)
    tokens[:, 0] = d.text
    if status_code:
        tables.status[0] = status_code
    ops.depth_decode_frame(tables, d.h_all[:, :q * c.E].contiguous() if q < c.Q else d.h_all, tokens, noise, use_sampling=noise is not None, temp=1.0,
                           top_k=c.top_k, eps=d.co.eps, context=c.context, limits=limits, ring_cap=c.ring_cap)
    torch.cuda.synchronize()
    return tokens.cpu()
