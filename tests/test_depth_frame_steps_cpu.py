"""tests/helpers/depth_frame_ref.py checked without a GPU: the case table of tests/test_depth_frame_steps_gpu.py turns every loop of the
persistent depth-frame launch (csrc/lm_depth.hip) at both batch sizes, the dtype-generic reference agrees with oracle/lm_oracle.py,
its ring map is RingKV.complete's, and the acceptance function of the GPU test rejects every defect the cases are there to find."""
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import lm_oracle as L
from rstnet_amd import synth
from tests.helpers import depth_frame_ref as R


def test_the_cases_turn_every_loop_at_both_batch_sizes():
    seen = {1: set(), 2: set()}
    for c in R.CASES:
        g = R.grid(c, 256)
        assert g.ok, f"{c.name}: not a shape the launcher serves (G {g.G}, LDS {g.lds})"
        assert -(-min(3 * c.E, c.Hd, c.card) // 4) <= 128, f"{c.name}: the grid would depend on the CU count"
        assert g.flags == R.grid(c, 128).flags == R.grid(c, 304).flags
        assert len(c.text) == c.B
        seen[c.B] |= g.flags
    for B in (1, 2):
        assert not set(R.FLAGS) - seen[B], f"batch {B}: no case for {sorted(set(R.FLAGS) - seen[B])}"
    assert set(R.REPAIR_CASES) <= set(R.BY_NAME) and {R.BY_NAME[n].B for n in R.REPAIR_CASES} == {1, 2}
    # a device with fewer CUs than a case's grid changes the paths, and `grid` says so (the GPU test asserts on it)
    assert R.grid(R.BY_NAME["idle-B1"], 16).flags != R.grid(R.BY_NAME["idle-B1"], 256).flags


def test_the_named_shapes_take_the_paths_the_kernel_comments_promise():
    g = R.grid(R.BY_NAME["rows-B1"], 256)
    assert (g.G, g.W) == (10, 40) and {"rows2_in", "rows2_gate", "rows2_out", "k_partial", "card37", "topk_ge_card"} <= g.flags
    g = R.grid(R.BY_NAME["headrows-B2"], 256)
    assert (g.G, g.W) == (10, 40) and "rows2_head" in g.flags
    moshi = R.Case("moshi", 1, 1024, 16, 2816, 2048, 8, 6, 250, 8, None, False, ("ok",))
    g = R.grid(moshi, 256)
    assert g.ok and g.G == 256 and not g.flags & {"rows2_in", "rows2_gate", "rows2_out", "rows2_head", "idle_waves", "k_partial", "k2_E", "k2_Hd",
                                                  "norm_tail", "lds_big", "s16"}
    assert R.grid(R.BY_NAME["wide-B2"], 256).lds > 64 * 1024 >= R.grid(R.BY_NAME["wide-B1"], 256).lds


def test_reference_in_fp32_is_the_oracle_at_the_tiny_depth_shape():
    cfg = synth.LM_TINY
    sd = {k: v.float() for k, v in synth.lm_state_dict(cfg, seed=11).items()}
    ocfg = L.LMConfig(**cfg)
    B, Q, E, nl = 2, cfg["dep_q"], cfg["depformer_dim"], cfg["depformer_num_layers"]
    Hd = sd["depformer.layers.0.gating.0.linear_out.weight"].shape[1]
    g = torch.Generator().manual_seed(5)
    h = torch.randn(B, cfg["dim"], generator=g)
    tokens = torch.stack([torch.tensor([-1, 7]), torch.randint(0, cfg["card"], (B,), generator=g)], 1)          # [B, Q]: text (one -1), step 0's token
    case = R.Case("tiny", B, E, cfg["depformer_num_heads"], Hd, cfg["card"], Q, nl, 0, Q, None, False, ("neg1", "ok"))
    p = "depformer.layers"
    co = R.SimpleNamespace(
        case=case, eps=float(torch.tensor(1e-8, dtype=torch.float32)), ring_cap=Q, context=None,
        in_proj=[sd[f"{p}.{l}.self_attn.in_proj_weight"] for l in range(nl)], out_proj=[sd[f"{p}.{l}.self_attn.out_proj.weight"] for l in range(nl)],
        norm1=[sd[f"{p}.{l}.norm1.alpha"].view(-1) for l in range(nl)], norm2=[sd[f"{p}.{l}.norm2.alpha"].view(-1) for l in range(nl)],
        gate_in=[[sd[f"{p}.{l}.gating.{k}.linear_in.weight"] for k in range(Q)] for l in range(nl)],
        gate_out=[[sd[f"{p}.{l}.gating.{k}.linear_out.weight"] for k in range(Q)] for l in range(nl)],
        heads=[sd[f"linears.{k}.weight"] for k in range(Q)], head_bias=[None] * Q,
        emb=[sd["depformer_text_emb.weight"]] + [sd[f"depformer_emb.{k}.weight"] for k in range(Q - 1)],
        h_all=torch.cat([F.linear(h, sd[f"depformer_in.{k}.weight"]) for k in range(Q)], 1))
    st = L.new_transformer_state(B, nl, case.H, E // case.H, Q)
    want = torch.stack([L.forward_depformer(sd, ocfg, k, tokens[:, k, None, None], h[:, None], st)[:, 0, 0] for k in range(Q)])
    got = R.reference(co, tokens, dtype=torch.float32)
    for k in range(Q):
        for b in range(B):
            assert R.ratio(got.logits[k, b], want[k, b]) < 1e-5, (k, b)
    assert R.reference(co, tokens).logits.dtype == torch.float64


def test_ring_map_is_ringkv_complete_with_the_streaming_mask():
    combos = {(c.ring_cap, c.context, c.Q) for c in R.CASES} | {(8, None, 8), (9, None, 8), (8, 2, 8), (4, 3, 4)}
    for cap, context, Q in sorted(combos, key=str):
        ring = L.RingKV(1, 1, 1, cap)
        for k in range(Q):
            _, _, pos_k = ring.complete(torch.zeros(1, 1, 1, 1), torch.zeros(1, 1, 1, 1))
            delta = k - pos_k
            mask = (pos_k >= 0) & (delta >= 0)
            if context is not None:
                mask = mask & (delta < context)
            want = [s for s in range(cap) if bool(mask[s])]
            assert R.visible_steps(k, Q, cap, context) == want, (cap, context, Q, k)
    # the slot that hides step 0 at the last step of a ring of dep_q slots
    assert R.visible_steps(2, 3, 3, None) == [1, 2] and R.visible_steps(2, 3, 4, None) == [0, 1, 2]


@functools.lru_cache(maxsize=None)
def _refs(name):
    """Operands, a teacher-forcing token matrix that takes the embedding's three branches at later steps too, the fp64 and fp32
    references and the case's tolerance."""
    c = R.BY_NAME[name]
    co = R.make_case(c)
    g = torch.Generator().manual_seed(17)
    tokens = torch.cat([co.text[:, None], torch.randint(0, c.card, (c.B, c.Q), generator=g)], 1)
    ref64, ref32 = R.reference(co, tokens), R.reference(co, tokens, dtype=torch.float32)
    return co, tokens, ref64, ref32, R.tolerance(ref32, ref64, c.H)


# defect -> cases whose flag it belongs to (every defect at both batch sizes where the table has both)
DEFECT_CASES = {
    "last_row_block": ("rows-B1", "headrows-B2"),
    "k_tail_E": ("e1088-B2", "e1088-B1"),
    "k_tail_Hd": ("hd3080-B1", "hd3080-B2"),
    "norm_tail": ("wide-B1",),
    "head_dims": ("d192-B2", "wide-B1"),
    "hidden_slot": ("rows-B2", "idle-B1"),
    "context_ignored": ("d24-B1", "heads16-B2"),
    "ring_cap_as_Q": ("headrows-B1", "hd3080-B2"),
    "bias_ignored": ("rows-B1", "d24-B2"),
    "neg1_not_zeroed": ("rows-B1", "idle-B2"),
    "unclamped_row0": ("headrows-B1", "rows-B2"),
}


def test_every_defect_has_cases():
    assert set(DEFECT_CASES) == set(R.DEFECTS)


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_acceptance_rejects_the_defect(defect):
    for name in DEFECT_CASES[defect]:
        co, tokens, ref64, _, tol = _refs(name)
        bad = R.reference(co, tokens, defect=defect)
        ok, where, r = R.accept(bad, ref64, tol, co.case.H)
        assert not ok, f"{defect} on {name}: worst {where} {r:.3e} passes tol {tol:.3e}"
        # and through the logits alone, which is all a prefix launch shows of the steps before the last
        ok, where, r = R.accept(bad._replace(qkv=None, att=None, hid=None, x=None), ref64, tol, co.case.H)
        assert not ok, f"{defect} on {name}: logits worst {where} {r:.3e} pass tol {tol:.3e}"


@pytest.mark.parametrize("name", ["rows-B1", "headrows-B2", "idle-B2", "heads16-B1", "d24-B2", "d192-B1", "e1088-B1", "hd3080-B2", "hd16392-B1"])
def test_clean_fp32_reference_is_accepted(name):
    co, _, ref64, ref32, tol = _refs(name)
    assert R.TOL_FLOOR <= tol <= R.TOL_CEIL
    ok, where, r = R.accept(ref32, ref64, tol, co.case.H)
    assert ok, f"{name}: {where} {r:.3e} vs tol {tol:.3e}"
    nan = ref32._replace(logits=ref32.logits.clone())
    nan.logits[0, 0, 0] = float("nan")
    assert not R.accept(nan, ref64, tol, co.case.H)[0]


@pytest.mark.parametrize("name", ["rows-B2", "headrows-B2", "heads16-B2", "d24-B2", "idle-B1"])
def test_sampler_readout_design_and_its_defects(name):
    co, _, ref64, _, _ = _refs(name)
    c = co.case
    limits = R.design_limits(c)
    co = R.make_case(c, limits=limits)
    logits = R.reference(co, _refs(name)[1]).logits
    want, gap = R.expected_tokens(logits, c, limits)
    assert float(gap.max()) < 50
    for k, lim in enumerate(limits):          # the +8 lifts the first blanked id above the rank read: a sampler that let it race would read another id
        for b in range(c.B):
            if 0 < lim < c.card:
                assert logits[k, b, lim] > logits[k, b, want[b, k]], (k, b)
    for extra in (0, 3):
        noise = R.design_noise(c, limits, extra)
        assert noise.shape == (c.B, c.Q * c.top_k + extra)
        assert torch.equal(R.emulate_sampler(logits, noise, limits, c), want)
    noise = R.design_noise(c, limits)
    for defect in R.SAMPLER_DEFECTS:
        if defect == "noise_row0" and c.B == 1:
            continue
        assert not torch.equal(R.emulate_sampler(logits, noise, limits, c, defect), want), defect
