"""Host side of the per-stream adapter bank (GPT.load_adapter_bank / set_adapter_ids), no GPU: the stacked kernel-form tensors equal
what a single-adapter ``merge_lora=False`` model builds for every set, the refusals, and the error bounds of tests/helpers/lora_bank.py
held against a plain fp32 emulation of the two launches and against four planted defects."""
import pytest
import torch

from rstnet_amd import ops, synth
from rstnet_amd.lm.generate import GPTGen
from rstnet_amd.lm.gpt import GPT, Config
from tests.golden import cases
from tests.helpers import gemv_bounds as GB
from tests.helpers import lora_bank as LB


def _unmerged(cfg_d, adapters=None):
    sd = {**{k: v.clone() for k, v in LB.base_sd(cfg_d).items()}, **(adapters or {})}
    return GPT.from_state_dict(sd, Config.from_dict(cfg_d), merge_lora=False)


@pytest.mark.parametrize("name", ["gqa", "gqa_qkv_alpha6"])
def test_bank_slices_equal_the_single_adapter_forms(name):
    cfg_d = LB.CFGS[name]
    sets = LB.adapter_sets(cfg_d)
    model = _unmerged(cfg_d)                       # a state dict without adapters of its own
    assert model.adapter_bank() is None
    model.load_adapter_bank(sets)
    bank = model.adapter_bank()
    L = cfg_d["n_layer"]
    assert sorted(bank) == sorted(["lm_head"] + [f"transformer.h.{l}.{m}" for l in range(L) for m in ("attn.attn", "attn.proj", "mlp.fc", "mlp.proj")])
    for n, ad in enumerate(sets):
        single = _unmerged(cfg_d, ad)
        want = {"lm_head": single.lm_head.adapter()}
        for l, blk in enumerate(single.transformer.h):
            p = f"transformer.h.{l}"
            want.update({f"{p}.attn.attn": blk.attn.packed_qkv_adapter(), f"{p}.attn.proj": blk.attn.proj.adapter(),
                         f"{p}.mlp.fc": blk.mlp.packed_fc_adapter(), f"{p}.mlp.proj": blk.mlp.proj.adapter()})
        for key, (A, Bm, scale) in want.items():
            Ab, Bb, sb = bank[key]
            assert Ab.dtype == torch.bfloat16 and Bb.dtype == torch.bfloat16 and Ab.shape[0] == len(sets) and Ab.shape[1] % 16 == 0
            assert torch.equal(Ab[n], A) and torch.equal(Bb[n], Bm) and sb == scale, (key, n)
    # the scale: alpha / r = 2 is folded into B exactly, 6 / 4 = 1.5 is applied to A x
    assert bank["lm_head"][2] == (1.0 if name == "gqa" else 1.5)
    # every view holds the model's one id vector; without set_adapter_ids every row is -1
    model._bank_rows(3)
    views = [v for blk in model.transformer.h for v in blk.bank.values()] + [model._head_bank]
    assert all(v.ids is model._bank_ids for v in views) and model._bank_ids.tolist() == [-1, -1, -1]
    assert model._bank_ids.dtype == torch.int32
    model.set_adapter_ids([2, -1, 0])
    assert all(v.ids is model._bank_ids for v in views) and model._bank_ids.tolist() == [2, -1, 0]      # in place
    model.set_adapter_ids(torch.tensor([1, 1]))
    assert model._bank_ids.tolist() == [1, 1] and model._head_bank.ids is model._bank_ids
    model.load_adapter_bank(None)
    assert model.adapter_bank() is None and all(blk.bank is None for blk in model.transformer.h)


def test_a_set_that_lacks_a_linear_gets_zero_blocks():
    cfg_d = LB.CFGS["gqa"]
    sets = LB.adapter_sets(cfg_d)
    lacking = {k: v for k, v in sets[1].items() if ".mlp.fc_2." not in k and not k.startswith("lm_head")}
    model = _unmerged(cfg_d, sets[0])              # a model with adapters of its own
    model.load_adapter_bank([sets[0], lacking])
    bank, full = model.adapter_bank(), _unmerged(cfg_d, sets[1])
    r = cfg_d["lora_r"]
    A, Bm, _ = full.transformer.h[1].mlp.packed_fc_adapter()
    Ab, Bb, _ = bank["transformer.h.1.mlp.fc"]
    assert torch.equal(Ab[1, :r], A[:r]) and not Ab[1, r:].any() and torch.equal(Bb[1, :, :r], Bm[:, :r]) and not Bb[1, :, r:].any()
    assert not bank["lm_head"][0][1].any() and not bank["lm_head"][1][1].any() and bank["lm_head"][0][0].any()
    model.load_adapter_bank(None)                  # back to the model's own set
    assert model.transformer.h[0].view().qkv.lora is model.transformer.h[0].attn.packed_qkv_adapter()


def test_refusals():
    cfg_d = LB.CFGS["gqa"]
    sets = LB.adapter_sets(cfg_d)
    with pytest.raises(RuntimeError, match="merge_lora=False"):
        GPT.from_state_dict({**LB.base_sd(cfg_d), **sets[0]}, Config.from_dict(cfg_d)).load_adapter_bank(sets)
    model = _unmerged(cfg_d)
    with pytest.raises(RuntimeError, match="no adapter bank"):
        model.set_adapter_ids([0])
    key = "transformer.h.0.attn.proj"
    wrong_rank = {**sets[0], f"{key}.lora_A": torch.zeros(cfg_d["lora_r"] + 1, cfg_d["n_embd"]), f"{key}.lora_B": torch.zeros(cfg_d["n_embd"], cfg_d["lora_r"] + 1)}
    with pytest.raises(RuntimeError, match="do not fit r="):
        model.load_adapter_bank([sets[0], wrong_rank])
    with pytest.raises(RuntimeError, match="come as a pair"):
        model.load_adapter_bank([{k: v for k, v in sets[0].items() if k != f"{key}.lora_B"}])
    mha = _unmerged(LB.CFGS["mha"])                # attn.proj is not adapted there
    with pytest.raises(RuntimeError, match="does not adapt"):
        mha.load_adapter_bank([{**LB.adapter_sets(LB.CFGS["mha"])[0], f"{key}.lora_A": sets[0][f"{key}.lora_A"], f"{key}.lora_B": sets[0][f"{key}.lora_B"]}])
    with pytest.raises(ValueError, match="1 to 256"):
        model.load_adapter_bank([sets[0]] * 257)
    with pytest.raises(ValueError, match="1 to 256"):
        model.load_adapter_bank([])
    assert model.adapter_bank() is None            # nothing was installed by a refused call
    model.load_adapter_bank(sets)
    with pytest.raises(ValueError, match=r"\[-1, 3\)"):
        model.set_adapter_ids([0, 3])
    with pytest.raises(ValueError, match=r"\[-1, 3\)"):
        model.set_adapter_ids(torch.tensor([-2, 0]))
    with pytest.raises(ValueError, match="vector of integers"):
        model.set_adapter_ids(torch.tensor([0.0, 1.0]))
    model.set_adapter_ids([0, 1])
    toks = cases.gpt_tokens(cfg_d, steps=3, batch=3)
    with pytest.raises(ValueError, match="batch size 3 differs from the 2 ids"):
        model.forward_global(toks)
    with pytest.raises(ValueError, match="batch size 3 differs from the 2 ids"):
        model.forward(toks)
    with pytest.raises(ValueError, match="batch size 3 differs from the 2 ids"):
        with model.streaming(3):
            pass
    gen = GPTGen(model, use_sampling=False)
    with pytest.raises(ValueError, match=r"\[-1, 3\)"):
        gen.begin(2, adapter_ids=[0, 7])
    assert model.transformer._streaming_state is None
    with model.streaming(2):
        with pytest.raises(RuntimeError, match="between sessions"):
            model.load_adapter_bank(None)
        with pytest.raises(RuntimeError, match="between sessions"):
            model.load_adapter_bank(sets)
        with pytest.raises(RuntimeError, match="another batch size"):
            model.set_adapter_ids([0, 1, 2])
        model.set_adapter_ids([2, -1])             # same B: in place
    assert model._bank_ids.tolist() == [2, -1]


def test_unsupported_shape_is_refused_before_any_tensor_is_built(monkeypatch):
    cfg_d = LB.CFGS["gqa"]
    model = _unmerged(cfg_d)
    assert ops.lora_bank_supported(256, 16, 320) and ops.lora_bank_supported(16384, 256, 1)
    for K, r, N in [(260, 16, 8), (16392, 16, 8), (256, 24, 8), (256, 272, 8), (256, 16, 0), (0, 16, 8), (256, 0, 8)]:
        assert not ops.lora_bank_supported(K, r, N), (K, r, N)
    monkeypatch.setattr(ops, "lora_bank_supported", lambda K, r, N: N != 320)      # (the head: N = padded_vocab_size)
    built = []
    monkeypatch.setattr(torch, "stack", lambda *a, **k: built.append(1))
    with pytest.raises(ValueError, match="lm_head .* outside the adapter-bank kernels"):
        model.load_adapter_bank(LB.adapter_sets(cfg_d))
    assert not built and model.adapter_bank() is None


def test_cpu_tensors_are_refused():
    A, Bm = LB.bank_operands(2, 16, 64, 8)
    ids = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.lora_bank_shrink(torch.zeros(2, 64), A, ids)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.lora_bank_expand(torch.zeros(2, 16), Bm, ids, torch.zeros(2, 8))


# ---- the bounds -------------------------------------------------------------------------------------------------------------------------
def _case(K, r, N, prologue, rows=6, rows_per_id=1, seed=0):
    g = torch.Generator().manual_seed(seed)
    A, Bm = LB.bank_operands(3, r, K, N, seed)
    x = GB.mixed_rows(rows, 2 * K if prologue == 2 else K, g)
    alpha = 1 + 0.1 * torch.randn(K, generator=g) if prologue == 1 else None
    ids = torch.tensor([0, 1, 2, -1, 1, 0][: rows // rows_per_id], dtype=torch.int32)
    y = GB.mixed_rows(rows, N, g, -4, 4)
    return A, Bm, x, alpha, ids, y


@pytest.mark.parametrize("prologue", [0, 1, 2])
@pytest.mark.parametrize("K,r", [(64, 16), (520, 96), (1024, 32)])
def test_bounds_pass_plain_fp32_and_fail_the_planted_defects(K, r, prologue):
    N, ps = 50, 0.1875
    A, Bm, x, alpha, ids, y = _case(K, r, N, prologue)
    kw = dict(prologue=prologue, alpha=alpha, post_scale=ps)
    a64, ba = LB.shrink_ref(x, A, ids, **kw)
    a = LB.emul_shrink(x, A, ids, **kw)
    assert LB.worst(a, a64, ba) <= 1.0
    assert not a[3].any() and not ba[3].any()                     # the base-model row: zeros, no tolerance
    y64, by = LB.expand_ref(a, Bm, ids, y)
    got = LB.emul_expand(a, Bm, ids, y)
    assert LB.worst(got, y64, by) <= 1.0 and torch.equal(got[3], y[3])
    # carried through both launches: the reference on the fp64 a, the shrink's bound as the input error
    y64c, byc = LB.expand_ref(a64.float(), Bm, ids, y, da=ba + LB.U * a64.abs())
    assert LB.worst(got, y64c, byc) <= 1.0
    # planted defects
    assert LB.worst(LB.emul_shrink(x, A, ids, **kw, neighbour=True), a64, ba) > 1.0
    assert LB.worst(LB.emul_shrink(x, A, ids, **kw, no_post_scale=True), a64, ba) > 1.0
    if prologue:
        assert LB.worst(LB.emul_shrink(x, A, ids, **kw, skip_prologue=True), a64, ba) > 1.0
    assert LB.worst(LB.emul_expand(a, Bm, ids, y, neighbour=True), y64, by) > 1.0
    assert LB.worst(LB.emul_expand(a, Bm, ids, y, drop_last_block=True), y64, by) > 1.0


def test_bound_constants():
    assert LB.c_shrink(64) == 16 and LB.c_shrink(520) == 24 and LB.c_shrink(11264) == 8 * 22 + 8 and LB.c_expand(96) == 98


def test_rows_per_id_lays_rows_out_stream_major():
    ids = torch.tensor([2, -1, 0], dtype=torch.int32)
    assert LB.row_ids(ids, 6, 2).tolist() == [2, 2, -1, -1, 0, 0]
    A, _, x, _, _, _ = _case(64, 16, 8, 0, rows=6)
    a = LB.emul_shrink(x, A, ids, rows_per_id=2)
    assert not a[2:4].any() and a[:2].any() and a[4:].any()
