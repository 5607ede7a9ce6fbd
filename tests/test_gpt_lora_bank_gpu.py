"""``GPT.load_adapter_bank`` / ``set_adapter_ids`` on the GPU: every stream of a batch with its own LoRA adapter set from one copy of the
base weights (csrc/lm_lora_bank.hip behind ``lm.stack._lora_add``).  Tiny ``gqa`` / ``mha`` configs, ONE base and the adapter tensors of
``synth.gpt_state_dict`` seeds 21 / 22 / 23 (tests/helpers/lora_bank.py).  Row ``b`` of a mixed batch is held to (i) the existing
single-adapter ``merge_lora=False`` model of its set (the ``lora_r = 0`` base for -1) fed the same batch, and (ii) the oracle's unmerged
path fed that row alone, at the 1e-3 of tests/test_gpt_gpu.py; and, the kernels' summation schedule being independent of the batch, to
the SAME BITS as the same call under uniform ids."""
import functools

import pytest
import torch

from oracle import gpt_oracle as Gp
from rstnet_amd.lm.generate import GPTGen
from rstnet_amd.lm.gpt import GPT, Config
from tests.golden import cases
from tests.helpers import lora_bank as LB

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-3
MIXED = {5: [0, 2, -1, 1, 0], 2: [1, -1]}      # B = 2 takes the weight-streaming base products, B = 5 the matrix-core ones


def rel_err(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@functools.lru_cache(maxsize=None)
def fixtures(name):
    """(cfg_d, base state dict, adapter sets) on the device -- shared and never modified (models are built on clones)."""
    cfg_d = LB.CFGS[name]
    return cfg_d, {k: v.to(DEV) for k, v in LB.base_sd(cfg_d).items()}, [{k: v.to(DEV) for k, v in s.items()} for s in LB.adapter_sets(cfg_d)]


def bank_model(name, own=None, **cfg_extra):
    cfg_d, base, sets = fixtures(name)
    sd = {**{k: v.clone() for k, v in base.items()}, **({} if own is None else sets[own])}
    model = GPT.from_state_dict(sd, Config.from_dict({**cfg_d, **cfg_extra}), merge_lora=False)
    model.load_adapter_bank(sets)
    return model


def single_model(name, k, **cfg_extra):
    """The existing route: one adapter set per model instance (k = -1: the base model, no LoRA at all)."""
    cfg_d, base, sets = fixtures(name)
    if k < 0:
        return GPT.from_state_dict({n: v.clone() for n, v in base.items()}, Config.from_dict({**cfg_d, **cfg_extra, "lora_r": 0}))
    return GPT.from_state_dict({**{n: v.clone() for n, v in base.items()}, **sets[k]}, Config.from_dict({**cfg_d, **cfg_extra}), merge_lora=False)


def oracle_of(name, k):
    cfg_d, base, sets = fixtures(name)
    keep = set(Gp.GPTConfig.__dataclass_fields__)
    ocfg = Gp.GPTConfig(**{n: v for n, v in {**cfg_d, **({"lora_r": 0} if k < 0 else {})}.items() if n in keep})
    return {n: v.float().cpu() for n, v in {**base, **({} if k < 0 else sets[k])}.items()}, ocfg


def run_model(model, toks, ids=None):
    """(h, logits) of the full-sequence pass over the first GPT_T_FULL positions, then of every graph-replayed T = 1 step across the wrap."""
    B = toks.shape[0]
    if ids is not None:
        model.set_adapter_ids(ids)
    full = model.forward_global(toks[:, :, :cases.GPT_T_FULL].to(DEV))
    steps = []
    with model.streaming(B):
        for t in range(cases.GPT_STEPS):
            h, lg = model.forward_global(toks[:, :, t:t + 1].to(DEV))
            steps.append((h.clone(), lg.clone()))
    return full, steps


@functools.lru_cache(maxsize=None)
def mixed_run(name, B):
    cfg_d = fixtures(name)[0]
    toks = cases.gpt_tokens(cfg_d, steps=cases.GPT_STEPS, batch=B)
    return toks, run_model(bank_model(name), toks, MIXED[B])


@pytest.mark.parametrize("B", [5, 2])
@pytest.mark.parametrize("name", ["gqa", "mha"])
def test_mixed_batch_against_the_single_adapter_route_and_the_oracle(name, B):
    toks, (full, steps) = mixed_run(name, B)
    ids = MIXED[B]
    for k in sorted(set(ids)):
        rows = [b for b in range(B) if ids[b] == k]
        full_r, steps_r = run_model(single_model(name, k), toks)                  # (i) the existing route, fed the same batch
        for got, ref in [(full, full_r)] + list(zip(steps, steps_r)):
            for b in rows:
                assert rel_err(got[0][b], ref[0][b]) < TOL and rel_err(got[1][b], ref[1][b]) < TOL, (k, b)
        osd, ocfg = oracle_of(name, k)                                            # (ii) the oracle's unmerged path, that row alone
        for b in rows:
            with torch.no_grad():
                h_o, lg_o = Gp.forward_global(osd, ocfg, toks[b:b + 1, :, :cases.GPT_T_FULL])
                assert rel_err(full[0][b], h_o[0]) < TOL and rel_err(full[1][b], lg_o[0]) < TOL, (k, b)
                st = Gp.new_global_state(ocfg, 1)
                for t in range(cases.GPT_STEPS):
                    h_o, lg_o = Gp.forward_global(osd, ocfg, toks[b:b + 1, :, t:t + 1], st)
                    assert rel_err(steps[t][0][b], h_o[0]) < TOL and rel_err(steps[t][1][b], lg_o[0]) < TOL, (k, b, t)
    # the adapters matter: rows 0 and 4 of the B = 5 batch share a set but not their tokens; sets differ by far more than the tolerance
    if B == 5:
        other = run_model(bank_model(name), toks, [1, 2, -1, 1, 0])[0]
        assert rel_err(other[1][0], full[1][0]) > 10 * TOL and torch.equal(other[1][1:], full[1][1:])


@pytest.mark.parametrize("name", ["gqa", "mha"])
def test_a_row_has_the_same_bits_under_uniform_ids(name):
    B = 5
    toks, (full, steps) = mixed_run(name, B)
    model = bank_model(name)
    for k in sorted(set(MIXED[B])):
        full_u, steps_u = run_model(model, toks, [k] * B)
        for b in [b for b in range(B) if MIXED[B][b] == k]:
            assert torch.equal(full_u[0][b], full[0][b]) and torch.equal(full_u[1][b], full[1][b]), (k, b)
            for t in range(cases.GPT_STEPS):
                assert torch.equal(steps_u[t][0][b], steps[t][0][b]) and torch.equal(steps_u[t][1][b], steps[t][1][b]), (k, b, t)


def test_greedy_token_streams_do_not_depend_on_the_other_rows():
    """``GPTGen`` greedy, 12 frames behind a 6-position prefill (the ring of context + 1 = 11 slots wraps): row b under mixed ids draws the
    tokens it draws under uniform ``ids[b]`` -- the logits are bit-identical, so there is no tie to break differently."""
    name, B = "gqa", 5
    cfg_d = fixtures(name)[0]
    model = bank_model(name)
    n_codes = cfg_d["audio_card"] - 2
    prompt = torch.randint(0, n_codes, (B, cfg_d["n_q"] + 1, 6), generator=torch.Generator().manual_seed(3)).to(DEV)

    def run(ids):
        gen = GPTGen(model, use_sampling=False, n_audio_codes=n_codes)
        gen.begin(B, adapter_ids=ids)
        frames = []
        try:
            h, logits = gen.prefill(prompt)
            text, audio = gen.start(h, logits, 0)
            frames.append(torch.cat([text[:, None], audio], 1).clone())
            for _ in range(11):
                text, audio = gen.step()
                frames.append(torch.cat([text[:, None], audio], 1).clone())
        finally:
            gen.end()
        return torch.stack(frames, 1).cpu()                     # [B, 12, 1 + dep_q]

    mixed = run(MIXED[B])
    streams = {k: run([k] * B) for k in sorted(set(MIXED[B]))}
    for b, k in enumerate(MIXED[B]):
        assert torch.equal(mixed[b], streams[k][b]), b
    assert not torch.equal(streams[0], streams[1])              # the sets draw different streams


def test_ids_changed_under_a_captured_graph(monkeypatch):
    """After 3 steps (warm-up, capture + replay, replay) ``set_adapter_ids`` writes other ids into the SAME device vector: the next replay
    reads them.  Reference: a fresh eager session brought to the same state under the old ids, switched at the same point."""
    name, B = "gqa", 5
    cfg_d = fixtures(name)[0]
    toks = cases.gpt_tokens(cfg_d, steps=5, batch=B).to(DEV)
    old, new = MIXED[B], [2, -1, 1, 0, 0]

    def run(model, switch):
        model.set_adapter_ids(old)
        with model.streaming(B):
            for t in range(3):
                model.forward_global(toks[:, :, t:t + 1])
            ptr = model._bank_ids.data_ptr()
            if switch:
                model.set_adapter_ids(torch.tensor(new, device=DEV))      # a device tensor: no host check, no synchronisation
            assert model._bank_ids.data_ptr() == ptr
            h, lg = model.forward_global(toks[:, :, 3:4])
            graphed = model._streaming_state.graphed_global.graph is not None
            return h.clone(), lg.clone(), graphed

    model = bank_model(name)
    h_old, lg_old, graphed = run(model, False)
    h_new, lg_new, _ = run(model, True)
    assert graphed
    monkeypatch.setenv("NO_CUDA_GRAPH", "1")
    h_ref, lg_ref, graphed = run(bank_model(name), True)
    assert not graphed
    assert torch.equal(h_new, h_ref) and torch.equal(lg_new, lg_ref)
    assert torch.equal(lg_new[4], lg_old[4]) and not torch.equal(lg_new[0], lg_old[0])      # row 4 kept its set; rows 0..3 changed theirs


def test_multi_position_call_in_a_session_across_the_wrap():
    """A T = 5 chunk behind 3 streamed positions on a ring of 6 slots (it wraps inside the chunk): the rows lie ``b * T + t``, so the
    launches take ``rows_per_id = T`` -- equal to the same positions streamed one at a time under the same ids."""
    name, B = "gqa", 5
    cfg_d = fixtures(name)[0]
    toks = cases.gpt_tokens(cfg_d, steps=8, batch=B).to(DEV)
    model = bank_model(name, context=6)
    model.set_adapter_ids(MIXED[B])
    with model.streaming(B):
        ref = [tuple(o.clone() for o in model.forward_global(toks[:, :, t:t + 1])) for t in range(8)]
    with model.streaming(B):
        for t in range(3):
            model.forward_global(toks[:, :, t:t + 1])
        h, lg = model.forward_global(toks[:, :, 3:8])
    assert rel_err(h, torch.cat([r[0] for r in ref[3:]], 1)) < TOL and rel_err(lg, torch.cat([r[1] for r in ref[3:]], 1)) < TOL
    # and the chunk alone, rows of different streams under different sets: against the single-adapter route
    for k in (2, -1):
        b = MIXED[B].index(k)
        single = single_model(name, k, context=6)
        with single.streaming(B):
            for t in range(3):
                single.forward_global(toks[:, :, t:t + 1])
            lg_s = single.forward_global(toks[:, :, 3:8])[1]
        assert rel_err(lg[b], lg_s[b]) < TOL, k


def test_dropping_the_bank_restores_the_single_adapter_model():
    name, B = "gqa", 5
    cfg_d = fixtures(name)[0]
    toks = cases.gpt_tokens(cfg_d, steps=4, batch=B).to(DEV)

    def logits_of(m):
        full = m.forward_global(toks)[1].clone()
        with m.streaming(B):
            return full, torch.cat([m.forward_global(toks[:, :, t:t + 1])[1] for t in range(4)], 1)

    never = logits_of(single_model(name, 0))
    model = bank_model(name, own=0)
    model.set_adapter_ids([1] * B)
    with_bank = logits_of(model)
    assert not torch.equal(with_bank[0], never[0])
    model.load_adapter_bank(None)
    back = logits_of(model)
    assert torch.equal(back[0], never[0]) and torch.equal(back[1], never[1])
    with pytest.raises(RuntimeError, match="no adapter bank"):
        model.set_adapter_ids([0] * B)
