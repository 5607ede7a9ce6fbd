"""CPU checks of the token bookkeeping behind ``LMGen.prefill``: ``prefill_token_plan`` (the model input columns and the token ring of
T teacher-forced frames at once) and ``LMGen.model_time`` against ``oracle.lm_oracle.LMGenOracle`` run frame by frame."""
import pytest
import torch

from oracle import lm_oracle as L
from rstnet_amd import synth
from rstnet_amd.lm.model import LMGen, prefill_token_plan
from tests.golden import cases

_RUNS = {}


def _oracle_run(name: str):
    """Greedy oracle run of LM_STEPS frames: per frame the ring BEFORE it, its input column and the tokens it sampled (model time:
    what the frame writes at column offset + 1); and the delay-aligned outputs."""
    if name not in _RUNS:
        cfg = dict(getattr(synth, name))
        sd = {k: v.float() for k, v in synth.lm_state_dict(cfg, cases.LM_SEED).items()}
        ora = L.LMGenOracle(sd, L.LMConfig(**cfg), cases.LM_BATCH)
        user = cases.lm_user_tokens(cfg)
        CT = ora.cache.shape[2]
        rings, inputs, own, outs = [ora.cache.clone()], [], [], []
        with torch.no_grad():
            for s in range(cases.LM_STEPS):
                o = ora.step(user[s])
                # (the frame's input column is not written again before the frame ends: CT >= 2)
                inputs.append(ora.cache[:, :, s % CT].clone())
                own.append(ora.cache[:, :cfg["dep_q"] + 1, (s + 1) % CT].clone())
                rings.append(ora.cache.clone())
                if o is not None:
                    outs.append(o)
        _RUNS[name] = dict(cfg=cfg, user=torch.cat(list(user), -1), rings=rings, inputs=torch.stack(inputs, -1), own=torch.stack(own, -1),
                           outs=torch.cat(outs, -1), initial=ora.initial.reshape(-1))
    return _RUNS[name]


@pytest.mark.parametrize("name", ["LM_TINY", "LM_TINY_16Q"])
@pytest.mark.parametrize("offset", [0, 1, 4])
@pytest.mark.parametrize("length", [1, 5, None])
def test_prefill_token_plan_equals_stepped_bookkeeping(name, offset, length):
    r = _oracle_run(name)
    T = cases.LM_STEPS - offset if length is None else length
    inputs, ring = prefill_token_plan(r["rings"][offset], offset, r["user"][:, :, offset:offset + T], r["own"][:, :, offset:offset + T],
                                      r["cfg"]["delays"], r["initial"])
    assert torch.equal(inputs, r["inputs"][:, :, offset:offset + T])
    # the whole ring, which covers every entry a later frame or gather reads
    assert torch.equal(ring, r["rings"][offset + T])


@pytest.mark.parametrize("name", ["LM_TINY", "LM_TINY_16Q"])
def test_prefill_token_plan_leaves_its_arguments_alone(name):
    r = _oracle_run(name)
    cache, user, own = r["rings"][2].clone(), r["user"][:, :, 2:7].clone(), r["own"][:, :, 2:7].clone()
    prefill_token_plan(cache, 2, user, own, r["cfg"]["delays"], r["initial"])
    assert torch.equal(cache, r["rings"][2]) and torch.equal(user, r["user"][:, :, 2:7]) and torch.equal(own, r["own"][:, :, 2:7])


class _Tokens:
    """What ``LMGen.model_time`` reads of a model: the stream layout and the initial tokens."""

    def __init__(self, cfg):
        self.cfg, self.delays, self.dep_q, self.training = cfg, cfg["delays"], cfg["dep_q"], False
        self.device = torch.device("cpu")

    def _get_initial_token(self):
        tok = torch.full([1, self.cfg["n_q"] + 1, 1], self.cfg["card"], dtype=torch.long)
        tok[:, 0] = self.cfg["text_card"]
        return tok


@pytest.mark.parametrize("name", ["LM_TINY", "LM_TINY_16Q"])
def test_model_time_inverts_the_delay_alignment(name):
    r = _oracle_run(name)
    gen = LMGen(_Tokens(r["cfg"]), use_sampling=False)
    A = r["outs"].shape[2]
    assert A == cases.LM_STEPS - max(r["cfg"]["delays"])
    own = gen.model_time(r["outs"])
    assert own.shape == r["outs"].shape
    for k, d in enumerate(r["cfg"]["delays"][:r["cfg"]["dep_q"] + 1]):
        assert torch.equal(own[:, k, d:], r["own"][:, k, d:A]), k       # every entry a prefill reads
        assert (own[:, k, :d] == (r["cfg"]["text_card"] if k == 0 else r["cfg"]["card"])).all()
