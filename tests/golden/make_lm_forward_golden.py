"""Generate tests/golden/lm_tiny_forward.npz by running the REAL reference's teacher-forced ``LMModel.forward``.

Runs only in the build container (needs /root/reference, read-only, imported in place; nothing from it is copied), in the style
of make_golden.py.  The .npz holds data only: a seeded token sequence and the reference's outputs on ``synth.LM_TINY``.

    NO_TORCH_COMPILE=1 python -B tests/golden/make_lm_forward_golden.py

``LMModel.forward`` (models/model.py:297-319) is the NON-streaming pass: positions 0 .. S-1 under the plain causal + context mask.
With S = 14 > context = 10 it differs from the stepped ``forward_text`` (whose ring hides one more key) from position 9
on; the script prints that difference so that the two windows can be told apart from the fixture's own numbers.
"""
import os
import sys

os.environ["NO_TORCH_COMPILE"] = "1"
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, "/root/reference/MLLM_v2")
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from rstnet_amd import synth  # noqa: E402
from tests.golden import cases  # noqa: E402

FWD_SEED, FWD_B, FWD_S = 91, 2, 14


def forward_sequence(cfg: dict) -> torch.Tensor:
    """int64 ``[B, n_q + 1, S]``: row 0 text ids, rows 1.. audio ids, one -1 ('no input') entry."""
    g = torch.Generator().manual_seed(FWD_SEED)
    text = torch.randint(0, cfg["text_card"], (FWD_B, 1, FWD_S), generator=g)
    audio = torch.randint(0, cfg["card"], (FWD_B, cfg["n_q"], FWD_S), generator=g)
    audio[0, 1, 2] = -1
    return torch.cat([text, audio], 1)


@torch.no_grad()
def main():
    from models.model import LMModel
    cfg = dict(synth.LM_TINY)
    sd = {k: v.float() for k, v in synth.lm_state_dict(cfg, cases.LM_SEED).items()}
    m = LMModel(causal=True, layer_scale=None, gating="silu", norm="rms_norm_f32", positional_embedding="rope",
                depformer_causal=True, depformer_layer_scale=None, depformer_multi_linear=True, depformer_context=8,
                depformer_max_period=10000, depformer_gating="silu", depformer_pos_emb="none",
                depformer_weights_per_step=True, **cfg).eval()
    m.load_state_dict(sd, strict=True)
    seq = forward_sequence(cfg)
    audio_logits, text_logits = m.forward(seq)
    shifted = torch.cat([m._get_initial_token().repeat(FWD_B, 1, 1), seq[:, :, :-1]], dim=2)
    transformer_out, _ = m.forward_text(shifted)
    # forward_local on its own: another text row as the start token and un-shifted audio rows, on the same transformer_out
    local_ids = seq[:, 0, :]
    local_seq = seq[:, 1:cfg["dep_q"] + 1, :]
    local_logits = m.forward_local(m.depformer_text_emb(local_ids), local_seq, transformer_out)
    # the stepped pass over the same input, for the record: where the two windows part
    outs = []
    with m.streaming(FWD_B):
        for t in range(FWD_S):
            outs.append(m.forward_text(shifted[:, :, t:t + 1])[0])
    stepped = torch.cat(outs, 1)
    rel = [(float((stepped[:, t] - transformer_out[:, t]).abs().max() / transformer_out[:, t].abs().max())) for t in range(FWD_S)]
    print("forward vs stepped forward_text, per position:", " ".join(f"{r:.1e}" for r in rel))
    np.savez(os.path.join(HERE, "lm_tiny_forward.npz"), sequence=seq.numpy().astype(np.int32), audio_logits=audio_logits.numpy(),
             text_logits=text_logits.numpy(), transformer_out=transformer_out.numpy(), local_ids=local_ids.numpy().astype(np.int32),
             local_sequence=local_seq.numpy().astype(np.int32), local_logits=local_logits.numpy())
    print("lm_tiny_forward", tuple(audio_logits.shape), tuple(text_logits.shape), tuple(local_logits.shape))


if __name__ == "__main__":
    main()
