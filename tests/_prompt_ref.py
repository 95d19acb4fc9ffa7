"""CPU expectation of prompted greedy decoding, composed from the fp32 restatement (oracle/blip_ref.py): the prompt's tokens are
FORCED through `decoder_step` one position at a time (their logits discarded), then the greedy loop of `greedy_generate` goes on
from the last prompt token.  What HF `BlipForConditionalGeneration.generate(pixel_values, input_ids=...)` computes, and what a
prefill must leave behind.  Never imported by the product package."""
import numpy as np
import torch

from oracle import blip_ref


@torch.no_grad()
def prompted_greedy(sd, arch, pixels, prompt, max_length, image_embeds=None):
    """prompt: ints [P], [1, P] or [B, P] with column 0 = BOS.  -> dict(sequences int64 [B, max_length] padded with pad (rows start
    with the prompt), lengths [B] incl. the prompt, logits [T, B, V] of the generated steps (T = steps run), margins [max_length - P, B]
    top-1 minus top-2 of the steps at which the row was open, 1e9 elsewhere)."""
    if image_embeds is None:
        image_embeds = blip_ref.encode_image(sd, arch, pixels)
    B = image_embeds.shape[0]
    p = torch.as_tensor(np.asarray(prompt), dtype=torch.int64)
    if p.dim() == 1:
        p = p[None]
    p = p.expand(B, p.shape[1]).clone()
    P = p.shape[1]
    state = blip_ref.DecoderState(arch.t_layers)
    blip_ref.cross_kv(sd, arch, image_embeds, state)
    for j in range(P - 1):
        blip_ref.decoder_step(sd, arch, p[:, j], state)           # forced token: the caches grow, nothing is selected
    seq = p
    unfinished = torch.ones(B, dtype=torch.int64)
    steps, margins = [], []
    while True:
        logits = blip_ref.decoder_step(sd, arch, seq[:, -1], state)
        steps.append(logits)
        t2 = torch.topk(logits, 2, dim=-1).values
        margins.append(torch.where(unfinished.bool(), t2[:, 0] - t2[:, 1], torch.full((B,), 1e9)))
        nxt = torch.argmax(logits, dim=-1)
        nxt = nxt * unfinished + arch.pad * (1 - unfinished)
        seq = torch.cat([seq, nxt[:, None]], dim=-1)
        unfinished = unfinished & (nxt != arch.eos).long()
        if seq.shape[1] >= max_length or unfinished.max() == 0:
            break
    out = torch.full((B, max_length), arch.pad, dtype=torch.int64)
    out[:, : seq.shape[1]] = seq
    lens = torch.tensor([r.index(arch.eos) + 1 if arch.eos in r else max_length for r in out[:, P:].tolist()]) + P
    lens = torch.clamp(lens, max=max_length)
    m = torch.full((max_length - P, B), 1e9)
    m[: len(margins)] = torch.stack(margins)
    return {"sequences": out, "lengths": lens, "logits": torch.stack(steps), "margins": m}


def full_margins(margins, P, L):
    """Margins of the generated steps [L - P, B] -> the [L - 1, B] array tests/_util.token_parity indexes by position: the prompt
    positions are given (never a near-tie)."""
    margins = np.asarray(margins)
    out = np.full((L - 1, margins.shape[1]), 1e9, dtype=np.float64)
    out[P - 1:] = margins[: L - P]
    return out
