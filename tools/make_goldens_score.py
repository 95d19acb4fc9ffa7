#!/usr/bin/env python
"""Generate the caption-scoring fixture from the REAL HF implementation (transformers 5.15.0 `BlipForConditionalGeneration`, CPU
fp32): teacher forcing, `model(pixel_values=..., input_ids=..., attention_mask=...).logits`, reduced in float64 to what
`CaptionerEngine.score` returns.  Run in the build container only:

    python tools/make_goldens_score.py            # writes tests/golden/blip_tiny_score.npz and blip2_tiny_score.npz

Same weights and frames as tools/make_goldens.py's blip_tiny (`procedural_blip_state_dict`, `synthetic_pixels`); data only.
4 images x 3 captions of up to L = 12 tokens: per image a caption of 2 tokens, one of a middle length and one of L; random ids that
are none of BOS / [SEP] / pad, the full-length captions of images 1 and 3 ending in [SEP]; the middle caption of image 0 is HF's
own greedy caption of that image including its [SEP].  Rows are right-padded with the pad id and go through HF with their
attention mask.  Stored per position j < lens - 1: log_softmax(logits[j])[ids[j + 1]], the arg-max and the top-2 logit margin.
The maker asserts that the CPU restatement (tests/_score_ref.py on oracle/blip_ref.py) reproduces HF within 1e-4, the bar
tools/make_goldens_blip2_beam.py asserts for scores.

BLIP-2 (`Blip2ForConditionalGeneration`, tools/make_goldens_blip2.py's tiny model): the same layout; `input_ids` = the image
placeholders, BOS and the caption, the logits of the positions from BOS on.  The row of HF's own greedy caption ends in the generation
EOS; the restatement is tests/_score_ref.py::blip2_score on oracle/blip2_ref.py."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from embodied_captioning_amd.config import BlipArch                      # noqa: E402
from embodied_captioning_amd.weights import procedural_blip_state_dict, synthetic_pixels  # noqa: E402
from make_goldens import build_hf                                         # noqa: E402
from _score_ref import blip2_score, blip_score, random_captions, reduce_rows           # noqa: E402

SEED, EOS_BOOST, BATCH, C, L, MIDDLE = 3, 2.0, 4, 3, 12, (0, 5, 7, 9)     # MIDDLE[0] is replaced by the greedy caption's length


def main():
    torch.manual_seed(0)
    arch = BlipArch.tiny()
    sd = procedural_blip_state_dict(arch, SEED, eos_boost=EOS_BOOST)
    model = build_hf(arch, sd)
    pixels = synthetic_pixels(BATCH, arch.image_size, seed=SEED)
    with torch.no_grad():
        own = model.generate(pixel_values=pixels[:1], max_length=L, num_beams=1, do_sample=False)[0].tolist()
    own = own[: own.index(arch.eos) + 1] if arch.eos in own else own
    assert own[0] == arch.bos and 2 <= len(own) <= L, own
    N = BATCH * C
    ids = random_captions(arch, N, L, None, seed=SEED)
    lens = np.zeros(N, dtype=np.int32)
    for b in range(BATCH):
        lens[b * C: b * C + 3] = (2, MIDDLE[b], L)
    ids[1, : len(own)] = own
    lens[1] = len(own)
    for b in (1, 3):
        ids[b * C + 2, L - 1] = arch.eos
    hf_ids = torch.from_numpy(ids).long()
    mask = (torch.arange(L)[None, :] < torch.from_numpy(lens).long()[:, None]).long()
    hf_ids = torch.where(mask.bool(), hf_ids, torch.full_like(hf_ids, arch.pad))
    with torch.no_grad():
        logits = model(pixel_values=pixels.repeat_interleave(C, dim=0), input_ids=hf_ids, attention_mask=mask).logits
    assert tuple(logits.shape) == (N, L, arch.vocab)
    tlp = np.zeros((N, L - 1))
    tid = np.zeros((N, L - 1), dtype=np.int64)
    margin = np.full((N, L - 1), np.inf)
    live = np.arange(L - 1)[None, :] < (lens[:, None] - 1)
    for j in range(L - 1):
        a, _, c, d = reduce_rows(logits[:, j], hf_ids[:, j + 1])
        on = live[:, j]
        tlp[on, j], tid[on, j], margin[on, j] = a.numpy()[on], c.numpy()[on], d.numpy()[on]
    for dt in (torch.float32, torch.float64):
        ref = blip_score(sd, arch, pixels, ids, lens, C, dtype=dt)
        err = float(np.abs(ref["token_logprobs"] - tlp)[live].max())
        print(f"restatement {dt} against HF: max |d log-prob| {err:.3e}")
        assert err <= 1e-4, err
        assert np.array_equal(ref["live"], live)
        assert np.array_equal(ref["top_ids"][live & (margin > 1e-4)], tid[live & (margin > 1e-4)])
    own_row = tid[1, : lens[1] - 1].tolist()
    assert own_row == own[1:], (own_row, own)                     # the greedy caption is its own arg-max path
    out = {"ids": ids, "lens": lens, "token_logprobs": tlp, "top_ids": tid.astype(np.int32), "margin": margin,
           "meta": np.array(json.dumps(dict(seed=SEED, eos_boost=EOS_BOOST, batch=BATCH, captions_per_image=C, max_length=L,
                                            own_caption_row=1, arch=arch.__dict__, transformers="5.15.0", torch=torch.__version__)))}
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "blip_tiny_score.npz"), **out)
    print("done", lens.tolist())


def main_blip2():
    from embodied_captioning_amd.config import Blip2Arch
    from embodied_captioning_amd.weights import procedural_blip2_state_dict
    from make_goldens_blip2 import build_hf as build_hf2
    import dataclasses
    torch.manual_seed(0)
    seed, boost = 3, 0.3
    arch = Blip2Arch.tiny()
    sd = procedural_blip2_state_dict(arch, seed, eos_boost=boost)
    model = build_hf2(arch, sd)
    pixels = synthetic_pixels(BATCH, arch.image_size, seed=seed)
    nq = arch.num_query_tokens
    with torch.no_grad():
        own = model.generate(pixel_values=pixels[:1], max_new_tokens=L - 1, do_sample=False, num_beams=1)[0].tolist()
    own = own[own.index(arch.bos):] if arch.image_token in own else ([arch.bos] + own if own[0] != arch.bos else own)
    own = own[: own.index(arch.eos) + 1] if arch.eos in own else own[:L]
    assert own[0] == arch.bos and 2 <= len(own) <= L, own
    N = BATCH * C
    ids = random_captions(arch, N, L, None, seed=seed, special=(arch.image_token,))
    lens = np.zeros(N, dtype=np.int32)
    for b in range(BATCH):
        lens[b * C: b * C + 3] = (2, MIDDLE[b] or 5, L)
    ids[1, : len(own)] = own
    lens[1] = len(own)
    for b in (1, 3):
        ids[b * C + 2, L - 1] = arch.eos
    cap = torch.from_numpy(ids).long()
    mask = torch.arange(L)[None, :] < torch.from_numpy(lens).long()[:, None]
    cap = torch.where(mask, cap, torch.full_like(cap, arch.pad))
    hf_ids = torch.cat([torch.full((N, nq), arch.image_token), cap], 1)
    hf_mask = torch.cat([torch.ones((N, nq), dtype=torch.long), mask.long()], 1)
    with torch.no_grad():
        logits = model(pixel_values=pixels.repeat_interleave(C, dim=0), input_ids=hf_ids, attention_mask=hf_mask).logits
    assert tuple(logits.shape) == (N, nq + L, arch.vocab), logits.shape
    logits = logits[:, nq:]
    tlp = np.zeros((N, L - 1))
    tid = np.zeros((N, L - 1), dtype=np.int64)
    margin = np.full((N, L - 1), np.inf)
    live = np.arange(L - 1)[None, :] < (lens[:, None] - 1)
    for j in range(L - 1):
        a, _, c, d = reduce_rows(logits[:, j], cap[:, j + 1])
        on = live[:, j]
        tlp[on, j], tid[on, j], margin[on, j] = a.numpy()[on], c.numpy()[on], d.numpy()[on]
    for dt in (torch.float32, torch.float64):
        ref = blip2_score(sd, arch, pixels, ids, lens, C, dtype=dt)
        err = float(np.abs(ref["token_logprobs"] - tlp)[live].max())
        print(f"blip2 restatement {dt} against HF: max |d log-prob| {err:.3e}")
        assert err <= 1e-4, err
        assert np.array_equal(ref["top_ids"][live & (margin > 1e-4)], tid[live & (margin > 1e-4)])
    assert tid[1, : lens[1] - 1].tolist() == own[1:], (tid[1].tolist(), own)
    out = {"ids": ids, "lens": lens, "token_logprobs": tlp, "top_ids": tid.astype(np.int32), "margin": margin,
           "meta": np.array(json.dumps(dict(seed=seed, eos_boost=boost, batch=BATCH, captions_per_image=C, max_length=L, own_caption_row=1,
                                            arch=dataclasses.asdict(arch), transformers="5.15.0", torch=torch.__version__)))}
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "blip2_tiny_score.npz"), **out)
    print("blip2 done", lens.tolist())


if __name__ == "__main__":
    main()
    main_blip2()
