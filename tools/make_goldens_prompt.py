#!/usr/bin/env python
"""Generate the text-prompt fixtures from the REAL HF implementation (transformers 5.15.0 `BlipForConditionalGeneration`, CPU
fp32): conditional captioning, `model.generate(pixel_values=..., input_ids=[bos, ids..., sep], ...)` - HF replaces column 0 by
BOS and hands `input_ids[:, :-1]` to the text decoder (modeling_blip.py:858-932).  Run in the build container only:

    python tools/make_goldens_prompt.py            # writes tests/golden/blip_tiny_prompt.npz and blip_base_prompt.npz
    python tools/make_goldens_prompt.py --tiny-only

Same weights and frames as tools/make_goldens.py's blip_tiny / blip_base (`procedural_blip_state_dict`, `synthetic_pixels`);
data only.  The prompt (3 tokens after BOS, P = 4, shared by the frames) comes from a seeded candidate search: the first draw of
`np.random.default_rng(1234)` whose captions keep a top-1 / top-2 margin of at least 5e-3 at every live step (so an fp32-grade
implementation must reproduce the tokens) and do not all have the same length (so early endings are exercised).
What the search lands on (recorded in each file's `meta`): tiny candidate 0, [491, 490, 496] - its captions are short (lengths
6 / 6 / 6 / 5 with P = 4: one or two generated steps per row), so the tiny fixture pins the prompt handling, the step indexing and
the zero tail on few steps; base candidate 2, [4095, 8723, 5095] (lengths 18 / 20 / ...: up to 16 generated steps per row) and the
own-prefix test of tests/test_prompt_gpu.py carry the coverage of long prompted captions.
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from embodied_captioning_amd.config import BlipArch                      # noqa: E402
from embodied_captioning_amd.weights import procedural_blip_state_dict, synthetic_pixels  # noqa: E402
from make_goldens import build_hf                                         # noqa: E402

MIN_MARGIN = 5e-3
N_PROMPT = 3            # tokens after BOS: P = 4


def prompted(model, arch, pixels, ids, max_length):
    """HF conditional generation with the shared prompt `ids` -> (sequences int64 [B, max_length] padded as run_greedy_only pads,
    logits [T, B, V] of the generated steps, live [T, B]: the row was open when step j ran)."""
    B = pixels.shape[0]
    inp = torch.tensor([[arch.bos] + [int(i) for i in ids] + [arch.eos]] * B, dtype=torch.long)
    with torch.no_grad():
        g = model.generate(pixel_values=pixels, input_ids=inp, max_length=max_length, do_sample=False, num_beams=1,
                           output_logits=True, return_dict_in_generate=True)
    seq = torch.full((B, max_length), arch.pad, dtype=torch.long)          # HF trims when every caption ends early
    seq[:, : g.sequences.shape[1]] = g.sequences
    logits = torch.stack(list(g.logits), 0)
    P = 1 + len(ids)
    assert torch.equal(seq[:, :P], inp[:, :P]) and g.sequences.shape[1] == P + logits.shape[0]
    live = torch.ones(logits.shape[:2], dtype=torch.bool)
    for j in range(1, logits.shape[0]):
        live[j] = live[j - 1] & (seq[:, P + j - 1] != arch.eos)
    return seq, logits, live


def lengths_of(seq, arch):
    out = []
    for r in seq.tolist():
        out.append(r.index(arch.eos) + 1 if arch.eos in r else len(r))
    return out


def search(model, arch, pixels, max_length, lo, hi, tries=64):
    rng = np.random.default_rng(1234)
    for k in range(tries):
        ids = [int(i) for i in rng.integers(lo, hi, size=N_PROMPT)]
        seq, logits, live = prompted(model, arch, pixels, ids, max_length)
        top = torch.topk(logits, k=2, dim=-1).values
        margin = top[..., 0] - top[..., 1]
        mmin = float(margin[live].min())
        lens = lengths_of(seq, arch)
        print(f"  candidate {k} {ids}: minimal live margin {mmin:.3e}, lengths {lens}")
        if mmin >= MIN_MARGIN and len(set(lens)) > 1:
            return ids, seq, logits, live, margin
    raise SystemExit(f"no prompt among {tries} candidates keeps a margin of {MIN_MARGIN} with unequal lengths")


def run(arch, seed, batch, max_length, eos_boost, lo, full):
    sd = procedural_blip_state_dict(arch, seed, eos_boost=eos_boost)
    model = build_hf(arch, sd)
    pixels = synthetic_pixels(batch, arch.image_size, seed=seed)
    t0 = time.time()
    ids, seq, logits, live, margin = search(model, arch, pixels, max_length, lo, arch.vocab - 10)
    print(f"  chosen {ids} after {time.time() - t0:.1f}s")
    lens = lengths_of(seq, arch)
    assert float(margin[live].min()) >= MIN_MARGIN, "minimal live margin below the bar"
    assert len(set(lens)) > 1, "every caption has the same length"
    P = 1 + len(ids)
    T = max_length - P
    m = torch.full((T, batch), 1e9)                                    # steps HF never ran (all captions over): no constraint
    m[: margin.shape[0]] = torch.where(live, margin, torch.full_like(margin, 1e9))
    lv = torch.zeros((T, batch), dtype=torch.bool)
    lv[: live.shape[0]] = live
    out = {"prompt_ids": np.asarray([arch.bos] + ids, dtype=np.int32), "greedy_sequences": seq.numpy().astype(np.int32),
           "greedy_margin": m.numpy(), "greedy_live": lv.numpy(), "greedy_lengths": np.asarray(lens, dtype=np.int32)}
    if full:
        lg = torch.zeros((T, batch, arch.vocab))
        lg[: logits.shape[0]] = logits
        out["greedy_logits_full"] = lg.numpy()
    else:
        top = torch.topk(logits, k=8, dim=-1)
        ti = torch.zeros((T, batch, 8), dtype=torch.int32)
        tv = torch.zeros((T, batch, 8))
        ti[: logits.shape[0]] = top.indices.to(torch.int32)
        tv[: logits.shape[0]] = top.values
        out["greedy_top8_ids"], out["greedy_top8_vals"] = ti.numpy(), tv.numpy()
    out["meta"] = np.array(json.dumps(dict(seed=seed, eos_boost=eos_boost, batch=batch, max_length=max_length, beams=1,
                                           prompt_ids=[arch.bos] + ids, min_live_margin=float(margin[live].min()),
                                           arch=arch.__dict__, transformers="5.15.0", torch=torch.__version__)))
    return out


def main():
    torch.manual_seed(0)
    gold = os.path.join(ROOT, "tests", "golden")
    print("blip_tiny_prompt")
    np.savez_compressed(os.path.join(gold, "blip_tiny_prompt.npz"),
                        **run(BlipArch.tiny(), seed=3, batch=4, max_length=12, eos_boost=2.0, lo=10, full=True))
    if "--tiny-only" in sys.argv:
        return
    print("blip_base_prompt")
    np.savez_compressed(os.path.join(gold, "blip_base_prompt.npz"),
                        **run(BlipArch(), seed=0, batch=8, max_length=20, eos_boost=9.0, lo=1000, full=False))
    print("done")


if __name__ == "__main__":
    main()
