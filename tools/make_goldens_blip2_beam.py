#!/usr/bin/env python
"""Golden vectors for BLIP-2 beam search: the REAL HuggingFace Blip2ForConditionalGeneration (imported only in the build container)
on `Blip2Arch.tiny()` procedural weights, `generate(pixel_values, num_beams=K, length_penalty=lp, return_dict_in_generate=True,
output_scores=True)` over 4 images at (K, lp) = (3, 1.0), (3, 2.0), (5, 1.0) -> tests/golden/blip2_tiny_beam.npz.

A beam search whose scores nearly tie somewhere cannot be compared token by token with another arithmetic, so per (K, lp) the
weights' seed is searched (0 .. 63, eos_boost 0.5) for the one whose smallest DECISION GAP over the images (tests/_blip2_beam_ref.py,
fp64 restatement) is largest - among the seeds whose search is worth pinning: at least MIN_REORDERS model steps run on re-ordered
beams and at least half of the captions have MIN_TOKENS new tokens (the widest gaps belong to searches that end on their first
token).  A seed that keeps every image above the bar is taken where one qualifies; only otherwise the seed with the largest
second-smallest gap, which leaves one image out.  The gap of every image is stored.  An image whose gap is below 1e-3 is listed in `omit_*` (at most one
per case, asserted here together with HF-fp32 = the fp64 restatement's tokens on the others): GPU tests compare tokens on the
others only, and read the list from the file.

    python tools/make_goldens_blip2_beam.py
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from embodied_captioning_amd.config import Blip2Arch  # noqa: E402
from embodied_captioning_amd.weights import procedural_blip2_state_dict, synthetic_pixels  # noqa: E402
from make_goldens_blip2 import build_hf  # noqa: E402
import _blip2_beam_ref as BR  # noqa: E402

CASES = [(3, 1.0), (3, 2.0), (5, 1.0)]
BATCH, EOS_BOOST, GAP_BAR = 4, 0.5, 1e-3
MIN_REORDERS, MIN_TOKENS = 3, 4


def case_key(K, lp):
    return f"k{K}_lp{lp:g}".replace(".", "p")


def hf_beams(a, sd, px, K, lp):
    """-> new tokens int32 [B, max_new] (fill behind the end), sequences_scores [B], best minus second-best returned score [B]."""
    m = build_hf(a, sd)
    n = a.max_new_tokens
    with torch.no_grad():
        out = m.generate(pixel_values=px, num_beams=K, length_penalty=lp, max_new_tokens=n, return_dict_in_generate=True,
                         output_scores=True)
        two = m.generate(pixel_values=px, num_beams=K, length_penalty=lp, max_new_tokens=n, return_dict_in_generate=True,
                         output_scores=True, num_return_sequences=2)
    new = out.sequences[:, a.num_query_tokens + 1:]                          # HF returns image placeholders + BOS + new tokens
    fill = a.pad if a.pad else a.eos
    ids = np.full((px.shape[0], n), fill, dtype=np.int32)
    ids[:, : new.shape[1]] = new.numpy()
    s2 = two.sequences_scores.view(px.shape[0], 2)
    return ids, out.sequences_scores.numpy().astype(np.float32), (s2[:, 0] - s2[:, 1]).numpy().astype(np.float32)


def main():
    a = Blip2Arch.tiny()
    out, meta = {}, {"eos_boost": EOS_BOOST, "batch": BATCH, "gap_bar": GAP_BAR, "transformers": __import__("transformers").__version__,
                     "cases": {}}
    for K, lp in CASES:
        best = None
        for seed in range(64):
            sd = procedural_blip2_state_dict(a, seed, eos_boost=EOS_BOOST)
            px = synthetic_pixels(BATCH, a.image_size, seed=seed)
            r64 = BR.beam_search(sd, a, px, K, lp, dtype=np.float64)
            if r64["reorders"] < MIN_REORDERS or np.median(r64["lens"]) < MIN_TOKENS:
                continue
            # a seed that leaves no image below the bar first, the largest minimal gap among those; only where no qualifying seed
            # does: the second-smallest gap (one image is then left out), then the smallest
            lo, second = np.sort(r64["gap"])[:2]
            rank = (lo >= GAP_BAR, lo, lo) if lo >= GAP_BAR else (False, second, lo)
            if best is None or rank > best[0]:
                best = (rank, seed, r64)
        _, seed, r64 = best
        sd = procedural_blip2_state_dict(a, seed, eos_boost=EOS_BOOST)
        px = synthetic_pixels(BATCH, a.image_size, seed=seed)
        ids, scores, top2 = hf_beams(a, sd, px, K, lp)
        omit = np.nonzero(r64["gap"] < GAP_BAR)[0].astype(np.int32)
        assert len(omit) <= 1, (K, lp, seed, r64["gap"])
        keep = np.setdiff1d(np.arange(BATCH), omit)
        assert np.array_equal(ids[keep], r64["ids"][keep]), (K, lp, seed, ids, r64["ids"])
        assert np.abs(scores[keep] - r64["scores"][keep]).max() < 1e-4, (scores, r64["scores"])
        key = case_key(K, lp)
        out[f"ids_{key}"], out[f"scores_{key}"], out[f"top2_{key}"] = ids, scores, top2
        out[f"gap_{key}"], out[f"omit_{key}"] = r64["gap"].astype(np.float64), omit
        meta["cases"][key] = {"K": K, "lp": lp, "seed": seed}
        print(key, "seed", seed, "reorders", r64["reorders"], "gaps", r64["gap"], "omit", omit.tolist(), "top2", top2, "\n", ids)
    out["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "blip2_tiny_beam.npz"), **out)
    print("done")


if __name__ == "__main__":
    main()
