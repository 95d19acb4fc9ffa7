"""Pseudo-captions by probability fusion - the reference's third way to an object's pseudo-caption
(captioner/generate_pseudo_caption_from_file.py with captioner/test_pseudo_caption_generation.py:28-63): for every caption of an
object the softmax of each decode step's logits row and each vocabulary entry's maximum over the steps; those vectors averaged
over the object's captions; the tokens whose mean exceeds `th`, in ascending id order, decoded.  No second model.

Two ways in:
  * the host functions with the reference's names, for callers who hold `forward()["logits"]`:
    `compute_max_tokens_probability`, `compute_average_tokens_probability`, `generate_pseudo_caption(probs, th, tokenizer)`;
  * `fused_pseudo_captions(grouped, captioner)` over `pseudocaptioner.group_records` output: one batched
    `generate_batch(..., output_vocab_maxprob=True)` per micro-batch (the selection kernel keeps the per-caption vector, no logits
    buffer, pool and row compaction on) and one group kernel per batch of groups (`engine.fuse_vocab_groups`); a few dozen token
    ids per object cross to the host.

    python -m embodied_captioning_amd.captioner.pseudo_caption_fusion --file_path DIR --output_csv_path OUT.csv \\
        --arch_name blip|coca|blip2 [--model DIR] [--th 0.25]

writes the reference's CSV: `episode_id, object_id, pseudo_caption`.

Three deliberate departures from the reference script:
  1. objects are grouped by (episode, object); the script flushes after every third object (its intended condition is commented out);
  2. decoding uses the model's own tokenizer and skips special ids; the script uses `open_clip.decode` for BLIP-2 as well and cuts
     at the EOS text, which on a BERT vocabulary would drop everything above id 102;
  3. a caption's steps are the steps at which its row was open - what coca_model.py:311-313 appends, = `scored_steps`.
"""
from __future__ import annotations

import argparse
import csv
import glob
import os
from typing import Dict, List, Sequence

import numpy as np
import torch

from ..engine import fusion_max_tokens, vocab_group_csr          # noqa: F401  (re-exported: the CSR builder and the K bound)

DEFAULT_MODELS = {"blip": "Salesforce/blip-image-captioning-base", "coca": "coca_ViT-L-14", "blip2": "Salesforce/blip2-opt-2.7b"}
CSV_HEADER = ["episode_id", "object_id", "pseudo_caption"]


# ------------------------------------------------------------------------------------------------ host functions
def compute_max_tokens_probability(probs: torch.Tensor) -> torch.Tensor:
    """probs [steps, vocab] of one caption -> [vocab]: each token's maximal probability over the caption's steps."""
    return torch.max(probs, dim=0)[0]


def compute_average_tokens_probability(token_probs: torch.Tensor) -> torch.Tensor:
    """token_probs [captions, vocab] -> [vocab]: the mean over the captions."""
    return torch.sum(token_probs, dim=0) / token_probs.shape[0]


def pseudo_caption_tokens(probs: Sequence[torch.Tensor], th: float):
    """probs: one [steps_s, vocab] probability tensor per caption -> (ids int64 ascending, their mean probabilities)."""
    if len(probs) == 0:
        raise ValueError("generate_pseudo_caption needs at least one caption's probabilities")
    token_probs = torch.stack([compute_max_tokens_probability(p) for p in probs], dim=0)
    mean = compute_average_tokens_probability(token_probs)
    ids = torch.where(mean > th)[0]                     # strict, ascending ids
    return ids, mean[ids]


def special_token_ids(arch) -> set:
    """The ids a decoded pseudo-caption never shows: BOS / SOT and EOS, and the pad id where it is a token of its own (CoCa's pad
    id 0 is an ordinary vocabulary entry, "!")."""
    names = ("sot", "eos") if hasattr(arch, "sot") else ("bos", "eos", "pad")
    return {int(getattr(arch, n)) for n in names if getattr(arch, n, None) is not None}


def decode_tokens(ids: Sequence[int], tokenizer) -> str:
    """Token ids -> text with the special ids skipped.  tokenizer: an HF tokenizer (`decode(ids, skip_special_tokens=True)`), one of
    this package's captioners (its `arch` names the special ids, its `decode` does the rest), or a callable ids -> str."""
    ids = [int(i) for i in ids]
    if hasattr(tokenizer, "arch") and hasattr(tokenizer, "decode"):
        skip = special_token_ids(tokenizer.arch)
        return tokenizer.decode([i for i in ids if i not in skip]).strip()
    if hasattr(tokenizer, "decode"):
        return tokenizer.decode(ids, skip_special_tokens=True).strip()
    if callable(tokenizer):
        return tokenizer(ids).strip()
    raise TypeError(f"cannot decode with {type(tokenizer).__name__}: need .decode(ids, skip_special_tokens=True) or a callable")


def generate_pseudo_caption(probs: Sequence[torch.Tensor], th: float, tokenizer) -> str:
    """The reference's `generate_pseudo_caption(probs, th)` with the tokenizer made explicit (departure 2)."""
    ids, _ = pseudo_caption_tokens(probs, th)
    return decode_tokens(ids.tolist(), tokenizer)


# ------------------------------------------------------------------------------------------------ batched device path
def _host_crops(frames, rects):
    from ..pseudocaptioner import host_crops
    from PIL import Image
    return [Image.fromarray(c) for c in host_crops(frames, rects)]


def fused_pseudo_captions(grouped: Dict, captioner, th: float = 0.25, expand_factor: float = 0.0, crop=None,
                          rows_per_call: int = 1024) -> Dict[str, dict]:
    """grouped: (episode, object) -> [{'image': BGR uint8 frame, 'pred_box': (x1, y1, x2, y2), ...}, ...] as
    `pseudocaptioner.group_records` returns it.  -> {str(key): {'captions': [str], 'token_ids': [int], 'token_probs': [float],
    'pseudo_caption': str}} for every group with at least one instance.
    The crop of an instance is the reference script's numpy slice of its box (expand_factor 0.0; crop(frames, rects) -> images in
    frame-major order replaces it).  Consecutive groups are batched up to `rows_per_call` crops: one
    `captioner.generate_batch(crops, output_vocab_maxprob=True)` and one `captioner.engine.fuse_vocab_groups` per batch."""
    from ..pseudocaptioner import crop_rect
    crop = crop or _host_crops
    keys = [k for k in grouped if len(grouped[k])]
    out: Dict[str, dict] = {}
    start = 0
    while start < len(keys):
        stop, n = start, 0
        while stop < len(keys) and (stop == start or n + len(grouped[keys[stop]]) <= rows_per_call):
            n += len(grouped[keys[stop]])
            stop += 1
        batch = keys[start:stop]
        start = stop
        frames, rects, owner, frame_idx = [], [], [], {}
        for k in batch:
            for inst in grouped[k]:
                img = inst["image"]
                fi = frame_idx.setdefault(id(img), len(frames))
                if fi == len(frames):
                    frames.append(np.ascontiguousarray(img))
                    rects.append([])
                rects[fi].append(crop_rect(inst["pred_box"], img.shape, expand_factor))
                owner.append((fi, len(rects[fi]) - 1))
        images = crop(frames, rects)
        first = np.cumsum([0] + [len(r) for r in rects])
        images = [images[int(first[fi]) + j] for fi, j in owner]               # group / input order
        res = captioner.generate_batch(images, output_vocab_maxprob=True)
        groups, r0 = [], 0
        for k in batch:
            groups.append(list(range(r0, r0 + len(grouped[k]))))
            r0 += len(grouped[k])
        ids, probs, counts = captioner.engine.fuse_vocab_groups(res["vocab_maxprob"], groups, th)
        ids, probs, counts = ids.cpu(), probs.cpu(), counts.cpu()
        for g, k in enumerate(batch):
            c = int(counts[g])
            tok = ids[g, :c].tolist()
            out[str(k)] = {"captions": [res["texts"][r] for r in groups[g]], "token_ids": tok,
                           "token_probs": [float(p) for p in probs[g, :c]], "pseudo_caption": decode_tokens(tok, captioner)}
    return out


def write_csv(path: str, grouped: Dict, result: Dict[str, dict]) -> int:
    """The reference's CSV: header `episode_id, object_id, pseudo_caption`, one row per (episode, object) in `grouped` order."""
    rows = 0
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(CSV_HEADER)
        for k in grouped:
            if str(k) in result:
                w.writerow([k[0], k[1], result[str(k)]["pseudo_caption"]])
                rows += 1
    return rows


def build_captioner(args):
    from .utils.utils import Configuration
    from .utils.utils_captioner import select_captioner
    kw = dict(arch_name=args.arch_name, model_name=args.model or DEFAULT_MODELS[args.arch_name], height=224, width=224, dtype=args.dtype,
              batch_size=args.batch_size, streams=args.streams, device=args.device)
    return select_captioner(Configuration(**kw).captioner).eval()


def main(argv=None, captioner=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--file_path", required=True, help="directory of pseudo-label records (*.npz)")
    ap.add_argument("--output_csv_path", required=True)
    ap.add_argument("--arch_name", required=True, choices=sorted(DEFAULT_MODELS))
    ap.add_argument("--model", default=None, help="checkpoint directory / name (default: the architecture's published checkpoint)")
    ap.add_argument("--th", type=float, default=0.25)
    ap.add_argument("--dtype", default=None)
    ap.add_argument("--batch_size", type=int, default=256)
    ap.add_argument("--streams", type=int, default=3)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    from ..pseudocaptioner import group_records
    grouped = group_records(sorted(glob.glob(os.path.join(args.file_path, "*.npz"))), apply_filter=False)
    captioner = captioner or build_captioner(args)
    result = fused_pseudo_captions(grouped, captioner, th=args.th)
    rows = write_csv(args.output_csv_path, grouped, result)
    print(f"{rows} pseudo-captions -> {args.output_csv_path}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
