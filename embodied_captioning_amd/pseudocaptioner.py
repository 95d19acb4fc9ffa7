"""Pseudo-caption scoring - the reference's `PseudoCaptioner` (experimenting_env/captioner/pseudocaptioner.py:125-154 grouping,
:345-357 crop + score) with `--method clip` (:463-489 selection by CLIP score) and `--method blip2_itm | blip2_itc` (:193-308, :491-
`blip2_score`: the BLIP-2 matching probability / contrastive similarity of every caption), every pair of every group scored in
batched device calls (captioner/clip_scorer.py, captioner/blip2_itm_scorer.py) instead of one model call per pair.

    python -m embodied_captioning_amd.pseudocaptioner --file_path DIR --output_csv_path OUT.json --method clip
    python -m embodied_captioning_amd.pseudocaptioner --file_path DIR --output_csv_path OUT.json --method blip2_itm [--model DIR]

    python -m embodied_captioning_amd.pseudocaptioner --file_path DIR --output_csv_path OUT.json --method blip_ll [--model DIR]

`--method blip_ll` has no counterpart in the reference: the selector is the BLIP captioner's OWN likelihood of each caption given each
crop of the object (captioner/likelihood_scorer.py), so no second model is needed; `--method blip2_ll` is the same under BLIP-2.
`--method sbert [--model all-MiniLM-L6-v2]` has none either: no image is read, the pseudo-caption of an object is the MEDOID of its captions
under the sentence encoder - the caption with the largest mean cosine to the object's other captions, repeats counted
(captioner/sentence_encoder.py `caption_statistics`, csrc/similarity.hip).
The reference's other methods (`llm`, `mobileclip`, `openclip` ViT-bigG-14) are refused by name.
"""
from __future__ import annotations

import argparse
import glob
import json
import os
from typing import Dict, List, Sequence, Tuple

import numpy as np

from .distributed import filter_caption
from .pseudolabeler import expand_box

REFUSED_METHODS = ("llm", "mobileclip", "openclip")
BLIP2_METHODS = {"blip2_itm": "itm", "blip2_itc": "itc"}          # --method -> the scorer's head
LIKELIHOOD_METHODS = {"blip_ll": "blip", "blip2_ll": "blip2"}     # --method -> the captioner family whose likelihood selects
DEFAULT_MODELS = {"clip": "openai/clip-vit-base-patch32", "blip2_itm": "Salesforce/blip2-itm-vit-g-coco",
                  "blip2_itc": "Salesforce/blip2-itm-vit-g-coco", "blip_ll": "Salesforce/blip-image-captioning-base",
                  "blip2_ll": "Salesforce/blip2-opt-2.7b", "sbert": "all-MiniLM-L6-v2"}
REFERENCE_FRAME = (1280, 1280)       # the reference's hard-coded image size for expand_box (:346)


def crop_rect(pred_box, frame_shape, expand_factor: float = 0.1, image_size=REFERENCE_FRAME) -> Tuple[int, int, int, int]:
    """The rectangle the reference's numpy slice `image[y1:y2, x1:x2]` keeps (:345-348): expand_box against the hard-coded
    (1280, 1280), then clamped to the real frame as a slice clamps (the device crop would zero-pad instead)."""
    x1, y1, x2, y2 = (int(v) for v in expand_box(pred_box, expand_factor, image_size))
    H, W = int(frame_shape[0]), int(frame_shape[1])
    x1, x2 = min(max(x1, 0), W), min(max(x2, 0), W)
    y1, y2 = min(max(y1, 0), H), min(max(y2, 0), H)
    if x2 <= x1 or y2 <= y1:
        raise ValueError(f"box {list(map(float, pred_box))} leaves nothing of a {W} x {H} frame after the reference's slice")
    return x1, y1, x2, y2


def host_crops(frames: Sequence[np.ndarray], rects: Sequence[Sequence[Tuple[int, int, int, int]]]) -> List[np.ndarray]:
    """The reference's crop itself (:345-348): numpy slice of each (already clamped) rectangle, BGR -> RGB; frame-major, unresized."""
    return [np.ascontiguousarray(f[y1:y2, x1:x2, ::-1]) for f, rs in zip(frames, rects) for x1, y1, x2, y2 in rs]


def device_crops(scorer, center_crop: bool = True):
    """The default crop step: every box of every frame cut, swapped to RGB and resized to the scorer's image size on the device in
    one go (bit-exact with Pillow) -> uint8 [n, S, S, 3], frame-major.  center_crop: HF CLIPImageProcessorPil's geometry (the CLIP
    scorer); False: the straight resize to S x S of LAVIS `blip_image_eval` (the BLIP-2 scorer)."""
    from .preprocess import crop_resize_u8_frames

    def crop(frames, rects):
        return crop_resize_u8_frames(frames, rects, scorer.arch.image_size, bgr=True, device=scorer.device, center_crop=center_crop,
                                     geometry="hf")
    return crop


def _score_all_pairs(grouped: Dict, scorer, expand_factor, image_size, crop, **score_kw):
    """Every pair of every group in ONE `scorer.score_pairs(images, captions, **score_kw)` call -> (keys, float64 scores in group /
    input order), or (keys, None) when there is no pair."""
    keys = list(grouped)
    frames, rects, caps, owner = [], [], [], []
    frame_idx = {}
    for k in keys:
        for inst in grouped[k]:
            img = inst["image"]
            fi = frame_idx.setdefault(id(img), len(frames))
            if fi == len(frames):
                frames.append(np.ascontiguousarray(img))
                rects.append([])
            rects[fi].append(crop_rect(inst["pred_box"], img.shape, expand_factor, image_size))
            caps.append(inst["caption"])
            owner.append((fi, len(rects[fi]) - 1))
    if not caps:
        return keys, None
    images = crop(frames, rects)
    first = np.cumsum([0] + [len(r) for r in rects])
    order = [int(first[fi]) + j for fi, j in owner]               # pair i's image in the frame-major crops
    if hasattr(images, "index_select"):
        import torch
        images = images.index_select(0, torch.tensor(order, device=images.device))
    else:
        images = [images[i] for i in order]
    sc = scorer.score_pairs(images, caps, **score_kw)
    return keys, np.asarray(sc.double().cpu() if hasattr(sc, "cpu") else sc, dtype=np.float64)


def clip_pseudo_captions(grouped: Dict, scorer, expand_factor: float = 0.1, image_size=REFERENCE_FRAME, crop=None) -> Dict[str, dict]:
    """grouped: (episode, object) -> [{'image': BGR uint8 frame, 'pred_box': (x1, y1, x2, y2), 'caption': str}, ...].
    -> {str(key): {'captions_list': [[score, caption], ...] (by score, descending, stable), 'pseudocaption': [score, caption]}}
    as :463-483 builds it.  crop(frames, rects) -> the images of all boxes, frame-major (default `device_crops(scorer)`: one
    batched device crop + resize); then one `scorer.score_pairs(images, captions)` call for every pair of every group."""
    keys, scores = _score_all_pairs(grouped, scorer, expand_factor, image_size, crop or device_crops(scorer))
    if scores is None:
        return {}
    out: Dict[str, dict] = {}
    i = 0
    for k in keys:
        lst = []
        for inst in grouped[k]:
            lst.append([float(scores[i]), inst["caption"]])
            i += 1
        if not lst:
            continue
        lst.sort(key=lambda x: x[0], reverse=True)       # list.sort is stable: equal scores keep input order
        out[str(k)] = {"captions_list": lst, "pseudocaption": list(lst[0])}
    return out


def blip2_pseudo_scores(grouped: Dict, scorer, head: str = "itm", expand_factor: float = 0.1, image_size=REFERENCE_FRAME, crop=None) -> Dict[str, dict]:
    """grouped as for `clip_pseudo_captions` -> {str(key): {'captions': [...], 'scores': [...]}} in INPUT order (no sorting, no
    'pseudocaption' key): what the reference's `blip2_score` writes for `--method blip2_itm` (head "itm": the matching
    probability) and `blip2_itc` (head "itc": the contrastive similarity).  crop(frames, rects) defaults to the straight device
    resize of `blip_image_eval`; then one `scorer.score_pairs(images, captions, head=head)` call for every pair of every group."""
    keys, scores = _score_all_pairs(grouped, scorer, expand_factor, image_size, crop or device_crops(scorer, center_crop=False), head=head)
    if scores is None:
        return {}
    out: Dict[str, dict] = {}
    i = 0
    for k in keys:
        n = len(grouped[k])
        if n:
            out[str(k)] = {"captions": [inst["caption"] for inst in grouped[k]], "scores": [float(v) for v in scores[i:i + n]]}
        i += n
    return out


def likelihood_pseudo_captions(grouped: Dict, scorer, expand_factor: float = 0.1, image_size=REFERENCE_FRAME, crop=None) -> Dict[str, dict]:
    """grouped as for `clip_pseudo_captions`; scorer: a `CaptionLikelihoodScorer` (anything with `score_matrix(images, captions) ->
    [n_images, n_captions]`).  Per object, every DISTINCT caption of the group (first occurrence order) is scored against EVERY crop
    of the group - one `score_matrix` call per group, each crop encoded once - and a caption's score is the mean over the crops of
    its mean token log-prob.  -> `clip_pseudo_captions`' structure, one entry per distinct caption: {str(key): {'captions_list':
    [[score, caption], ...] (by score, descending, stable), 'pseudocaption': [score, caption]}}."""
    crop = crop or device_crops(scorer, center_crop=False)
    keys = list(grouped)
    frames, rects, owner = [], [], {}
    frame_idx = {}
    for k in keys:
        owner[k] = []
        for inst in grouped[k]:
            img = inst["image"]
            fi = frame_idx.setdefault(id(img), len(frames))
            if fi == len(frames):
                frames.append(np.ascontiguousarray(img))
                rects.append([])
            rects[fi].append(crop_rect(inst["pred_box"], img.shape, expand_factor, image_size))
            owner[k].append((fi, len(rects[fi]) - 1))
    if not any(owner.values()):
        return {}
    images = crop(frames, rects)
    first = np.cumsum([0] + [len(r) for r in rects])
    out: Dict[str, dict] = {}
    for k in keys:
        if not owner[k]:
            continue
        order = [int(first[fi]) + j for fi, j in owner[k]]
        if hasattr(images, "index_select"):
            import torch
            imgs = images.index_select(0, torch.tensor(order, device=images.device))
        else:
            imgs = [images[i] for i in order]
        caps: List = []
        for inst in grouped[k]:
            if inst["caption"] not in caps:
                caps.append(inst["caption"])
        m = scorer.score_matrix(imgs, caps)
        m = np.asarray(m.double().cpu() if hasattr(m, "cpu") else m, dtype=np.float64).reshape(len(order), len(caps))
        lst = [[float(s), c] for s, c in zip(m.mean(axis=0), caps)]
        lst.sort(key=lambda x: x[0], reverse=True)       # list.sort is stable: equal scores keep first-occurrence order
        out[str(k)] = {"captions_list": lst, "pseudocaption": list(lst[0])}
    return out


def sbert_pseudo_captions(grouped: Dict, encoder) -> Dict[str, dict]:
    """grouped as for `clip_pseudo_captions` (only 'caption' is read); encoder: a `SentenceEncoder`.  Per object, every DISTINCT caption
    (first occurrence order) with its mean cosine to the object's other captions, repeats counted -> `clip_pseudo_captions`'
    structure: {str(key): {'captions_list': [[score, caption], ...] (by score, descending, stable), 'pseudocaption': [score,
    caption] = the medoid}}."""
    from .distributed import captions_frequency
    freq = captions_frequency({k: [inst["caption"] for inst in v] for k, v in grouped.items() if v})
    stats = encoder.caption_statistics(freq)
    out: Dict[str, dict] = {}
    for k, lst in freq.items():
        scored = [[float(s), c] for s, (_, c) in zip(stats[k]["row_mean"], lst)]
        scored.sort(key=lambda x: x[0], reverse=True)    # list.sort is stable: equal scores keep first-occurrence order
        out[str(k)] = {"captions_list": scored, "pseudocaption": list(scored[0])}
    return out


def _instances_fields(inst, idx):
    if isinstance(inst, dict):
        info, box, cap = inst["infos"][idx], inst["pred_boxes"][idx], inst["captions"][idx]
    else:
        info, box, cap = inst.infos[idx], inst.pred_boxes[idx], inst.captions[idx]
    if hasattr(box, "tensor"):                        # detectron2 Boxes row
        box = box.tensor[0]
    if hasattr(box, "numpy"):
        box = box.numpy()
    return info, np.asarray(box, dtype=np.float32), cap


def group_records(paths: Sequence[str], apply_filter: bool = True) -> Dict[Tuple, List[dict]]:
    """The `.npz` records of pseudolabeler.save_record -> (id_episode, id_object) -> [{'filename', 'image', 'pred_box', 'info',
    'caption'}, ...], captions with a banned word dropped (reference :125-154)."""
    grouped: Dict[Tuple, List[dict]] = {}
    for p in paths:
        rec = np.load(p, allow_pickle=True)["arr_0"].item()
        inst, rgb = rec["instances"], rec["image"]
        n = len(inst["captions"]) if isinstance(inst, dict) else len(inst.captions)
        for idx in range(n):
            info, box, cap = _instances_fields(inst, idx)
            if apply_filter and not filter_caption(cap):
                continue
            key = (info["id_episode"], info["id_object"])
            grouped.setdefault(key, []).append({"filename": p, "image": rgb, "pred_box": box, "info": info, "caption": cap})
    return grouped


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--file_path", required=True, help="directory of pseudo-label records (*.npz)")
    ap.add_argument("--output_csv_path", required=True, help="JSON output (the reference's name for it)")
    ap.add_argument("--method", default="clip")
    ap.add_argument("--model", default=None, help="checkpoint directory / cached hub id (default: the method's own; BLIP-2: HF format only)")
    ap.add_argument("--dtype", default="f32s")
    ap.add_argument("--batch_size", type=int, default=256)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    if args.method in REFUSED_METHODS:
        raise SystemExit(f"--method {args.method} is not supported here (it needs models this project does not run); "
                         f"use --method clip, blip2_itm or blip2_itc")
    if args.method not in ("clip", "sbert") and args.method not in BLIP2_METHODS and args.method not in LIKELIHOOD_METHODS:
        raise SystemExit(f"unknown --method {args.method!r}; supported: clip, blip2_itm, blip2_itc, blip_ll, blip2_ll, sbert")
    model = args.model or DEFAULT_MODELS[args.method]
    grouped = group_records(sorted(glob.glob(os.path.join(args.file_path, "*.npz"))))
    if args.method == "sbert":
        from .captioner.sentence_encoder import SentenceEncoder
        scorer = SentenceEncoder(model, device=args.device, dtype="f32", batch_size=min(args.batch_size, 64))
    elif args.method in LIKELIHOOD_METHODS:
        from .captioner.likelihood_scorer import CaptionLikelihoodScorer
        scorer = CaptionLikelihoodScorer(model, device=args.device, dtype=args.dtype, batch_size=min(args.batch_size, 32),
                                         family=LIKELIHOOD_METHODS[args.method])
    elif args.method == "clip":
        from .captioner.clip_scorer import ClipScorer
        scorer = ClipScorer(model, device=args.device, dtype=args.dtype, batch_size=args.batch_size)
    else:
        from .captioner.blip2_itm_scorer import Blip2ItmScorer
        scorer = Blip2ItmScorer(model, device=args.device, dtype=args.dtype, batch_size=args.batch_size)
    try:
        if args.method == "sbert":
            result = sbert_pseudo_captions(grouped, scorer)
        elif args.method in LIKELIHOOD_METHODS:
            result = likelihood_pseudo_captions(grouped, scorer)
        else:
            result = clip_pseudo_captions(grouped, scorer) if args.method == "clip" else blip2_pseudo_scores(grouped, scorer, BLIP2_METHODS[args.method])
    finally:
        scorer.close()
    print("Scoring completed. Saving scores to", args.output_csv_path)
    with open(args.output_csv_path, "w") as f:
        json.dump(result, f)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
