"""Pseudo-caption selection by CLIP score - the reference's `PseudoCaptioner` with `--method clip`
(experimenting_env/captioner/pseudocaptioner.py:125-154 grouping, :345-357 crop + score, :463-489 selection), every pair of every
group scored in batched device calls (captioner/clip_scorer.py) instead of one HF call per pair.

    python -m embodied_captioning_amd.pseudocaptioner --file_path DIR --output_csv_path OUT.json --method clip

Only `clip` is built: the reference's other methods (`llm`, `blip2_itm` / `blip2_itc` through LAVIS, `mobileclip`, `openclip`
ViT-bigG-14) are refused by name.
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

REFUSED_METHODS = ("llm", "blip2_itm", "blip2_itc", "mobileclip", "openclip")
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


def device_crops(scorer):
    """The default crop step: every box of every frame cut, swapped to RGB and resized to the scorer's image size on the device in
    one go, with HF CLIPImageProcessorPil's geometry (bit-exact with Pillow) -> uint8 [n, S, S, 3], frame-major."""
    from .preprocess import crop_resize_u8_frames

    def crop(frames, rects):
        return crop_resize_u8_frames(frames, rects, scorer.arch.image_size, bgr=True, device=scorer.device, center_crop=True,
                                     geometry="hf")
    return crop


def clip_pseudo_captions(grouped: Dict, scorer, expand_factor: float = 0.1, image_size=REFERENCE_FRAME, crop=None) -> Dict[str, dict]:
    """grouped: (episode, object) -> [{'image': BGR uint8 frame, 'pred_box': (x1, y1, x2, y2), 'caption': str}, ...].
    -> {str(key): {'captions_list': [[score, caption], ...] (by score, descending, stable), 'pseudocaption': [score, caption]}}
    as :463-483 builds it.  crop(frames, rects) -> the images of all boxes, frame-major (default `device_crops(scorer)`: one
    batched device crop + resize); then one `scorer.score_pairs(images, captions)` call for every pair of every group."""
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
        return {}
    images = (crop or device_crops(scorer))(frames, rects)
    first = np.cumsum([0] + [len(r) for r in rects])
    order = [int(first[fi]) + j for fi, j in owner]               # pair i's image in the frame-major crops
    if hasattr(images, "index_select"):
        import torch
        images = images.index_select(0, torch.tensor(order, device=images.device))
    else:
        images = [images[i] for i in order]
    sc = scorer.score_pairs(images, caps)
    scores = np.asarray(sc.double().cpu() if hasattr(sc, "cpu") else sc, dtype=np.float64)
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
    ap.add_argument("--model", default="openai/clip-vit-base-patch32")
    ap.add_argument("--dtype", default="f32s")
    ap.add_argument("--batch_size", type=int, default=256)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    if args.method in REFUSED_METHODS:
        raise SystemExit(f"--method {args.method} is not supported here (it needs models this project does not run); use --method clip")
    if args.method != "clip":
        raise SystemExit(f"unknown --method {args.method!r}; supported: clip")
    from .captioner.clip_scorer import ClipScorer
    grouped = group_records(sorted(glob.glob(os.path.join(args.file_path, "*.npz"))))
    scorer = ClipScorer(args.model, device=args.device, dtype=args.dtype, batch_size=args.batch_size)
    try:
        result = clip_pseudo_captions(grouped, scorer)
    finally:
        scorer.close()
    print("Scoring completed. Saving scores to", args.output_csv_path)
    with open(args.output_csv_path, "w") as f:
        json.dump(result, f)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
