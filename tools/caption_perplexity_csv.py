#!/usr/bin/env python
"""Caption a folder of images, or the boxes of recorded frames, and write `filename, caption, perplexity` to a CSV - the file
the reference's per-crop perplexity script produces and its selection / analysis scripts read, made through the batched path
(`generate_batch(..., output_perplexity=True)`: pooled streams, dynamic batching, perplexity from the selection kernel).

    python tools/caption_perplexity_csv.py --images DIR --out captions.csv
    python tools/caption_perplexity_csv.py --npz frames.npz --out captions.csv

--npz: `frames` uint8 [F, H, W, 3] BGR and `boxes` float [N, 5] = (frame index, x1, y1, x2, y2); every box is expanded by
--expand (the pseudo-labeler's crop) and its row is named `frame<k>_box<j>`.
"""
import argparse
import csv
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

IMAGE_SUFFIXES = (".jpg", ".jpeg", ".png", ".bmp", ".webp")


def load_folder(path):
    from PIL import Image
    names = sorted(n for n in os.listdir(path) if n.lower().endswith(IMAGE_SUFFIXES))
    if not names:
        raise SystemExit(f"no image ({', '.join(IMAGE_SUFFIXES)}) under {path}")
    return names, [Image.open(os.path.join(path, n)).convert("RGB") for n in names]


def load_boxes(path, expand):
    from embodied_captioning_amd.pseudolabeler import crop_boxes
    with np.load(path) as z:
        frames, boxes = z["frames"], np.asarray(z["boxes"], dtype=np.float64).reshape(-1, 5)
    names, crops = [], []
    for k in range(frames.shape[0]):
        mine = boxes[boxes[:, 0] == k][:, 1:]
        crops += crop_boxes(frames[k], [tuple(b) for b in mine], expand)
        names += [f"frame{k}_box{j}" for j in range(len(mine))]
    if not crops:
        raise SystemExit(f"{path} holds no box")
    return names, crops


def write_csv(path, names, texts, perplexities):
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["filename", "caption", "perplexity"])
        for n, t, p in zip(names, texts, perplexities):
            w.writerow([n, t, repr(float(p))])


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--images", metavar="DIR")
    src.add_argument("--npz", metavar="FILE")
    ap.add_argument("--out", required=True)
    ap.add_argument("--arch", default="blip", help="blip | coca | blip2 (captioner.arch_name)")
    ap.add_argument("--model", default="Salesforce/blip-image-captioning-base", help="captioner.model_name (a local checkpoint "
                    "directory or name, or procedural-tiny:<seed>:<eos boost> for a weightless trial)")
    ap.add_argument("--dtype", default="f32s")
    ap.add_argument("--batch-size", type=int, default=256)
    ap.add_argument("--streams", type=int, default=3)
    ap.add_argument("--max-length", type=int, default=None)
    ap.add_argument("--expand", type=float, default=0.2)
    a = ap.parse_args(argv)
    from embodied_captioning_amd.captioner.utils.utils import Configuration
    from embodied_captioning_amd.captioner.utils.utils_captioner import select_captioner
    names, crops = load_folder(a.images) if a.images else load_boxes(a.npz, a.expand)
    kw = dict(arch_name=a.arch, model_name=a.model, height=224, width=224, dtype=a.dtype, batch_size=a.batch_size, streams=a.streams)
    if a.max_length:
        kw["max_new_tokens" if a.arch == "blip2" else "max_length"] = a.max_length
    model = select_captioner(Configuration(**kw).captioner).eval()
    out = model.generate_batch(crops, output_perplexity=True)
    write_csv(a.out, names, out["texts"], out["perplexities"].tolist())
    print(f"{len(names)} captions -> {a.out}")


if __name__ == "__main__":
    main()
