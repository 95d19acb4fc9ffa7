#!/usr/bin/env python
"""Throughput of the CLIP scorer (the `--method clip` pseudo-caption step): pairs/s per compute mode for n pairs, (a) from BGR
frames + boxes through the device crop / resize, both towers and the paired logits (`pseudocaptioner.clip_pseudo_captions`'
device path), (b) the towers + logits alone on resized uint8 crops.  Device events after warm-up; prints the algorithmic FLOPs
from the shapes and the `cap_profile` kernel breakdown of one towers step.  One JSON line per (mode, n).

    python tools/bench_clip_score.py [--modes f32s,bf16,f32] [--pairs 256,1024] [--arch b32|tiny] [--iters 5]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from embodied_captioning_amd.config import ClipArch  # noqa: E402
from embodied_captioning_amd.engine import ClipEngine  # noqa: E402
from embodied_captioning_amd.preprocess import crop_resize_u8_frames  # noqa: E402
from embodied_captioning_amd.weights import procedural_clip_state_dict  # noqa: E402


def workload(a: ClipArch, n: int, seed: int = 0):
    """n pairs: boxes on 1280 x 720 BGR frames (3 boxes per frame), ragged captions of 8..24 tokens."""
    rng = np.random.default_rng(seed)
    nf = (n + 2) // 3
    frames = [rng.integers(0, 256, size=(720, 1280, 3), dtype=np.uint8) for _ in range(nf)]
    rects = []
    for _ in range(nf):
        rs = []
        for _ in range(3):
            x1, y1 = int(rng.integers(0, 1000)), int(rng.integers(0, 500))
            rs.append((x1, y1, x1 + int(rng.integers(40, 280)), y1 + int(rng.integers(40, 220))))
        rects.append(rs)
    lens = rng.integers(8, 25, size=n)
    L = int(lens.max())
    ids = np.full((n, L), a.eos_token_id, dtype=np.int32)
    for b in range(n):
        ids[b, 0] = a.bos_token_id
        ids[b, 1:lens[b] - 1] = rng.integers(1, 40000 if a.vocab > 40000 else a.vocab - 3, size=lens[b] - 2)
    return frames, rects, torch.from_numpy(ids), torch.from_numpy(lens.astype(np.int32))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="f32s,bf16,f32")
    ap.add_argument("--pairs", default="256,1024")
    ap.add_argument("--arch", default="b32")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256, help="micro-batch of the engine (pairs per tower call)")
    args = ap.parse_args()
    a = ClipArch() if args.arch == "b32" else ClipArch.tiny()
    sd = procedural_clip_state_dict(a, 0)
    for mode in args.modes.split(","):
        eng = ClipEngine(a, dtype=mode, max_batch=args.batch)
        eng.load_state_dict(sd)
        for n in (int(x) for x in args.pairs.split(",")):
            frames, rects, ids, lens = workload(a, n)
            ids_d, lens_d = ids.cuda(), lens.cuda()

            def towers(px):
                outs = []
                for i in range(0, n, args.batch):
                    img = eng.embed_images(px[i:i + args.batch])
                    txt = eng.embed_text(ids_d[i:i + args.batch], lens_d[i:i + args.batch])
                    outs.append(eng.logits(img, txt, paired=True))
                return torch.cat(outs)

            def full():
                px = crop_resize_u8_frames(frames, rects, a.image_size, bgr=True, center_crop=True, geometry="hf")[:n]
                return towers(px)

            px = crop_resize_u8_frames(frames, rects, a.image_size, bgr=True, center_crop=True, geometry="hf")[:n].contiguous()
            res = {"bench": "clip_score", "mode": mode, "pairs": n, "micro_batch": args.batch}
            for name, fn in (("towers", lambda: towers(px)), ("crop_to_logits", full)):
                for _ in range(2):
                    fn()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.iters):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                ms = e0.elapsed_time(e1) / args.iters
                res[f"{name}_ms"] = round(ms, 3)
                res[f"{name}_pairs_per_s"] = round(n / ms * 1e3, 1)
            tok = int(lens.sum())
            flops = n * a.image_flops() + tok * a.text_flops_per_token()
            res["gflop_per_image"] = round(a.image_flops() / 1e9, 3)
            res["mflop_per_caption_token"] = round(a.text_flops_per_token() / 1e6, 2)
            res["towers_tflops"] = round(flops / (res["towers_ms"] * 1e-3) / 1e12, 2)
            eng.profile(True)
            towers(px)
            rep = eng.profile_report()
            eng.profile(False)
            res["profile"] = {k: {"launches": v["launches"], "ms": round(v["ms"], 3)} for k, v in sorted(rep.items(), key=lambda kv: -kv[1]["ms"])}
            tot_v = sum(v["ms"] for k, v in rep.items() if k.startswith("clip_v_") or k == "clip_patchify")
            res["image_attention_share"] = round(rep.get("clip_v_attention", {"ms": 0})["ms"] / tot_v, 4) if tot_v else None
            print(json.dumps(res), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
