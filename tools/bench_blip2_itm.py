#!/usr/bin/env python
"""Throughput of the BLIP-2 image-text scorer (the `--method blip2_itm | blip2_itc` pseudo-caption step) on procedural weights:
pairs/s per compute mode and image size for n pairs, ITM and ITC, (a) from normalised tensors, (b) from BGR frames + boxes through
the device crop / resize.  Device events after warm-up, median of --iters; `cap_device_bytes` of the engine; the `cap_profile`
kernel breakdown of one ITM step.  Two same-process comparisons:

  * n pairs in one call against n one-pair calls (the reference scores one pair per call) - `one_call_ms` / `per_pair_calls_ms`;
  * the two-segment self-attention kernel against the same pass expressed with the existing generic attention launcher on
    full-length unmasked rows (64 rows per pair: `cap_op_generic_attention`, i.e. the key-parallel generic kernel that
    `run_qformer`'s self-attention runs on), the two alternating call by call - a timing partner only, it is not the same
    function (no per-pair length) and nothing in the product path calls it.

One JSON line per measurement, appended to --out.  `--trace-step MODE:SIZE` instead runs two warm-up steps and `--iters` ITM steps
of --batch pairs and nothing else: the program to put after `rocprofv3 --kernel-trace --stats --`.

    python tools/bench_blip2_itm.py [--modes f32s,bf16,f32] [--pairs 256,1024] [--sizes 224,364] [--layers 39,12] [--iters 3]
"""
from __future__ import annotations

import argparse
import ctypes as C
import dataclasses
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from embodied_captioning_amd import _native as N  # noqa: E402
from embodied_captioning_amd.config import Blip2ItmArch  # noqa: E402
from embodied_captioning_amd.engine import _DTYPES, Blip2ItmEngine  # noqa: E402
from embodied_captioning_amd.preprocess import crop_resize_u8_frames  # noqa: E402
from embodied_captioning_amd.weights import _draw, blip2_itm_param_specs, procedural_blip2_itm_state_dict  # noqa: E402


def workload(a: Blip2ItmArch, n: int, seed: int = 0):
    """n pairs: boxes on 1280 x 720 BGR frames (3 boxes per frame), ragged captions of 6..24 tokens."""
    rng = np.random.default_rng(seed)
    nf = (n + 2) // 3
    frame = rng.integers(0, 256, size=(720, 1280, 3), dtype=np.uint8)
    frames = [np.roll(frame, 7 * i, axis=1) for i in range(nf)]
    rects = []
    for _ in range(nf):
        rs = []
        for _ in range(3):
            x1, y1 = int(rng.integers(0, 1000)), int(rng.integers(0, 500))
            rs.append((x1, y1, x1 + int(rng.integers(40, 280)), y1 + int(rng.integers(40, 220))))
        rects.append(rs)
    lens = rng.integers(6, 25, size=n)
    ids = np.zeros((n, int(lens.max())), dtype=np.int32)
    for b in range(n):
        ids[b, :lens[b]] = rng.integers(3, a.vocab, size=lens[b])
    return frames, rects, torch.from_numpy(ids), torch.from_numpy(lens.astype(np.int32))


def timed(fn, iters: int, warmup: int = 2):
    """-> (median ms, all ms) of fn() by device events."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), [round(v, 3) for v in ms]


def score(eng: Blip2ItmEngine, px, ids, lens, head: str, batch: int):
    out = []
    for i in range(0, px.shape[0], batch):
        eng.encode_images(px[i:i + batch])
        L = int(lens[i:i + batch].max())
        if head == "itm":
            out.append(eng.itm(ids[i:i + batch, :L], lens[i:i + batch])[1])
        else:
            out.append(eng.itc_scores(eng.itc_image_features(), eng.itc_text_features(ids[i:i + batch, :L], lens[i:i + batch])))
    return out


def attention_pair(mode: str, B: int, H: int, iters: int, emit):
    """The new kernel on [32 queries | 32 text rows, ragged lengths] against the generic kernel on 64 unmasked rows per pair."""
    lib = N.load_library()
    dt = _DTYPES[mode]
    tdt = torch.bfloat16 if mode == "bf16" else torch.float32
    W = H * 64
    g = torch.Generator(device="cuda").manual_seed(0)
    qkv = torch.randn((B * 64, 3 * W), device="cuda", generator=g).to(tdt)
    qq, qt = qkv[:B * 32].contiguous(), qkv[B * 32:].contiguous()
    lens = torch.randint(6, 25, (B,), device="cuda", dtype=torch.int32, generator=g)
    full = torch.full((B,), 32, device="cuda", dtype=torch.int32)
    esz = 2 if mode == "bf16" else 4
    cq = torch.empty(B * 32 * W * esz, dtype=torch.uint8, device="cuda")
    ct = torch.empty_like(cq)
    cf = torch.empty(B * 64 * W * esz, dtype=torch.uint8, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731

    def two_seg(ln):
        return lambda: N.check(lib.cap_op_itm_self_attention(dt, p(qq), p(qt), p(ln), p(cq), p(ct), B, 32, 32, H, s), "cap_op_itm_self_attention")

    def generic():
        N.check(lib.cap_op_generic_attention(dt, p(qkv), p(cf), B, 64, H, 64, s), "cap_op_generic_attention")

    def one(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    fns = dict(two_segment_ragged_ms=two_seg(lens), two_segment_full_ms=two_seg(full), generic_kp_full_unmasked_ms=generic)
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(max(iters * 5, 15)):          # alternating: neither kernel gets the warmer clocks or caches
        for k, fn in fns.items():
            ms[k].append(one(fn))
    emit(dict(kind="self_attention_pair", mode=mode, pairs=B, heads=H, reps=len(ms["two_segment_full_ms"]),
              **{k: round(float(np.median(v)), 4) for k, v in ms.items()},
              **{k.replace("_ms", "_min_ms"): round(float(np.min(v)), 4) for k, v in ms.items()}))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="f32s,bf16,f32")
    ap.add_argument("--pairs", default="256,1024")
    ap.add_argument("--sizes", default="224,364")
    ap.add_argument("--layers", default="39,12", help="ViT-g, Q-Former layers (the production model: 39,12)")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256, help="micro-batch of the engine (pairs per call)")
    ap.add_argument("--single", type=int, default=32, help="pairs of the one-call / per-pair-calls comparison")
    ap.add_argument("--profile", action="store_true", help="cap_profile breakdown of one ITM and one ITC step per (mode, size)")
    ap.add_argument("--trace-step", default=None, help="MODE:SIZE - only warm-up + --iters ITM steps of --batch pairs (for rocprofv3)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blip2_itm_bench.jsonl"))
    args = ap.parse_args()
    vl, ql = (int(v) for v in args.layers.split(","))
    if args.trace_step:
        mode, size = args.trace_step.split(":")
        a = Blip2ItmArch(v_layers=vl, q_layers=ql, image_size=int(size))
        eng = Blip2ItmEngine(a, dtype=mode, max_batch=args.batch)
        eng.load_state_dict(procedural_blip2_itm_state_dict(a, 0))
        frames, rects, ids, lens = workload(a, args.batch)
        u8 = crop_resize_u8_frames(frames, rects, a.image_size, bgr=True, device="cuda", center_crop=False)[:args.batch]
        for _ in range(2 + args.iters):
            score(eng, u8, ids, lens, "itm", args.batch)
        torch.cuda.synchronize()
        print(f"trace-step: {2 + args.iters} ITM steps of {args.batch} pairs, {mode}, {size} px")
        eng.close()
        return
    f = open(args.out, "a")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        f.write(line + "\n")
        f.flush()

    base = Blip2ItmArch(v_layers=vl, q_layers=ql)
    sd = procedural_blip2_itm_state_dict(base, 0)
    pos_name = "vision_model.embeddings.position_embedding"
    for size in (int(v) for v in args.sizes.split(",")):
        a = dataclasses.replace(base, image_size=size)
        spec = next(t for t in blip2_itm_param_specs(a) if t[0] == pos_name)
        sd[pos_name] = torch.from_numpy(_draw(0, *spec))
        for mode in args.modes.split(","):
            eng = Blip2ItmEngine(a, dtype=mode, max_batch=args.batch)
            eng.load_state_dict(sd)
            common = dict(mode=mode, image_size=size, tokens=a.n_tokens, v_layers=vl, q_layers=ql, batch=args.batch,
                          device_bytes=eng.device_bytes, weights="procedural")
            for n in (int(v) for v in args.pairs.split(",")):
                frames, rects, ids, lens = workload(a, n)
                u8 = crop_resize_u8_frames(frames, rects, size, bgr=True, device="cuda", center_crop=False)[:n]
                px = ((u8.float() / 255.0 - torch.tensor(eng_mean(), device="cuda")) / torch.tensor(eng_std(), device="cuda")).permute(0, 3, 1, 2).contiguous()
                for head in ("itm", "itc"):
                    ms, all_ms = timed(lambda: score(eng, px, ids, lens, head, args.batch), args.iters)
                    emit(dict(kind="pairs", head=head, input="normalised", pairs=n, ms=round(ms, 3), ms_all=all_ms, pairs_per_s=round(n / ms * 1e3, 1), **common))

                    def from_frames():
                        c = crop_resize_u8_frames(frames, rects, size, bgr=True, device="cuda", center_crop=False)[:n]
                        return score(eng, c, ids, lens, head, args.batch)
                    ms, all_ms = timed(from_frames, args.iters)
                    emit(dict(kind="pairs", head=head, input="frames+boxes", pairs=n, ms=round(ms, 3), ms_all=all_ms, pairs_per_s=round(n / ms * 1e3, 1), **common))
            # n pairs in one call against n one-pair calls
            k = args.single
            frames, rects, ids, lens = workload(a, k, seed=1)
            u8 = crop_resize_u8_frames(frames, rects, size, bgr=True, device="cuda", center_crop=False)[:k]
            for head in ("itm", "itc"):
                one, _ = timed(lambda: score(eng, u8, ids, lens, head, k), args.iters)
                per, _ = timed(lambda: score(eng, u8, ids, lens, head, 1), args.iters)
                emit(dict(kind="one_call_vs_per_pair", head=head, pairs=k, one_call_ms=round(one, 3), per_pair_calls_ms=round(per, 3),
                          speedup=round(per / one, 2), **common))
            if args.profile:
                frames, rects, ids, lens = workload(a, args.batch)
                u8 = crop_resize_u8_frames(frames, rects, size, bgr=True, device="cuda", center_crop=False)[:args.batch]
                for head in ("itm", "itc"):
                    score(eng, u8, ids, lens, head, args.batch)
                    eng.profile(True)
                    score(eng, u8, ids, lens, head, args.batch)
                    rep = eng.profile_report()
                    eng.profile(False)
                    tot = sum(v["ms"] for v in rep.values())
                    emit(dict(kind=f"profile_{head}_step", pairs=args.batch, total_ms=round(tot, 3),
                              kernels={k2: round(v["ms"], 3) for k2, v in sorted(rep.items(), key=lambda kv: -kv[1]["ms"])}, **common))
            eng.close()
    for mode in args.modes.split(","):
        attention_pair(mode, 256, base.q_heads, args.iters, emit)
    f.close()


def eng_mean():
    from embodied_captioning_amd.engine import OPENAI_CLIP_MEAN
    return list(OPENAI_CLIP_MEAN)


def eng_std():
    from embodied_captioning_amd.engine import OPENAI_CLIP_STD
    return list(OPENAI_CLIP_STD)


if __name__ == "__main__":
    main()
