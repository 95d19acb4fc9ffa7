#!/usr/bin/env python
"""What scoring given captions costs against generating them (GPU box only): BLIP-base geometry, procedural weights, "f32s".

    python tools/bench_score_captions.py            256 pairs of 20 tokens: `score` against `generate` of the same frames at full
                                                    length (no EOS boost, early exit off), and 32 images x 8 candidates against the
                                                    same 256 captions as pairs - what sharing the image side buys
    python tools/bench_score_captions.py --trace    a few `score` calls of the 256 pairs and nothing else: the program of a
                                                    `rocprofv3 --kernel-trace --stats` run (tools/summarize_prof.py)
    python tools/bench_score_captions.py --tiny     the fixture geometry, to rehearse the tool

One process; the configurations alternate inside each of --rounds rounds (drift of the box hits all alike), a round times --iters
calls between two device events after a warm-up call, and the record holds the median over the rounds with the smallest and
largest round.  Lines are appended to profiles/score_bench.jsonl.  The one relation to check: `score` of a pass does a subset of
`generate`'s work (one prefill against 19 steps, the same head rows), so its median must not exceed `generate`'s; the tool says so
in the record (`score_not_slower`) and gates nothing.
    python tools/bench_score_captions.py --blip2    BLIP-2 at full depth (OPT-2.7b geometry, procedural weights), bf16: one crop x 5
                                                    candidates x 20 tokens scored, against a 5-beam `generate` of 20 new tokens
                                                    (--blip2 --trace: a few such score calls alone; --blip2 --tiny: the fixture geometry)"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from embodied_captioning_amd.config import BlipArch  # noqa: E402
from embodied_captioning_amd.engine import CaptionerEngine  # noqa: E402
from embodied_captioning_amd.weights import procedural_blip_state_dict, synthetic_pixels  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "score_bench.jsonl")


def emit(rec):
    rec["tool"] = "tools/bench_score_captions.py"
    print(json.dumps(rec), flush=True)
    with open(OUT, "a") as f:
        f.write(json.dumps(rec) + "\n")


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main_blip2(a):
    from embodied_captioning_amd.config import Blip2Arch
    from embodied_captioning_amd.weights import procedural_blip2_state_dict
    arch = Blip2Arch.tiny() if a.tiny else Blip2Arch()
    C, L = 5, min(a.L, arch.max_new_tokens) + 1                    # BOS + 20 tokens
    sd = procedural_blip2_state_dict(arch, 0, eos_boost=0.0)
    px = synthetic_pixels(1, arch.image_size, seed=0).cuda()
    g = np.random.default_rng(0)
    ok = np.array([i for i in range(min(arch.vocab, 50000)) if i not in (arch.bos, arch.eos, arch.pad, arch.image_token)])
    ids = ok[g.integers(0, len(ok), size=(C, L))].astype(np.int32)
    ids[:, 0] = arch.bos
    lens = np.full(C, L, dtype=np.int32)
    eng = CaptionerEngine(arch, dtype="bf16", max_batch=4, max_beams=C, max_len=L - 1)
    eng.load_state_dict(sd)
    eng.set_early_exit(0)
    cfgs = {"score_candidates": lambda: eng.score(px, ids, lens, captions_per_image=C),
            "generate_5_beams": lambda: eng.generate(px, num_beams=C, max_length=L - 1)}
    if a.trace:
        for _ in range(4):
            cfgs["score_candidates"]()
        torch.cuda.synchronize()
        return
    ms = {k: [] for k in cfgs}
    for _ in range(a.rounds):
        for k, fn in cfgs.items():
            ms[k].append(timed(fn, a.iters))
    eng.score(px, ids, lens, captions_per_image=C)
    med = {k: statistics.median(v) for k, v in ms.items()}
    emit({"what": "blip2 score vs 5 beams", "arch": "tiny" if a.tiny else "opt-2.7b geometry", "dtype": "bf16", "crops": 1, "candidates": C,
          "tokens": L - 1, "rounds": a.rounds, "iters": a.iters, "score_passes": eng.last_score_passes,
          "ms": {k: {"median": round(med[k], 3), "min": round(min(v), 3), "max": round(max(v), 3)} for k, v in ms.items()},
          "score_over_beams": round(med["score_candidates"] / med["generate_5_beams"], 4)})
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--candidates", type=int, default=8)
    ap.add_argument("--len", type=int, default=20, dest="L")
    ap.add_argument("--dtype", default="f32s")
    ap.add_argument("--tiny", action="store_true")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--blip2", action="store_true")
    a = ap.parse_args()
    if a.blip2:
        return main_blip2(a)
    arch = BlipArch.tiny() if a.tiny else BlipArch()
    N, C, L = a.pairs, a.candidates, a.L
    assert N % C == 0
    sd = procedural_blip_state_dict(arch, 0, eos_boost=0.0)
    px = synthetic_pixels(N, arch.image_size, seed=0).cuda()
    g = np.random.default_rng(0)
    ok = np.array([i for i in range(arch.vocab) if i not in (arch.bos, arch.eos, arch.pad)])
    ids = ok[g.integers(0, len(ok), size=(N, L))].astype(np.int32)
    ids[:, 0] = arch.bos
    lens = np.full(N, L, dtype=np.int32)
    eng = CaptionerEngine(arch, dtype=a.dtype, max_batch=N, max_beams=1, max_len=L, max_score_rows=N * (L - 1))
    eng.load_state_dict(sd)
    eng.set_early_exit(0)
    cfgs = {"score_pairs": lambda: eng.score(px, ids, lens),
            "generate": lambda: eng.generate(px, max_length=L),
            "score_candidates": lambda: eng.score(px[: N // C], ids, lens, captions_per_image=C)}
    if a.trace:
        for _ in range(4):
            cfgs["score_pairs"]()
        torch.cuda.synchronize()
        assert eng.last_score_passes == 1
        return
    ms = {k: [] for k in cfgs}
    for _ in range(a.rounds):
        for k, fn in cfgs.items():
            ms[k].append(timed(fn, a.iters))
    eng.score(px, ids, lens)
    passes = eng.last_score_passes
    gen_steps = int(eng.generate(px, max_length=L)["lengths"].min())
    med = {k: statistics.median(v) for k, v in ms.items()}
    emit({"what": "blip score vs generate", "arch": "tiny" if a.tiny else "base", "dtype": a.dtype, "pairs": N, "L": L, "candidates": C,
          "rounds": a.rounds, "iters": a.iters, "score_passes": passes, "shortest_generated_caption": gen_steps,
          "ms": {k: {"median": round(med[k], 3), "min": round(min(v), 3), "max": round(max(v), 3)} for k, v in ms.items()},
          "score_not_slower": bool(med["score_pairs"] <= med["generate"]),
          "candidates_over_pairs": round(med["score_candidates"] / med["score_pairs"], 4)})
    eng.close()


if __name__ == "__main__":
    main()
