#!/usr/bin/env python
"""What splitting a call at the image state costs and buys (GPU box only): procedural weights, early exit off.

    python tools/bench_image_state.py            BLIP-base geometry, "f32s" (KV16 cross cache), 256 rows, max_length 20:
                                                 `generate(pixels)`, `image_state(pixels)`, `generate(state)`, and a plain
                                                 device-to-device `copy_` of the state's bytes (what the two copy kernels are set against)
    python tools/bench_image_state.py --blip2    BLIP-2 at full depth (OPT-2.7b geometry), bf16, 8 crops, 20 new tokens: the same calls
    python tools/bench_image_state.py --trace    a few `image_state` and `generate(state)` calls and nothing else: the program of a
                                                 `rocprofv3 --kernel-trace --stats` run (tools/summarize_prof.py; kernels
                                                 image_state_pack_kernel / image_state_unpack_kernel)
    python tools/bench_image_state.py --tiny     the fixture geometry, to rehearse the tool

One process; every shape is warmed up, the configurations alternate inside each of --rounds rounds (drift of the box hits all alike),
a round times --iters calls between two device events, and the record holds the median over the rounds with the smallest and largest
round.  Lines are appended to profiles/image_state_bench.jsonl.  `split_cost_ms` = image_state + generate(state) - generate(pixels)
stands next to the round-to-round spread of generate(pixels), which is what it has to be told apart from.  The two copy kernels are
also timed by the library's own event pairs (`profile_report`: state_export / state_import) in a pass of their own, and set against the
plain copy of the same bytes (`export_over_copy`, `import_over_copy`).  The one relation to check: generate(state) does a subset of
generate(pixels)' work, so its median must be the smaller; the tool says so in the record (`state_is_faster`) and gates nothing."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from embodied_captioning_amd.config import Blip2Arch, BlipArch  # noqa: E402
from embodied_captioning_amd.engine import CaptionerEngine  # noqa: E402
from embodied_captioning_amd.weights import procedural_blip2_state_dict, procedural_blip_state_dict, synthetic_pixels  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "image_state_bench.jsonl")


def emit(rec):
    rec["tool"] = "tools/bench_image_state.py"
    print(json.dumps(rec), flush=True)
    with open(OUT, "a") as f:
        f.write(json.dumps(rec) + "\n")


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rows", type=int, default=0, help="images per call (default 256; --blip2: 8)")
    ap.add_argument("--len", type=int, default=20, dest="L")
    ap.add_argument("--dtype", default="")
    ap.add_argument("--tiny", action="store_true")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--blip2", action="store_true")
    a = ap.parse_args()
    if a.blip2:
        arch = Blip2Arch.tiny() if a.tiny else Blip2Arch()
        sd, dtype, B = procedural_blip2_state_dict(arch, 0, eos_boost=0.0), a.dtype or "bf16", a.rows or 8
        L = min(a.L, arch.max_new_tokens)
    else:
        arch = BlipArch.tiny() if a.tiny else BlipArch()
        sd, dtype, B, L = procedural_blip_state_dict(arch, 0, eos_boost=0.0), a.dtype or "f32s", a.rows or 256, a.L
    px = synthetic_pixels(B, arch.image_size, seed=0).cuda()
    eng = CaptionerEngine(arch, dtype=dtype, max_batch=B, max_beams=1, max_len=L)
    eng.load_state_dict(sd)
    eng.set_early_exit(0)
    state = eng.image_state(px)
    spare = torch.empty_like(state)
    cfgs = {"generate_pixels": lambda: eng.generate(px, max_length=L),
            "image_state": lambda: eng.image_state(px),
            "generate_state": lambda: eng.generate(state, max_length=L),
            "plain_copy": lambda: spare.copy_(state)}
    for fn in cfgs.values():          # every shape once before anything is timed
        fn()
    torch.cuda.synchronize()
    if a.trace:
        for _ in range(4):
            cfgs["image_state"]()
            cfgs["generate_state"]()
        torch.cuda.synchronize()
        return
    same = all(torch.equal(x, y) for x, y in zip(eng.generate(px, max_length=L).values(), eng.generate(state, max_length=L).values()))
    ms = {k: [] for k in cfgs}
    for _ in range(a.rounds):
        for k, fn in cfgs.items():
            ms[k].append(timed(fn, a.iters))
    # the two copy kernels alone, by the library's event pairs, in a pass of their own
    eng.profile(True)
    for _ in range(a.iters):
        cfgs["image_state"]()
        cfgs["generate_state"]()
    rep = eng.profile_report()
    eng.profile(False)
    kern = {k: rep[k]["ms"] / rep[k]["launches"] for k in ("state_export", "state_import")}
    med = {k: statistics.median(v) for k, v in ms.items()}
    nbytes = int(state.numel())
    emit({"what": "image state: split cost and copy kernels", "arch": ("blip2 " if a.blip2 else "blip ") + ("tiny" if a.tiny else "full geometry"),
          "dtype": dtype, "cross_cache": eng.cross_cache_kind, "rows": B, "max_length": L, "rounds": a.rounds, "iters": a.iters,
          "state_bytes_per_image": eng.image_state_bytes, "state_bytes": nbytes, "same_outputs": bool(same),
          "ms": {k: {"median": round(med[k], 3), "min": round(min(v), 3), "max": round(max(v), 3)} for k, v in ms.items()},
          "split_cost_ms": round(med["image_state"] + med["generate_state"] - med["generate_pixels"], 3),
          "generate_pixels_spread_ms": round(max(ms["generate_pixels"]) - min(ms["generate_pixels"]), 3),
          "state_is_faster": bool(med["generate_state"] < med["generate_pixels"]),
          "kernel_ms": {k: round(v, 4) for k, v in kern.items()},
          "kernel_GBps_read_plus_write": {k: round(2 * nbytes / v / 1e6, 1) for k, v in kern.items()},
          "plain_copy_GBps_read_plus_write": round(2 * nbytes / med["plain_copy"] / 1e6, 1),
          "export_over_copy": round(kern["state_export"] / med["plain_copy"], 3),
          "import_over_copy": round(kern["state_import"] / med["plain_copy"], 3)})
    eng.close()


if __name__ == "__main__":
    main()
