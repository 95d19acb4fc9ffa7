#!/usr/bin/env python
"""What beams cost for BLIP-2 (GPU box only): OPT-2.7b geometry at full depth, procedural weights, 20 new tokens, early exit off.

    python tools/bench_blip2_beams.py                  1 and 8 crops per call x 1 / 3 / 5 beams, bf16 and load_in_8bit
    python tools/bench_blip2_beams.py --ab-old         one crop, greedy, load_in_8bit: this build against lib/libcaptioner_old.so
                                                       (tools/build_old_lib.sh <parent revision>), both in this process
                                                       (with --grid: both measurements on one draw of the weights)
    python tools/bench_blip2_beams.py --trace-step     a few 5-beam one-crop int8 calls and nothing else: the program of a
                                                       `rocprofv3 --kernel-trace` run (tools/summarize_prof.py steps: the last call's steps)

Every figure: the configurations of a mode alternate inside each of --rounds rounds (so drift of the box hits all alike), a round
times --iters calls between two device events after a warm-up call, and the record holds the median over the rounds with the
smallest and largest round (the run-to-run spread).  --ab-old measures both creation orders of the two handles and, as the floor
under their difference, four handles of this build against one another.  Lines are appended to profiles/blip2_beam_bench.jsonl;
--process N tags them with the run they come from (the record holds several separate runs of --ab-old).
--tiny: the fixture geometry, to rehearse the tool."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from embodied_captioning_amd import _native as N  # noqa: E402
from embodied_captioning_amd.config import Blip2Arch  # noqa: E402
from embodied_captioning_amd.engine import CaptionerEngine  # noqa: E402
from embodied_captioning_amd.weights import procedural_blip2_state_dict, synthetic_pixels  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "blip2_beam_bench.jsonl")
OLD = os.path.join(ROOT, "embodied_captioning_amd", "lib", "libcaptioner_old.so")


PROCESS = None


def emit(rec):
    rec["tool"] = "tools/bench_blip2_beams.py"
    if PROCESS is not None:
        rec["process"] = PROCESS
    print(json.dumps(rec), flush=True)
    with open(OUT, "a") as f:
        f.write(json.dumps(rec) + "\n")


def engine(arch, sd, int8, batch, beams, lib_path=None):
    """An engine on this build, or on another build of the library (its own handle type and kernels, same process)."""
    if lib_path is None:
        eng = CaptionerEngine(arch, dtype="bf16", max_batch=batch, max_beams=beams, max_len=arch.max_new_tokens, weight_int8=int8)
    else:
        mine, path = N._lib, N.LIB_PATH
        other = C.CDLL(lib_path)
        newer = {k: N._SIGNATURES.pop(k) for k in [k for k in N._SIGNATURES if not hasattr(other, k)]}      # entry points it predates
        N._lib, N.LIB_PATH = None, lib_path
        try:
            eng = CaptionerEngine(arch, dtype="bf16", max_batch=batch, max_beams=beams, max_len=arch.max_new_tokens, weight_int8=int8)
        finally:
            N._lib, N.LIB_PATH = mine, path
            N._SIGNATURES.update(newer)
    eng.load_state_dict(sd)
    eng.set_early_exit(0)
    return eng


def one_round(call, iters):
    call()                                                   # warm-up of this configuration in this round
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def alternate(calls, rounds, iters):
    """calls: {name: callable} -> {name: [ms per call, one per round]}, the names alternating inside every round."""
    ms = {k: [] for k in calls}
    for _ in range(rounds):
        for k, c in calls.items():
            ms[k].append(one_round(c, iters))
    return ms


def summary(v):
    return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3), "rounds": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--tiny", action="store_true")
    ap.add_argument("--ab-old", action="store_true")
    ap.add_argument("--grid", action="store_true", help="the crops x beams grid (the default when nothing else is asked for)")
    ap.add_argument("--trace-step", action="store_true")
    ap.add_argument("--process", type=int, default=None, help="tag of this run in the record's lines")
    a = ap.parse_args()
    global PROCESS
    PROCESS = a.process
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    if a.tiny:
        from dataclasses import replace
        arch = replace(Blip2Arch.tiny(), t_hidden=256, t_heads=4, t_ffn=512)          # OPT widths the int8 weight stream takes
    else:
        arch = Blip2Arch()
    t0 = time.perf_counter()
    sd = procedural_blip2_state_dict(arch, 0, eos_boost=0.0)
    print(f"weights drawn in {time.perf_counter() - t0:.0f}s", flush=True)
    n, geom = arch.max_new_tokens, "tiny" if a.tiny else "OPT-2.7b geometry, full depth"
    px = synthetic_pixels(8, arch.image_size, seed=0).cuda()

    if a.trace_step:
        eng = engine(arch, sd, True, 1, 5)
        for _ in range(4):
            eng.generate(px[:1], num_beams=5, max_length=n)
        torch.cuda.synchronize()
        return
    if a.ab_old:
        if not os.path.exists(OLD):
            sys.exit(f"{OLD} is missing: bash tools/build_old_lib.sh <parent revision>")
        for first in ("this", "parent"):        # which handle is created (and measured) first: its arena lies elsewhere in memory
            if first == "this":
                new = engine(arch, sd, True, 1, 1)
                old = engine(arch, sd, True, 1, 1, OLD)
            else:
                old = engine(arch, sd, True, 1, 1, OLD)
                new = engine(arch, sd, True, 1, 1)
            ids = [e.generate(px[:1], max_length=n)["sequences"].cpu() for e in (new, old)]
            calls = {"parent": lambda: old.generate(px[:1], max_length=n), "this": lambda: new.generate(px[:1], max_length=n)}
            if first == "this":
                calls = dict(reversed(list(calls.items())))
            ms = alternate(calls, a.rounds, a.iters)
            p, t = summary(ms["parent"]), summary(ms["this"])
            emit({"what": "greedy must not pay: one crop, num_beams 1, load_in_8bit, this build against the parent's library in one process",
                  "geometry": geom, "new_tokens": n, "created_and_timed_first": first, "same_tokens": bool(torch.equal(ids[0], ids[1])),
                  "parent": p, "this": t, "difference_ms": round(t["median_ms"] - p["median_ms"], 3),
                  "parent_spread_ms": round(p["max_ms"] - p["min_ms"], 3),
                  "within_parent_spread": abs(t["median_ms"] - p["median_ms"]) <= p["max_ms"] - p["min_ms"]})
            new.close()
            old.close()
        # what handles of ONE build differ by (their arenas lie at different addresses): the floor under the differences above
        same = [engine(arch, sd, True, 1, 1) for _ in range(4)]
        ms = alternate({f"handle {i}": (lambda e=e: e.generate(px[:1], max_length=n)) for i, e in enumerate(same)}, a.rounds, a.iters)
        hs = {k: summary(v) for k, v in ms.items()}
        med = [h["median_ms"] for h in hs.values()]
        emit({"what": "four handles of this build, same call, same process: the handle-to-handle difference", "geometry": geom,
              "new_tokens": n, "handles": hs, "largest_difference_of_medians_ms": round(max(med) - min(med), 3)})
        for e in same:
            e.close()
        if not a.grid:
            return
    for int8 in (False, True):
        eng = engine(arch, sd, int8, 8, 5)
        calls = {f"{B} crops x {K} beams": (lambda B=B, K=K: eng.generate(px[:B], num_beams=K, max_length=n))
                 for B in (1, 8) for K in (1, 3, 5)}
        ms = alternate(calls, a.rounds, a.iters)
        emit({"what": "ms per generate call by crops per call and beams (handle: max_batch 8, max_beams 5)", "geometry": geom,
              "new_tokens": n, "mode": "load_in_8bit" if int8 else "bf16", "device_GiB": round(eng.device_bytes / 2 ** 30, 2),
              "calls": {k: summary(v) for k, v in ms.items()}})
        eng.close()


if __name__ == "__main__":
    main()
