#!/usr/bin/env python
"""Cost of the repetition controls (`CaptionerEngine.set_repeat_controls`) on the decode loops.  Procedural weights with eos_boost 0
(every caption runs to its full length), early exit off, ONE process, legs alternating round by round after --warmup rounds, each
call timed with device events:

  configuration 1   BLIP-base, f32s, --rows rows, max_length 20, greedy: the handle with the controls off against the SAME handle with
                    --penalty and --ngram set
  configuration 2   BLIP-2 (--blip2 opt2.7b: OPT-2.7b geometry; tiny: the fixture), bf16, one crop: greedy and 5 beams, each with the
                    controls off and on

One JSON line: the median and every round of each leg, each controlled-minus-uncontrolled delta beside the uncontrolled leg's own
run-to-run spread (max - min over its rounds), and the `greedy_select` / `beam_step` profile tags of one extra call per leg (the
selection kernels' time).  A `rocprofv3 --kernel-trace --stats -- python tools/bench_repeat_controls.py --out "" --controls off` run of
its own names the kernels a handle launches with nothing set.

    python tools/bench_repeat_controls.py [--rows 256] [--rounds 7] [--blip2 opt2.7b] [--out profiles/repeat_controls_bench.jsonl]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--max-length", type=int, default=20)
    ap.add_argument("--arch", default="base", choices=["base", "tiny"])
    ap.add_argument("--blip2", default="opt2.7b", choices=["opt2.7b", "tiny", "none"])
    ap.add_argument("--penalty", type=float, default=1.3)
    ap.add_argument("--ngram", type=int, default=2)
    ap.add_argument("--controls", default="both", choices=["both", "off"], help="off: only the uncontrolled legs run (kernel-name traces)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "repeat_controls_bench.jsonl"))
    a = ap.parse_args(argv)
    import torch
    from embodied_captioning_amd.config import Blip2Arch, BlipArch
    from embodied_captioning_amd.engine import CaptionerEngine
    from embodied_captioning_amd.weights import procedural_blip2_state_dict, procedural_blip_state_dict, synthetic_pixels

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    legs = (("", (1.0, 0)), ("_controlled", (a.penalty, a.ngram))) if a.controls == "both" else (("", (1.0, 0)),)

    def run(eng, calls):
        """calls: name -> generate kwargs.  Legs `name` (controls off) and `name_controlled`, alternating; -> (ms, selection-kernel ms per leg)."""
        ms = {f"{k}{s}": [] for k in calls for s, _ in legs}
        sel = {}
        for r in range(a.warmup + a.rounds):
            for k, (px, kw) in calls.items():
                for s, q in legs:
                    eng.set_repeat_controls(*q)
                    t, _ = timed(lambda: eng.generate(px, **kw))
                    if r >= a.warmup:
                        ms[k + s].append(round(t, 3))
        for k, (px, kw) in calls.items():
            for s, q in legs:
                eng.set_repeat_controls(*q)
                eng.profile(True)
                eng.generate(px, **kw)
                rep = eng.profile_report()
                eng.profile(False)
                sel[k + s] = {t: {"launches": v["launches"], "ms": round(v["ms"], 4)} for t, v in rep.items() if t in ("greedy_select", "beam_step")}
        eng.set_repeat_controls()
        return ms, sel

    def summary(ms):
        out = {}
        for k in [k for k in ms if not k.endswith("_controlled")]:
            b, c = ms[k], ms.get(k + "_controlled")
            out[k] = {"uncontrolled_ms": round(statistics.median(b), 3), "uncontrolled_spread_ms": round(max(b) - min(b), 3)}
            if c:
                out[k].update(controlled_ms=round(statistics.median(c), 3), delta_ms=round(statistics.median(c) - statistics.median(b), 3))
        return out

    say = lambda m: print(f"[bench_repeat_controls] {m}", file=sys.stderr, flush=True)      # noqa: E731
    say("BLIP: weights")
    rec = {"bench": "repeat_controls", "penalty": a.penalty, "ngram": a.ngram, "rounds": a.rounds}
    arch = BlipArch() if a.arch == "base" else BlipArch.tiny()
    L = a.max_length
    eng = CaptionerEngine(arch, dtype="f32s", max_batch=a.rows, max_beams=1, max_len=L)
    eng.load_state_dict(procedural_blip_state_dict(arch, 0, eos_boost=0.0))
    eng.set_early_exit(0)
    px = synthetic_pixels(a.rows, arch.image_size, seed=0).cuda()
    say("BLIP: timing")
    ms, sel = run(eng, {"greedy": (px, {"max_length": L})})
    rec["blip"] = {"arch": a.arch, "dtype": "f32s", "rows": a.rows, "max_length": L, "vocab": arch.vocab, "summary": summary(ms), "ms": ms,
                   "selection_kernels": sel}
    eng.close()
    if a.blip2 != "none":
        a2 = Blip2Arch() if a.blip2 == "opt2.7b" else Blip2Arch.tiny()
        n = a2.max_new_tokens
        say("BLIP-2: weights")
        eng = CaptionerEngine(a2, dtype="bf16", max_batch=1, max_beams=5, max_len=n)
        eng.load_state_dict(procedural_blip2_state_dict(a2, 0, eos_boost=0.0))
        eng.set_early_exit(0)
        px = synthetic_pixels(1, a2.image_size, seed=0).cuda()
        say("BLIP-2: timing")
        ms, sel = run(eng, {"greedy": (px, {"max_length": n}), "beams5": (px, {"max_length": n, "num_beams": 5})})
        rec["blip2"] = {"arch": a.blip2, "dtype": "bf16", "rows": 1, "max_new_tokens": n, "vocab": a2.vocab, "summary": summary(ms), "ms": ms,
                        "selection_kernels": sel}
        eng.close()
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
