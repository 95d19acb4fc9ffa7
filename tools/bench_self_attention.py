#!/usr/bin/env python
"""The decoder's fused self-attention step (q|k|v partial sums in, k / v appended, up to 32 positions): the form in which every
key sub-lane finishes its own partial sums (1) against the one that finishes each column once per unit (2), by row count and
position, us per launch.  Launches replayed from a captured graph over rotating caches (a pass walks 12 layers' caches: they come
from HBM), HIP events.  --live F: the compacted loop's launch with a fraction F of the rows open.
    python tools/bench_self_attention.py [--rows 256,512,768,1024] [--keys 4,10,20] [--live 0.6]"""
import argparse
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from embodied_captioning_amd import _native as N  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", default="256,512,768,1024")
ap.add_argument("--keys", default="4,10,20")
ap.add_argument("--live", type=float, default=1.0)
args = ap.parse_args()

lib = N.load_library()
p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
H, S, LM, NB = 12, 4, 20, 4
W = H * 64
print(f"live fraction {args.live}")
print(" rows keys dtype  form1  form2  (us per launch)")
for R in (int(x) for x in args.rows.split(",")):
    n_live = torch.tensor([int(round(R * args.live))], dtype=torch.int32, device="cuda") if args.live < 1.0 else None
    live = torch.arange(R, dtype=torch.int32, device="cuda") if n_live is not None else None
    for tag, tdt, name in ((2, torch.float32, "f32s"), (1, torch.bfloat16, "bf16")):
        parts = [torch.randn(S, R, 3 * W, device="cuda") for _ in range(NB)]
        kcs = [torch.randn(R, H, LM, 64, device="cuda").to(tdt) for _ in range(NB)]
        vcs = [torch.randn(R, H, LM, 64, device="cuda").to(tdt) for _ in range(NB)]
        ctx = [torch.empty(R, W, dtype=tdt, device="cuda") for _ in range(NB)]
        bias = torch.randn(3 * W, device="cuda")
        for nk in (int(x) for x in args.keys.split(",")):
            def run(form, i):
                rc = lib.cap_op_decode_attention_live(tag, p(parts[i]), S, p(bias), 3 * W, 0, 1, p(kcs[i]), p(vcs[i]), LM, nk, p(ctx[i]), R, H,
                                                      p(live), p(n_live), form, st())
                assert rc == 0, lib.cap_last_error().decode()
            res = {}
            for form in (1, 2):
                for i in range(NB):
                    run(form, i)
                torch.cuda.synchronize()
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr):
                    for j in range(60):
                        run(form, j % NB)
                gr.replay()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(5):
                    gr.replay()
                e1.record()
                torch.cuda.synchronize()
                res[form] = e0.elapsed_time(e1) / 300 * 1e3
            print(f"{R:5d} {nk:4d} {name:5s} {res[1]:6.2f} {res[2]:6.2f}", flush=True)
