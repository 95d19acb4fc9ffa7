#!/usr/bin/env python
"""What the per-object caption statistics cost on the device (GPU box only): `similarity.group_similarity` (one call: disagreement,
pair mean / variance, row means and medoid of every group) against torch on the same device computing the same definitions
 - one group at a time, as the reference's loop does (`_cosine_distance` per object, scripts/compute_cosine_sim.py per group), and
 - as one batched `bmm` over the groups (equal sizes here, so the batch needs no padding: the best case for torch).

    python tools/bench_caption_disagreement.py            5 000 groups of 10, 100 groups of 500, one group of 4 096; D = 384
    python tools/bench_caption_disagreement.py --tiny     small shapes, to rehearse the tool

One process; the three forms alternate inside each of --rounds rounds (drift of the box hits all alike), a round times --iters calls
between two device events after a warm-up call, and a record holds the median over the rounds with the smallest and largest round.
Lines are appended to profiles/caption_disagreement_bench.jsonl.  The comparison is reported, not gated; `agree` says that the three
forms gave the same numbers (to 1e-4) on the shape that was timed."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from embodied_captioning_amd.similarity import group_similarity  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "caption_disagreement_bench.jsonl")


def emit(rec):
    rec["tool"] = "tools/bench_caption_disagreement.py"
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


def torch_one_group(e):
    n = e.shape[0]
    eh = F.normalize(e, dim=1, eps=1e-12)
    s = eh @ eh.T
    dis = (1.0 - s).mean()
    iu = torch.triu_indices(n, n, 1, device=e.device)
    v = s[iu[0], iu[1]]
    rm = (s.sum(1) - s.diagonal()) / (n - 1)
    return dis, v.mean(), v.var(unbiased=False), rm, rm.argmax()


def torch_loop(e, G, n):
    out = [torch_one_group(e[g * n:(g + 1) * n]) for g in range(G)]
    return (torch.stack([o[0] for o in out]), torch.stack([o[1] for o in out]), torch.stack([o[2] for o in out]),
            torch.cat([o[3] for o in out]), torch.stack([o[4] for o in out]))


def torch_batched(e, G, n):
    eh = F.normalize(e, dim=1, eps=1e-12).view(G, n, -1)
    s = torch.bmm(eh, eh.transpose(1, 2))
    dis = (1.0 - s).mean(dim=(1, 2))
    up = torch.triu(torch.ones(n, n, device=e.device, dtype=torch.bool), 1)
    v = s[:, up]
    rm = (s.sum(2) - s.diagonal(dim1=1, dim2=2)) / (n - 1)
    return dis, v.mean(1), v.var(1, unbiased=False), rm.reshape(-1), rm.argmax(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--tiny", action="store_true")
    a = ap.parse_args()
    shapes = [(50, 10), (4, 100), (1, 300)] if a.tiny else [(5000, 10), (100, 500), (1, 4096)]
    for G, n in shapes:
        g = torch.Generator(device="cpu").manual_seed(G)
        e = (torch.randn(G * n, a.dim, generator=g) + 0.5 * torch.randn(1, a.dim, generator=g)).cuda()
        offsets = np.arange(G + 1, dtype=np.int64) * n
        cfgs = {"group_similarity": lambda: group_similarity(e, offsets),
                "torch_per_group": lambda: torch_loop(e, G, n),
                "torch_batched_bmm": lambda: torch_batched(e, G, n)}
        iters = {k: 1 if k == "torch_per_group" and G > 100 else a.iters for k in cfgs}       # the long loop is timed one call a round
        ms = {k: [] for k in cfgs}
        for _ in range(a.rounds):
            for k, fn in cfgs.items():
                ms[k].append(timed(fn, iters[k]))
        st = group_similarity(e, offsets)
        ref = torch_batched(e, G, n)
        loop = torch_loop(e, G, n)
        agree = all(float((x.double() - y.double()).abs().max()) < 1e-4 and float((x.double() - z.double()).abs().max()) < 1e-4
                    for x, y, z in zip((st.disagreement, st.pair_mean, st.pair_var, st.row_mean), ref, loop))
        med = {k: statistics.median(v) for k, v in ms.items()}
        emit({"what": "caption disagreement", "groups": G, "group_size": n, "D": a.dim, "rounds": a.rounds, "iters": iters,
              "ms": {k: {"median": round(med[k], 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in ms.items()},
              "per_group_over_kernel": round(med["torch_per_group"] / med["group_similarity"], 2),
              "batched_over_kernel": round(med["torch_batched_bmm"] / med["group_similarity"], 2), "agree": bool(agree)})


if __name__ == "__main__":
    main()
