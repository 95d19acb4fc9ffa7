#!/usr/bin/env python
"""Golden vectors for the sampling distribution from the REAL HF warpers (transformers 5.x, CPU fp32): `TemperatureLogitsWarper`,
`TopKLogitsWarper` and `TopPLogitsWarper` in HF's order on rows regenerated from recorded seeds.  Data only:

    python tools/make_goldens_sampling.py        # writes tests/golden/sampling_warpers.npz (under 100 KB)

Per case (vocabulary size, seed, temperature, top_k, top_p): the ids HF keeps (finite scores after the warpers) and their fp32
softmax probabilities.  The rows themselves are not stored: tests/_sampling_ref.py::golden_row(seed, V) regenerates them.

The library's rule differs from HF's in two places only, and the script asserts on every row that neither is in play: HF's top-k
removes `scores < k-th value` and so keeps ties, as the library does, but a tie at the boundary would make the kept COUNT depend on
it - no two equal values at the top-k boundary after the fp32 division; HF's top-p compares an fp32 cumulative sum with 1 - top_p,
the library an integer sum with floor((1 - top_p) W) - no cumulative probability within 1e-4 of 1 - top_p.  A third assertion
keeps HF's own fp32 softmax within the 1e-6 relative the test compares with: a kept score lies less than 16 below the maximum, so
the fp32 subtraction z - max rounds by at most half an ulp of [8, 16) = 4.8e-7 (the relative error of the probability), which with an
ulp of expf, the division and the sum's own rounding stays below 1e-6; from 16 on the subtraction alone may give 9.5e-7.  Seeds are
searched (base, base + 1, ...) for rows on which all three hold under every setting of their vocabulary."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from _sampling_ref import golden_row                                                                     # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "sampling_warpers.npz")
# vocabulary -> (rows, settings (temperature, top_k, top_p)); the full-vocabulary settings stay on the small vocabularies (file size)
PLAN = {
    64: (3, [(0.7, 0, 1.0), (1.0, 5, 1.0), (0.7, 12, 0.9), (1.3, 0, 0.8)]),
    509: (3, [(0.7, 0, 1.0), (1.0, 5, 1.0), (0.7, 50, 0.9), (1.3, 0, 0.8)]),
    30524: (2, [(1.0, 5, 1.0), (0.7, 50, 0.9), (0.5, 0, 0.6)]),
}
MARGIN = 1e-4


def hf_warp(row, T, k, p):
    """HF's warpers in `generate`'s order -> (kept ids, fp32 probabilities of the kept ids, preconditions hold)."""
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    scores = torch.from_numpy(np.array(row))[None].clone()
    scores = TemperatureLogitsWarper(float(T))(None, scores)
    ok = True
    if k > 0:
        srt = torch.sort(scores[0], descending=True).values
        ok = ok and bool(srt[k - 1] != srt[k])
        scores = TopKLogitsWarper(int(k))(None, scores)
    if p < 1.0:
        asc = torch.sort(scores[0], descending=False).values
        cum = torch.softmax(asc, dim=-1).cumsum(dim=-1)
        ok = ok and bool(((cum - (1.0 - p)).abs() > MARGIN).all())
        scores = TopPLogitsWarper(float(p))(None, scores)
    probs = torch.softmax(scores, dim=-1)[0]
    kept = torch.isfinite(scores[0]).nonzero()[:, 0]
    ok = ok and float(scores[0][kept].max() - scores[0][kept].min()) < 16.0
    return kept.numpy().astype(np.int32), probs[kept].numpy().astype(np.float32), ok


def main():
    Vs, seeds, Ts, ks, ps, offs, ids, probs = [], [], [], [], [], [0], [], []
    for V, (n_rows, settings) in PLAN.items():
        seed, found = 7000 + V, 0
        while found < n_rows:
            seed += 1
            assert seed < 7200 + V, f"no seed found for V = {V}"
            row = golden_row(seed, V)
            res = [hf_warp(row, *s) for s in settings]
            if not all(r[2] for r in res):
                continue
            found += 1
            for (T, k, p), (kept, pr, ok) in zip(settings, res):
                assert ok and len(kept) >= 1 and abs(float(pr.sum()) - 1.0) < 1e-5
                Vs.append(V); seeds.append(seed); Ts.append(T); ks.append(k); ps.append(p)
                ids.append(kept); probs.append(pr); offs.append(offs[-1] + len(kept))
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, V=np.array(Vs, np.int32), seed=np.array(seeds, np.int64), temperature=np.array(Ts, np.float64),
                        top_k=np.array(ks, np.int32), top_p=np.array(ps, np.float64), offsets=np.array(offs, np.int64),
                        ids=np.concatenate(ids), probs=np.concatenate(probs))
    size = os.path.getsize(OUT)
    assert size < 100 * 1024, size
    print(f"wrote {OUT}: {len(Vs)} cases, {offs[-1]} kept ids, {size} bytes")


if __name__ == "__main__":
    main()
