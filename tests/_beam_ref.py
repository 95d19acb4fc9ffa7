"""A plain serial beam search on the host, written from HF v5 `GenerationMixin._beam_search` (steps b - g of its loop), one item
and one selection at a time, every selection a repeated arg-max (numpy's argmax returns the FIRST maximal element: the flat-index
order on ties).  One implementation for two number formats: dtype = float32 mirrors torch's arithmetic operation by operation
(log-softmax as (x - max) - log(sum(exp(x - max))), the -1e9 masks added in fp32, the length-penalty denominator computed in
double and rounded to fp32 before the division), dtype = float64 is the truth.

mode LEGACY is the CoCa loop's pre-5.x scorer, as three differences from the above:
  1. a candidate's score is the RAW logit plus the running score (no log-softmax); MinLength puts -inf on EOS while cur_len < min_len;
  2. the start token counts in every length denominator: (cur_len + 1) ** lp where v5 has (cur_len + 1 - 1) ** lp;
  3. the early-stop test compares the pool's worst score with the step's best CANDIDATE (EOS ones included), not with the best
     running beam.

cur_len is HF's: the number of tokens a running beam holds, BOS included = the position the step writes; steps run for
cur_len = 1 .. max_len - 1.

Returned per step: the running beams and, for the margins of tests/test_beam_ref_cpu.py, the smallest gap of every deciding
comparison - "cut" (the order of the 2K best continuations and the first one left out), "run" (the K running beams and the first
left out), "pool" (the K pool entries and the first left out), "stop" (best running score against the pool's worst), each a list of differences.  A comparison
between two values that both carry a -1e9 mask decides nothing that is ever read again (empty pool slots; the running beams of the
max_len step, after which the loop ends), and is left out of the gaps."""
from __future__ import annotations

import numpy as np

from _beam_script import LEGACY, logits_row

MASKED = -1.0e8          # anything below carries at least one -1e9 mask
MARGIN = 8.0             # score bar: MARGIN x the fp32 reference's own error against fp64, plus one fp32 spacing of the score
_REFS = {}


def _pick(values, n):
    """n rounds of arg-max -> (indices, the sorted values of n + 1 rounds where that many exist)."""
    v = values.copy()
    idx, vals = [], []
    for r in range(min(n + 1, v.size)):
        i = int(np.argmax(v))
        if r < n:
            idx.append(i)
        vals.append(values[i])
        v[i] = -np.inf
    return idx, vals


def _gaps(sorted_vals):
    out = []
    for a, b in zip(sorted_vals[:-1], sorted_vals[1:]):
        if (a < MASKED and b < MASKED) or (np.isinf(a) and np.isinf(b)):
            continue
        out.append(float(a) - float(b))
    return out


def beam_search(case, dtype, items=None):
    """-> dict: ids [n, L] int32, lens [n], scores [n] (dtype), steps: list (one per step run) of dicts with cur_len, run_tokens
    [n, K, L], run_scores [n, K], run_src [n, K] (the beam each new running beam continues), active, open [n], gaps {cut, run,
    pool, stop}, displaced [n] (a finished best hypothesis lost its place); stop_cur_len."""
    dt = np.dtype(dtype).type
    items = list(range(case.B)) if items is None else list(items)
    n, K, V, L, C = len(items), case.K, case.V, case.max_len, 2 * case.K
    legacy = case.mode == LEGACY
    neg = dt(-1.0e9)
    run_seq = np.full((n, K, L), case.fill, dtype=np.int32)
    run_seq[:, :, 0] = case.bos
    pool_seq = run_seq.copy()
    run_sc = np.full((n, K), neg, dtype=dt)
    run_sc[:, 0] = 0
    pool_sc = np.full((n, K), neg, dtype=dt)
    pool_fin = np.zeros((n, K), dtype=bool)
    pool_len = np.zeros((n, K), dtype=np.int32)
    is_open = np.ones(n, dtype=bool)
    steps = []
    stop_cur_len = None
    for cur_len in range(1, L):
        gaps = {"cut": [], "run": [], "pool": [], "stop": []}
        all_hit = True
        displaced = np.zeros(n, dtype=bool)
        run_src = np.zeros((n, K), dtype=np.int32)
        glen = cur_len + 1 if legacy else cur_len + 1 - 1
        denom = dt(float(glen) ** float(case.lp))            # the power in double, then the format's rounding
        for a, item in enumerate(items):
            # b. accumulated scores of the K * V continuations
            acc = np.empty((K, V), dtype=dt)
            for k in range(K):
                x = logits_row(case, item, run_seq[a, k, :cur_len]).astype(dt)
                if legacy:
                    s = x + run_sc[a, k]
                    if cur_len < case.min_len:
                        s[case.eos] = -np.inf
                else:
                    z = x - x.max()
                    s = (z - np.log(np.sum(np.exp(z), dtype=dt))) + run_sc[a, k]
                acc[k] = s
            # c. the 2K best, best first
            flat_idx, vals = _pick(acc.reshape(-1), C)
            gaps["cut"] += _gaps(vals)
            val = np.array(vals[:C], dtype=dt)
            src = [f // V for f in flat_idx]
            tok = [f % V for f in flat_idx]
            # d. which of them stop
            hit = np.array([t == case.eos or cur_len + 1 >= L for t in tok])
            all_hit = all_hit and bool(hit.all())
            # e. the K best that go on
            run_lp = val + hit.astype(dt) * neg
            run_pick, rvals = _pick(run_lp, K)
            gaps["run"] += _gaps(rvals)
            # f. the pool: its K entries and the candidates among the first K that stopped
            just = hit & (np.arange(C) < K)
            f = val / denom
            f = f + dt(0.0 if is_open[a] else 1.0) * neg
            f = f + (~just).astype(dt) * neg
            msc = np.concatenate([pool_sc[a], f])
            pool_pick, pvals = _pick(msc, K)
            gaps["pool"] += _gaps(pvals)
            new_pool_seq = np.empty((K, L), dtype=np.int32)
            new_fin = np.zeros(K, dtype=bool)
            new_len = np.zeros(K, dtype=np.int32)
            for k, p in enumerate(pool_pick):
                if p < K:
                    new_pool_seq[k], new_fin[k], new_len[k] = pool_seq[a, p], pool_fin[a, p], pool_len[a, p]
                else:
                    c = p - K
                    new_pool_seq[k] = run_seq[a, src[c]]
                    new_pool_seq[k, cur_len] = tok[c]
                    new_fin[k], new_len[k] = just[c], cur_len + 1
            displaced[a] = bool(pool_fin[a, 0] and pool_pick[0] >= K)
            new_pool_sc = msc[pool_pick]
            new_run_seq = np.empty((K, L), dtype=np.int32)
            for k, c in enumerate(run_pick):
                new_run_seq[k] = run_seq[a, src[c]]
                new_run_seq[k, cur_len] = tok[c]
            best = (val[0] if legacy else run_lp[run_pick[0]]) / denom
            run_src[a] = [src[c] for c in run_pick]
            run_seq[a], run_sc[a] = new_run_seq, run_lp[run_pick]
            pool_seq[a], pool_sc[a], pool_fin[a], pool_len[a] = new_pool_seq, new_pool_sc, new_fin, new_len
            # g. can a running beam still beat the pool's worst entry?
            mn = new_pool_sc.min()
            worst = np.where(new_fin, mn, neg)
            # legacy, the best candidate stopped and is itself the pool's worst entry: both sides are the one expression
            # val[0] / denom, equal in every number format - nothing to decide
            same_expr = legacy and just[0] and pool_pick[int(np.argmin(new_pool_sc))] == K
            if is_open[a] and new_fin.all() and best > MASKED and not same_expr:
                gaps["stop"].append(abs(float(best) - float(mn)))
            is_open[a] = bool(is_open[a] and (best > worst).any())
        active = bool(is_open.any() and not all_hit)
        steps.append({"cur_len": cur_len, "run_tokens": run_seq.copy(), "run_scores": run_sc.copy(), "active": active,
                      "gaps": gaps, "displaced": displaced, "open": is_open.copy(), "run_src": run_src})
        if not active:
            stop_cur_len = cur_len
            break
    return {"ids": pool_seq[:, 0].copy(), "lens": pool_len[:, 0].copy(), "scores": pool_sc[:, 0].copy(), "steps": steps,
            "stop_cur_len": stop_cur_len}


def live(x):
    """Mask of the scores that carry no -1e9 mask (those have fp32 spacing 64: their rounding says nothing about the arithmetic)."""
    return np.asarray(x, dtype=np.float64) > MASKED


def score_error(r32, r64):
    """max |fp32 host reference - fp64 host reference| over a case's unmasked final and running scores (same decisions assumed)."""
    err = 0.0
    pairs = [(r32["scores"], r64["scores"])] + [(a["run_scores"], b["run_scores"]) for a, b in zip(r32["steps"], r64["steps"])]
    for a, b in pairs:
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        m = live(b)
        if m.any():
            err = max(err, float(np.abs(a[m] - b[m]).max()))
    return err


def same_decisions(r32, r64):
    if len(r32["steps"]) != len(r64["steps"]) or r32["stop_cur_len"] != r64["stop_cur_len"]:
        return False
    if not (np.array_equal(r32["ids"], r64["ids"]) and np.array_equal(r32["lens"], r64["lens"])):
        return False
    for a, b in zip(r32["steps"], r64["steps"]):
        last = a["cur_len"] + 1 >= r32["ids"].shape[1]           # the max_len step's running beams are all masked: see the header
        if a["active"] != b["active"] or not np.array_equal(a["open"], b["open"]):
            return False
        if not last and not np.array_equal(a["run_tokens"], b["run_tokens"]):
            return False
    return True


def min_gaps(r, positive_only=False):
    """Smallest gap per kind of comparison over the whole search (positive_only: exact ties left out)."""
    out = {"cut": np.inf, "run": np.inf, "pool": np.inf, "stop": np.inf}
    for s in r["steps"]:
        for k, v in s["gaps"].items():
            v = [g for g in v if g > 0.0 or not positive_only]
            out[k] = min([out[k]] + v)
    return out


def refs(case):
    """(fp32 reference, fp64 reference, score error) of a case: computed once per process, shared, never modified."""
    if case.name not in _REFS:
        r32, r64 = beam_search(case, np.float32), beam_search(case, np.float64)
        _REFS[case.name] = (r32, r64, score_error(r32, r64))
    return _REFS[case.name]


def bar(err, score):
    """The score bar: MARGIN x the case's fp32-vs-fp64 reference error + one fp32 spacing at the score's magnitude."""
    return MARGIN * err + float(np.spacing(np.float32(abs(score))))
