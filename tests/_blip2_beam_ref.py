"""Beam search over the CPU restatement of BLIP-2 (oracle/blip2_ref.py), for HF `Blip2ForConditionalGeneration.generate(num_beams=K)`.

The model: `language_inputs` and the prompt pass run once per image; the decoder state (`OptState`) is then expanded to K rows per
image and re-ordered by every step's choice of running beams, as HF does with its cache.  The bookkeeping is HF v5
`GenerationMixin._beam_search` restated as tests/_beam_ref.py states it (2K candidates by repeated arg-max, the -1e9 masks added in
the number format, the length-penalty denominator computed in double and rounded to the format), in HF's numbering with the prompt
taken off: a beam's token columns are [BOS, new tokens ...], `cur_len` = the column a step writes = the number of new tokens after
it, so `cur_len + 1 - prompt_len` of HF is `cur_len` here and its `max_length - prompt_len` is max_new.

Two number formats: float32 follows torch's arithmetic, float64 is the truth - the restatement's `.float()` casts are kept from
rounding by a Tensor subclass whose `.float()` is the identity.

The DECISION GAP of an image is the smallest difference, at any step while the image is open, between the last kept and the best
dropped entry of each of the step's three selections (the 2K candidates, the K running beams, the K pool entries), together with
the three other comparisons that change what is returned: candidates K - 1 and K where one of them ends a hypothesis (only the
first K may enter the pool), the early-stop comparison (best running beam against the pool's worst entry), and the pool's best
against its second entry when the search ends.  The order among kept entries otherwise only moves rows.  Two entries that both
carry a -1e9 mask decide nothing.  An arithmetic whose scores are within half that gap of the truth takes the same decisions."""
from __future__ import annotations

import numpy as np
import torch

from _beam_ref import MASKED, _gaps, _pick


def _cut(sorted_vals, n):
    """The gap between entry n - 1 (the last kept) and entry n (the best dropped), as a list; empty where nothing is decided."""
    return _gaps(sorted_vals[n - 1:n + 1])

LM = "language_model.model.decoder."


class _Keep(torch.Tensor):
    """A float64 tensor that stays float64 through the restatement's `.float()`."""

    def float(self):
        return self


def in_format(sd, dtype):
    if np.dtype(dtype) == np.float32:
        return sd
    return {k: v.double().as_subclass(_Keep) if v.is_floating_point() else v for k, v in sd.items()}


@torch.no_grad()
def beam_search(sd, a, pixels, K, lp=1.0, max_new=None, dtype=np.float32):
    """-> dict: ids int32 [B, max_new] (the new tokens, fill value behind the end), lens [B], scores [B] (dtype), gap [B] (the decision
    gap), top2 [B] (best minus second-best returned hypothesis), steps (model steps after the prompt pass), reorders (how many of them
    ran on rows that were not their own continuation: the steps at which a cache is read through another row's history)."""
    from oracle import blip2_ref as R
    dt = np.dtype(dtype).type
    tdt = torch.float32 if dt is np.float32 else torch.float64
    sdd = in_format(sd, dtype)
    n = max_new or a.max_new_tokens
    B, V, L, C = int(pixels.shape[0]), a.vocab, n + 1, 2 * K
    fill = a.pad if a.pad else a.eos
    neg = dt(-1.0e9)
    _, _, proj = R.language_inputs(sdd, a, pixels.to(tdt))
    tok = sdd[LM + "embed_tokens.weight"].float()
    st = R.OptState(a.t_layers)
    logits = R.opt_forward(sdd, a, torch.cat([proj, tok[torch.full((B, 1), a.bos)]], 1), st)
    st.k = [k.repeat_interleave(K, 0) for k in st.k]
    st.v = [v.repeat_interleave(K, 0) for v in st.v]
    logits = logits.repeat_interleave(K, 0)

    run_seq = np.full((B, K, L), fill, dtype=np.int32)
    run_seq[:, :, 0] = a.bos
    pool_seq = run_seq.copy()
    run_sc = np.full((B, K), neg, dtype=dt)
    run_sc[:, 0] = 0
    pool_sc = np.full((B, K), neg, dtype=dt)
    pool_fin = np.zeros((B, K), dtype=bool)
    pool_len = np.zeros((B, K), dtype=np.int32)
    is_open = np.ones(B, dtype=bool)
    gap = np.full(B, np.inf)
    steps = reorders = 0
    for cur_len in range(1, L):
        x_all = logits.as_subclass(torch.Tensor).numpy().astype(dt).reshape(B, K, V)
        denom = dt(float(cur_len) ** float(lp))
        all_hit = True
        run_src = np.zeros((B, K), dtype=np.int64)
        for b in range(B):
            z = x_all[b] - x_all[b].max(-1, keepdims=True)
            acc = (z - np.log(np.sum(np.exp(z), -1, dtype=dt, keepdims=True))) + run_sc[b][:, None]
            flat_idx, vals = _pick(acc.reshape(-1), C)
            g = _cut(vals, C)
            val = np.array(vals[:C], dtype=dt)
            src = [f // V for f in flat_idx]
            tk = [f % V for f in flat_idx]
            hit = np.array([t == a.eos or cur_len + 1 >= L for t in tk])
            all_hit = all_hit and bool(hit.all())
            if hit[K - 1] or hit[K]:
                g += _cut(vals, K)
            run_lp = val + hit.astype(dt) * neg
            run_pick, rvals = _pick(run_lp, K)
            g += _cut(rvals, K)
            just = hit & (np.arange(C) < K)
            f = val / denom
            f = f + dt(0.0 if is_open[b] else 1.0) * neg
            f = f + (~just).astype(dt) * neg
            msc = np.concatenate([pool_sc[b], f])
            pool_pick, pvals = _pick(msc, K)
            g += _cut(pvals, K)
            new_pool_seq = np.empty((K, L), dtype=np.int32)
            new_fin = np.zeros(K, dtype=bool)
            new_len = np.zeros(K, dtype=np.int32)
            for k, p in enumerate(pool_pick):
                if p < K:
                    new_pool_seq[k], new_fin[k], new_len[k] = pool_seq[b, p], pool_fin[b, p], pool_len[b, p]
                else:
                    c = p - K
                    new_pool_seq[k] = run_seq[b, src[c]]
                    new_pool_seq[k, cur_len] = tk[c]
                    new_fin[k], new_len[k] = just[c], cur_len + 1
            new_run_seq = np.empty((K, L), dtype=np.int32)
            for k, c in enumerate(run_pick):
                new_run_seq[k] = run_seq[b, src[c]]
                new_run_seq[k, cur_len] = tk[c]
            best = run_lp[run_pick[0]] / denom
            run_src[b] = [src[c] for c in run_pick]
            run_seq[b], run_sc[b] = new_run_seq, run_lp[run_pick]
            pool_seq[b], pool_sc[b], pool_fin[b], pool_len[b] = new_pool_seq, msc[pool_pick], new_fin, new_len
            mn = pool_sc[b].min()
            worst = np.where(new_fin, mn, neg)
            if is_open[b] and new_fin.all() and best > MASKED:
                g.append(abs(float(best) - float(mn)))
            if is_open[b]:                    # a closed image takes nothing into its pool any more: its later steps decide nothing
                gap[b] = min([gap[b]] + g)
            is_open[b] = bool(is_open[b] and (best > worst).any())
        if not (is_open.any() and not all_hit) or cur_len + 1 == L:
            break
        rows = torch.from_numpy((np.arange(B)[:, None] * K + run_src).reshape(-1))
        st.k = [k[rows] for k in st.k]
        st.v = [v[rows] for v in st.v]
        nxt = torch.from_numpy(run_seq[:, :, cur_len].reshape(-1).astype(np.int64))
        logits = R.opt_forward(sdd, a, tok[nxt][:, None], st)
        steps += 1
        reorders += int((run_src != np.arange(K)[None, :]).any())
    top2 = np.array([float(pool_sc[b, 0]) - float(pool_sc[b, 1]) for b in range(B)])
    gap = np.minimum(gap, np.where(pool_sc[:, 1] > MASKED, top2, np.inf))
    return {"ids": pool_seq[:, 0, 1:].copy(), "lens": pool_len[:, 0] - 1, "scores": pool_sc[:, 0].copy(), "gap": gap, "top2": top2,
            "steps": steps, "reorders": reorders}
