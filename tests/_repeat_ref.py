"""Restatements of HF's `repetition_penalty` / `no_repeat_ngram_size` semantics (transformers 5.x, generation/logits_process.py,
RepetitionPenaltyLogitsProcessor / NoRepeatNGramLogitsProcessor), written from the rules, for the repetition-control tests:

* penalty p (finite, > 0): every DISTINCT token id of the row's context that lies in [0, V) has its score x replaced by x * p if x < 0,
  else x / p - once, however often the token occurs; fp32 arithmetic, a true division (-inf stays -inf, 0 stays 0);
* n-gram size n (>= 1; 0 = off): with a context of c tokens nothing is banned when c + 1 < n; otherwise every token that followed an
  earlier occurrence of the context's last n - 1 tokens is banned (-inf); n = 1 bans every context token;
* order: penalty, n-grams, bad words (tests/_bad_words_ref.py);
* greedy: the processors act on the raw fp32 row, then arg-max (first maximal index; a row with nothing left gives 0);
* beam search: log-softmax of the RAW row, the penalty on the log-probs (all <= 0: lp * p), the bans, then + the running score;
* the context is what HF's processor sees: BLIP: BOS, prompt, generated tokens; BLIP-2: num_query_tokens image placeholders, BOS,
  generated tokens (`blip2_context`).
"""
import numpy as np

from _bad_words_ref import banned_mask


def penalise(row, context, p):
    """The row (any float dtype; fp32 in the greedy loop) after the penalty, as a new array of the same dtype."""
    x = np.array(row, copy=True)
    V = x.size
    ids = sorted({int(t) for t in context if 0 <= int(t) < V})
    if ids and p != 1.0:
        ids = np.asarray(ids, dtype=np.int64)
        v = x[ids]
        pp = x.dtype.type(p)
        with np.errstate(invalid="ignore"):
            x[ids] = np.where(v < 0, v * pp, v / pp)
    return x


def ngram_banned_mask(context, V, n):
    """bool [V]: the tokens the n-gram rule bans for a row with this context (oldest first)."""
    ctx = [int(t) for t in context]
    m = np.zeros(V, dtype=bool)
    c = len(ctx)
    if n <= 0 or c + 1 < n:
        return m
    tail = ctx[c - (n - 1):] if n > 1 else []
    for i in range(0, c - n + 1):
        if ctx[i:i + n - 1] == tail:
            t = ctx[i + n - 1]
            if 0 <= t < V:
                m[t] = True
    return m


def processed_row(row, context, p=1.0, n=0, seqs=(), eos=None, ban_context=None):
    """One fp32 logits row after the three processors in HF's order.  ban_context: the context of the bad-words processor where it
    differs (the library's BLIP-2 ban sees BOS and the generated tokens only); default = `context`."""
    x = penalise(np.asarray(row, dtype=np.float32), context, p)
    x[ngram_banned_mask(context, x.size, n)] = -np.inf
    if len(seqs):
        x[banned_mask(context if ban_context is None else ban_context, x.size, seqs, eos)] = -np.inf
    return x


def greedy_choice(row, context, p=1.0, n=0, seqs=(), eos=None, ban_context=None):
    x = processed_row(row, context, p, n, seqs, eos, ban_context)
    if not (x > -np.inf).any():
        return 0
    return int(np.argmax(x))                      # numpy: the first maximal index; NaN never appears in these tests


def beam_log_probs(row, context, p=1.0, n=0, seqs=(), dtype=np.float64, eos=None, ban_context=None):
    """log-softmax of the raw row in `dtype` (max-subtracted, as torch), then the penalty (lp * p on context tokens), then the bans."""
    x = np.asarray(row).astype(dtype)
    z = x - x.max()
    lp = (z - np.log(np.exp(z).sum(dtype=dtype))).astype(dtype)
    lp = penalise(lp, context, p)
    lp[ngram_banned_mask(context, x.size, n)] = -np.inf
    if len(seqs):
        lp[banned_mask(context if ban_context is None else ban_context, x.size, seqs, eos)] = -np.inf
    return lp


def blip2_context(generated, num_query_tokens, image_token, bos):
    """HF's BLIP-2 context: the image placeholders, BOS, the generated tokens."""
    return [int(image_token)] * int(num_query_tokens) + [int(bos)] + [int(t) for t in generated]


def has_repeated_ngram(tokens, n):
    """True when some n-gram occurs twice in the token list."""
    seen = set()
    for i in range(len(tokens) - n + 1):
        g = tuple(int(t) for t in tokens[i:i + n])
        if g in seen:
            return True
        seen.add(g)
    return False
