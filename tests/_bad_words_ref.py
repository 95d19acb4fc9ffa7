"""Restatements of HF's `bad_words_ids` semantics (transformers 5.x, generation/logits_process.py, NoBadWordsLogitsProcessor /
SequenceBiasLogitsProcessor with -inf biases), written from the rules, for the bad-words tests:

* a sequence of one token is banned at every step; `[eos]` alone is dropped;
* a sequence of n > 1 tokens bans its last token for a row exactly when the row's last n - 1 context tokens are its first n - 1; a
  sequence longer than the context (n > its length) never matches - HF skips it before it compares anything;
* banned = -inf added to the score;
* greedy: the ban goes on the logits row, then arg-max (first maximal index; an all -inf row gives 0, as torch.argmax);
* beam search: log-softmax of the RAW row, then the ban on the log-probs, then + the running score.
"""
import numpy as np


def banned_mask(context, V, seqs, eos=None):
    """bool [V]: the tokens banned for a row whose context (every token HF's processor sees for it, oldest first) is `context`."""
    ctx = [int(t) for t in context]
    m = np.zeros(V, dtype=bool)
    for s in seqs:
        s = [int(t) for t in s]
        if eos is not None and s == [int(eos)]:
            continue
        n = len(s)
        if n == 1:
            m[s[0]] = True
        elif n <= len(ctx) and ctx[len(ctx) - (n - 1):] == s[:-1]:
            m[s[-1]] = True
    return m


def greedy_choice(row, context, seqs, eos=None):
    """The greedy token of one fp32 logits row under the ban: arg-max of the row with banned entries at -inf."""
    x = np.asarray(row, dtype=np.float32).copy()
    x[banned_mask(context, x.size, seqs, eos)] = -np.inf
    if not (x > -np.inf).any():
        return 0
    return int(np.argmax(x))                      # numpy: the first maximal index; NaN never appears in these tests


def beam_log_probs(row, context, seqs, dtype=np.float64, eos=None):
    """log-softmax of the raw row in `dtype` (max-subtracted, as torch), banned entries -inf afterwards."""
    x = np.asarray(row).astype(dtype)
    z = x - x.max()
    lp = z - np.log(np.exp(z).sum(dtype=dtype))
    lp = lp.astype(dtype)
    lp[banned_mask(context, x.size, seqs, eos)] = -np.inf
    return lp


def bitmap_and_table(seqs, V, words, eos=None, rec=9):
    """What the kernels read (csrc/ops.h, BanSet): uint32 [words] static bitmap of the single tokens, int32 [n_multi, rec] records
    {n, tokens..., zeros} of the multi-token sequences."""
    bits = np.zeros(words, dtype=np.uint32)
    multi = []
    for s in seqs:
        s = [int(t) for t in s]
        if eos is not None and s == [int(eos)]:
            continue
        if len(s) == 1:
            assert 0 <= s[0] < V
            bits[s[0] >> 5] |= np.uint32(1 << (s[0] & 31))
        else:
            assert 2 <= len(s) <= rec - 1
            multi.append([len(s)] + s + [0] * (rec - 1 - len(s)))
    table = np.asarray(multi, dtype=np.int32).reshape(-1, rec)
    return bits, table
