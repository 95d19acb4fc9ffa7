"""The sampled token selection restated for the sampling tests (include/captioner_hip.h, cap_set_sampling): a numpy Philox4x32-10,
steps 1-6 of the distribution with fp64 weights, and the interval rule a drawn token is checked with.

For an open caption at the step that produces its j-th generated token, on the raw fp32 row x:
  1. s = processors(x) (tests/_repeat_ref.py: penalty, n-grams, bad words; banned = -inf, a NaN stands as -inf)
  2. z = s / T in fp32 (numpy's fp32 division is correctly rounded, as the kernel's)
  3. top-k (0 or >= V: off): keep z_i >= the k-th largest value, ties included - exact on the fp32 values
  4. m = max kept z; w_i = floor(exp(z_i - m) * 2^40), here with fp64 exp
  5. top-p (1: off): W = sum w, R = min(floor((1 - top_p) * W), W - 1) in fp64 as the kernel computes it; a value v stays iff the weight of
     the kept entries with z <= v exceeds R
  6. U = Philox4x32-10(counter (j, 0, key_lo, key_hi), key (seed_lo, seed_hi)), (out0 << 32) | out1; r = (U * W') >> 64; the token is
     the smallest id whose inclusive prefix sum exceeds r.

The kernel's weights come from fp32 expf, so its integers differ from these by rounding.  A token it returns for the uniform U is
accepted iff (unit: the maximal weight = 1)
    cdf64[i - 1] - delta <= (U / 2^64) * total <= cdf64[i] + delta,
    delta = total * ((max|z| + 28) * 2^-24 + 2^-22) + V * 2^-40
- the rounding of the division and of the subtraction on exponents no further than 40 ln 2 < 28 from the maximum (relative error of
exp(d) = absolute error of d), two ulp of expf, and the truncation of every weight.  `reference` reports how far the top-p cut is from a
flip in the same unit, so that a test can require its fixture to be further than delta from one.
"""
import math

import numpy as np

from _repeat_ref import processed_row

M32 = np.uint64(0xFFFFFFFF)
TWO40 = float(2 ** 40)


def philox4x32_10(counter, key):
    """counter: 4 words, key: 2 words (ints or equally shaped integer arrays) -> 4 uint64 arrays holding the 32-bit outputs."""
    c = [np.asarray(x, dtype=np.uint64) & M32 for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0 = np.asarray(key[0], dtype=np.uint64) & M32
    k1 = np.asarray(key[1], dtype=np.uint64) & M32
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return c


def uniform64(seed, key, draw):
    """The 64-bit uniform(s) of (seed, key, draw): python ints for scalar arguments, else a uint64 array."""
    key = np.asarray(key, dtype=np.uint64)
    seed = int(seed)
    o = philox4x32_10((draw, 0, key & M32, key >> np.uint64(32)), (seed & 0xFFFFFFFF, seed >> 32))
    u = (o[0] << np.uint64(32)) | o[1]
    return int(u) if u.ndim == 0 else u


def delta(ref):
    """The interval rule's slack for a row's reference, unit: maximal weight = 1."""
    return ref["total"] * ((ref["max_abs_z"] + 28.0) * 2.0 ** -24 + 2.0 ** -22) + ref["V"] * 2.0 ** -40


def reference(row, temperature=1.0, top_k=0, top_p=1.0, context=(), penalty=1.0, ngram=0, seqs=(), eos=None, ban_context=None):
    """Steps 1-5 on one fp32 row -> dict: z (fp32), w (fp64 [V]: exp(z - m) of what is left, 0 elsewhere; maximal weight 1), wi (the
    integer weights as python-exact fp64), kept (entries with wi > 0), total, topk_tie (the k-th and (k + 1)-th largest values are
    equal), topp_margin (distance of the top-p decision from a flip, unit weights; inf when off), edge (an integer weight
    within 1e-5 relative of the 2^-40 truncation edge)."""
    s = processed_row(row, context, penalty, ngram, seqs, eos, ban_context)
    s[np.isnan(s)] = -np.inf
    with np.errstate(invalid="ignore"):
        z = (s / np.float32(temperature)).astype(np.float32)
    z[z == 0] = 0.0
    V = z.size
    keep = z > -np.inf
    topk_tie = False
    if 0 < top_k < V:
        srt = np.sort(z)
        kth = srt[V - top_k]
        topk_tie = bool(srt[V - top_k - 1] == kth)
        keep &= z >= kth
    out = {"z": z, "V": V, "topk_tie": topk_tie, "topp_margin": math.inf, "edge": False}
    if not keep.any():
        out.update(w=np.zeros(V), wi=np.zeros(V), kept=0, total=0.0, max_abs_z=0.0)
        return out
    m = np.float64(z[keep].max())
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.where(keep, np.exp(z.astype(np.float64) - m), 0.0)
    scaled = e * TWO40
    wi = np.floor(scaled)
    near = (scaled > 0.5) & (np.abs(scaled - 1.0) < 1e-5)
    out["edge"] = bool(near.any())
    if top_p < 1.0:
        W = int(wi.sum())
        R = int(math.floor((1.0 - float(np.float32(top_p))) * float(W)))
        R = min(R, W - 1)
        live = np.flatnonzero(wi > 0)
        order = live[np.argsort(z[live], kind="stable")]   # ascending values
        zs, cs = z[order], np.cumsum(wi[order].astype(np.int64))   # a row's weights sum to less than V * 2^40: int64 holds them
        last = np.flatnonzero(np.r_[zs[1:] != zs[:-1], True])      # the last entry of every distinct value
        vals, cum = zs[last], [int(c) for c in cs[last]]
        stay = np.array([c > R for c in cum])
        first = int(np.argmax(stay))                       # the maximal value always stays: W > R
        thr = vals[first]
        below = int(cum[first - 1]) if first > 0 else None
        margin = (int(cum[first]) - R) / TWO40
        if below is not None:
            margin = min(margin, (R - below) / TWO40)
        out["topp_margin"] = float(margin)
        wi = np.where(z >= thr, wi, 0.0)
    w = np.where(wi > 0, e, 0.0)
    live = wi > 0
    out.update(w=w, wi=wi, kept=int(live.sum()), total=float(w.sum()), max_abs_z=float(np.abs(z[live]).max()) if live.any() else 0.0)
    return out


def draw(ref, U):
    """Step 6 on the reference's own integers: the token for the 64-bit uniform U."""
    wi = [int(x) for x in ref["wi"]]
    W = sum(wi)
    r = (int(U) * W) >> 64
    acc = 0
    for i, x in enumerate(wi):
        acc += x
        if acc > r:
            return i
    return 0


def draw_many(ref, U):
    """`draw` for an array of uniforms (uint64), vectorised: exact with python integers behind an object array."""
    cdf = np.cumsum(ref["wi"].astype(np.int64))            # a row's weights sum to less than V * 2^40: int64 holds them
    W = int(cdf[-1])
    r = np.array([(int(u) * W) >> 64 for u in np.asarray(U).ravel()], dtype=np.int64)
    tok = np.searchsorted(cdf, r, side="right")            # the smallest i with cdf[i] > r
    return np.where(tok < cdf.size, tok, 0).astype(np.int64).reshape(np.asarray(U).shape)


def check_draw(ref, token, U):
    """The interval rule -> None, or a string that says what is wrong with `token` as the draw for the uniform U."""
    w = ref["w"]
    i = int(token)
    if ref["total"] == 0.0:
        return None if i == 0 else f"token {i} from a row with nothing left (0 expected)"
    if not (0 <= i < w.size) or not w[i] > 0:
        return f"token {i} has no weight in the reference"
    cdf = np.cumsum(w)
    x = (int(U) / 2.0 ** 64) * ref["total"]
    lo = cdf[i - 1] if i > 0 else 0.0
    d = delta(ref)
    if not (lo - d <= x <= cdf[i] + d):
        return f"token {i}: u * total = {x!r} outside [{lo!r}, {cdf[i]!r}] by more than delta = {d!r}"
    return None


def chi_square(counts, probs):
    """Pearson's statistic of observed counts against probabilities (entries with probability 0 must have count 0) and its degrees
    of freedom."""
    counts = np.asarray(counts, dtype=np.float64)
    probs = np.asarray(probs, dtype=np.float64)
    live = probs > 0
    assert counts[~live].sum() == 0, "a token outside the kept set was drawn"
    n = counts.sum()
    exp = probs[live] / probs[live].sum() * n
    return float(((counts[live] - exp) ** 2 / exp).sum()), int(live.sum()) - 1


def chi_square_quantile(df, z=4.753424308822899):
    """Wilson-Hilferty's approximation of the chi-square quantile; the default z is the normal quantile of 1 - 1e-6."""
    a = 2.0 / (9.0 * df)
    return df * (1.0 - a + z * math.sqrt(a)) ** 3


def distribution_fixture():
    """The V = 64 row of the distribution tests with its settings (T = 0.7, top_k = 12, top_p = 0.9)."""
    g = np.random.default_rng(26)
    row = (g.standard_normal(64) * 1.1).astype(np.float32)
    row.setflags(write=False)
    return row, 0.7, 12, 0.9


def golden_row(seed, V):
    """The fp32 row of an HF warper golden (tools/make_goldens_sampling.py stores seeds, not rows)."""
    return (np.random.default_rng(int(seed)).standard_normal(int(V)) * 1.5).astype(np.float32)
