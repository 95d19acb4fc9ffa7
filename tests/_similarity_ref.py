"""Host reference of the caption-similarity kernels (csrc/similarity.hip: cap_cosine_matrix, cap_group_similarity) for
tests/test_similarity_kernels_gpu.py and tests/test_similarity_ref_cpu.py.  Plain numpy in float64, written from the definitions:

    e^_i = e_i / max(||e_i||, 1e-12),  s_ij = e^_i . e^_j,  W = sum w_i
    a weighted statistic is the unweighted statistic of the group with row i repeated w_i times
    disagreement = sum_ij w_i w_j (1 - s_ij) / W^2 (diagonal included; empty group 0)
    pairs = W (W - 1) / 2;  pair_mean / pair_var = mean / population variance of s over the unordered pairs of the expanded group
    row_mean_i = (sum_j w_j s_ij - s_ii) / (W - 1) (0 when W == 1);  medoid = first row with the largest row_mean (-1 when empty)

`group_stats64` evaluates the weighted closed forms, `expanded_stats64` repeats the rows literally and knows no weights; the CPU
file holds the one against the other.  Every reference returns, next to the values, a bound on an fp32 kernel's ABSOLUTE error,
derived below from the order in which the kernels sum (chain lengths, tree depths, the norm's floor) - never from what they give.
The case builder of the GPU file lives here too so that the CPU file can hold a sequential fp32 implementation to the same bounds on
the same inputs.  Never imported by the product package."""
import math
import os
import re

import numpy as np

U = 2.0 ** -24                 # unit roundoff of fp32
TINY = 2.0 ** -149             # a product that underflows is off by at most this
FLOOR = 1e-12
_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "embodied_captioning_amd", "csrc", "similarity.hip")


def kernel_constant(name):
    """an integer `constexpr int NAME = value;` of csrc/similarity.hip: the tile sizes the case list is built around"""
    m = re.search(r"constexpr int %s = (\d+);" % name, open(_SRC).read())
    assert m, name
    return int(m.group(1))


SIM_TILE = kernel_constant("SIM_TILE")      # rows of a Gram tile = rows of a sum-vector chunk
SIM_SUB = kernel_constant("SIM_SUB")        # rows of one wave's accumulator

# ---- how the kernels sum --------------------------------------------------------------------------------------------------
# k roundings on a sum give |fl(sum) - sum| <= ((1 + u)^k - 1) sum |term|, written (k + 1) u below: k <= 1100 here and
# (1 + u)^1100 - 1 - 1100 u < 0.04 u.  A fused multiply-add rounds once.
#
# A dot product of one wave over D columns (||e||^2, e^_i . m, e^_i . e^_i): lane l takes the float4 at columns 4 l + 256 q, one fma
# chain of 4 ceil(D / 256) links, then the 6-step butterfly.


def dot_roundings(D):
    return 4 * math.ceil(D / 256) + 6


def r_e(D):
    """relative error of a computed e^_i[k], in units of u: the squares are non-negative, so ||e||^2 carries dot_roundings(D) u; the
    root halves that and adds one; fmaxf with fl32(1e-12) (one more u against the definition's 1e-12: max is 1-Lipschitz); the
    reciprocal one; the product e * inv one; one for the second-order terms."""
    return dot_roundings(D) / 2 + 5


def s_bound(na, nb, D):
    """|s^ - s| for rows whose TRUE normalised lengths are na, nb (1, or less for a row under the floor; arrays broadcast): the MFMA
    is a D-link fma chain ((D + 1) u sum |e^_i e^_j| <= (D + 1) u na nb by Cauchy-Schwarz), each factor is off by r_e u, and each
    of the D products may underflow."""
    return (D + 1 + 2 * r_e(D) + 1) * U * na * nb + D * TINY


TILE_CHAIN = 16      # one 32 x 32 accumulator: 16 registers a lane, one fma chain for sum w s and one for sum w s^2; fp64 above
CHUNK_CHAIN = SIM_TILE   # the sum vector: one fma chain over a chunk's rows per column; chunks are added in fp64, rounded to fp32 once


def normalise64(e):
    e = np.asarray(e, dtype=np.float64)
    n = np.sqrt((e * e).sum(-1))
    eh = e / np.maximum(n, FLOOR)[:, None]
    return eh, np.sqrt((eh * eh).sum(-1))


def cosine64(a, b):
    """-> (s float64 [Na, Nb], bound)"""
    ah, na = normalise64(a)
    bh, nb = normalise64(b)
    return ah @ bh.T, s_bound(na[:, None], nb[None, :], np.asarray(a).shape[1])


def _pair_weights(w):
    """weight of the unordered pair (i, j), i <= j, of the expanded group: w_i w_j, and w_i (w_i - 1) / 2 among a row's own copies"""
    pw = np.triu(np.outer(w, w), 1)
    pw[np.diag_indices(len(w))] = w * (w - 1) / 2
    return pw


def group_stats64(e, w):
    """One group: rows e [n, D] (fp32 values), counts w [n] -> dict of values and of bounds ('*_bound')."""
    e = np.asarray(e, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    n, D = e.shape
    out = {"row_mean": np.zeros(n), "row_mean_bound": np.zeros(n)}
    if n == 0:
        out.update(disagreement=0.0, disagreement_bound=0.0, pairs=0, pair_mean=0.0, pair_mean_bound=0.0, pair_var=0.0,
                   pair_var_bound=0.0, medoid=-1, gap=math.inf)
        return out
    eh, nh = normalise64(e)
    s = eh @ eh.T
    W = w.sum()
    re = r_e(D)
    # the sum vector m = sum_j w_j e^_j: a chain of CHUNK_CHAIN fmas per chunk on terms that are off by r_e u, the fp32 rounding of
    # the total -> |dm[d]| <= (CHUNK_CHAIN + 1 + r_e + 1) u A[d], A[d] = sum_j w_j |e^_j[d]|
    m = (w[:, None] * eh).sum(0)
    A = (w[:, None] * np.abs(eh)).sum(0)
    dm = (CHUNK_CHAIN + 2 + re) * U * A + n * TINY
    # disagreement = 1 - m . m / W^2, the squares and their sum in fp64, rounded to fp32 at the end
    dis = 1.0 - (m @ m) / W ** 2
    out["disagreement"] = dis
    out["disagreement_bound"] = float((2 * np.abs(m) * dm + dm * dm).sum() / W ** 2 + U * abs(dis) + 1e-14)
    # row_mean: t_i = e^_i . m as one wave's dot product (dot_roundings u sum |e^_i m|, e^_i off by r_e u, m off by dm), s_ii the same
    # way; the difference and the division are fp64, the result rounded to fp32
    kd = dot_roundings(D)
    if W > 1:
        t = eh @ m
        absdot = np.abs(eh) @ np.abs(m)
        t_b = (kd + 1 + re) * U * absdot + np.abs(eh) @ dm + D * TINY
        sii = np.diag(s)
        sii_b = (kd + 1 + 2 * re) * U * sii + D * TINY
        rm = (t - sii) / (W - 1)
        out["row_mean"] = rm
        out["row_mean_bound"] = (t_b + sii_b) / (W - 1) + U * np.abs(rm) + 1e-14
    rm = out["row_mean"]
    out["medoid"] = int(np.argmax(rm))
    srt = np.sort(rm)
    out["gap"] = float(srt[-1] - srt[-2]) if n > 1 else math.inf
    # the pairs: every s_ij off by s_bound; a lane's chain adds TILE_CHAIN roundings to sum w s, one more (w s is rounded before it
    # is fused with s) to sum w s^2; the rest is fp64
    pw = _pair_weights(w)
    npairs = W * (W - 1) / 2
    out["pairs"] = int(npairs)
    if npairs > 0:
        b = s_bound(nh[:, None], nh[None, :], D)
        mean = (pw * s).sum() / npairs
        m2 = (pw * s * s).sum() / npairs
        mean_b = (pw * (b + (TILE_CHAIN + 1) * U * (np.abs(s) + b))).sum() / npairs + 1e-14
        m2_b = (pw * (b * (2 * np.abs(s) + b) + (TILE_CHAIN + 2) * U * (np.abs(s) + b) ** 2)).sum() / npairs + 1e-14
        var = max(0.0, m2 - mean * mean)
        out.update(pair_mean=mean, pair_mean_bound=float(mean_b + U * abs(mean)), pair_var=var,
                   pair_var_bound=float(m2_b + mean_b * (2 * abs(mean) + mean_b) + U * var))
    else:
        out.update(pair_mean=0.0, pair_mean_bound=0.0, pair_var=0.0, pair_var_bound=0.0)
    return out


def expanded_stats64(e, w):
    """The definition taken literally: repeat row i w_i times and compute every statistic with no weights at all.  row_mean / medoid
    are reported per ORIGINAL row (all copies of a row share a value; the first copy of the best row is the expanded medoid)."""
    e = np.asarray(e, dtype=np.float64)
    w = np.asarray(w).astype(np.int64)
    idx = np.repeat(np.arange(len(w)), w)
    n = len(idx)
    if n == 0:
        return dict(disagreement=0.0, pairs=0, pair_mean=0.0, pair_var=0.0, row_mean=np.zeros(0), medoid=-1)
    eh, _ = normalise64(e[idx])
    s = eh @ eh.T
    iu = np.triu_indices(n, 1)
    vals = s[iu]
    rm = (s.sum(1) - np.diag(s)) / (n - 1) if n > 1 else np.zeros(n)
    first = np.concatenate([[0], np.cumsum(w)[:-1]])
    return dict(disagreement=float((1.0 - s).mean()), pairs=n * (n - 1) // 2, pair_mean=float(vals.mean()) if len(vals) else 0.0,
                pair_var=float(vals.var()) if len(vals) else 0.0, row_mean=rm[first],
                medoid=int(idx[int(np.argmax(rm))]))


# ---- the GPU file's inputs ---------------------------------------------------------------------------------------------------
# 8 and 384 (production); 100 is neither a multiple of 8 (a half-empty last k-step) nor of the kernel's 64-column LDS pass (a partial
# last pass after a whole one)
DIMS = (8, 100, 384)
# the sizes the issue names, one below / at / above each tile dimension of the kernel, and a group of more than two whole tiles
PLAIN_SIZES = sorted({0, 1, 2, 3, 63, 64, 65, SIM_SUB - 1, SIM_SUB, SIM_SUB + 1, SIM_TILE - 1, SIM_TILE, SIM_TILE + 1,
                      2 * SIM_TILE + 2})
# The one group on which the medoid is NOT compared (the CPU file checks that every other group clears four times the bound): with every
# s within 1e-6 of 1, as the variance case needs, all row means are within 1e-6 of each other - inside the bound whatever the counts.
# `near_pair_and_medoid` is its counterpart with a comparable medoid.
MEDOID_EXEMPT = {"near_duplicates": "every row_mean is within 1e-6 of the others, far inside the bound"}


def _unit(rng, n, D):
    x = rng.standard_normal((n, D))
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def build_case(D, seed=0):
    """-> dict(e fp32 [N, D], offsets [G + 1], weights fp32 [N], names [G]).  Random groups of PLAIN_SIZES with integer counts up to 5,
    then the special groups."""
    rng = np.random.default_rng(1000 * D + seed)
    rows, wts, names, offsets = [], [], [], [0]

    def add(name, x, w=None):
        x = np.asarray(x, dtype=np.float64).reshape(-1, D)
        rows.append(x)
        wts.append(np.asarray(w if w is not None else rng.integers(1, 6, size=len(x)), dtype=np.float64))
        names.append(name)
        offsets.append(offsets[-1] + len(x))

    for n in PLAIN_SIZES:
        # random directions around a common one (so that cosines are not all near zero), random lengths; two rows get unequal counts
        # (with equal ones both row means are s_01)
        base = _unit(rng, 1, D)
        x = _unit(rng, n, D) + 0.6 * base if n else np.zeros((0, D))
        x = x * rng.uniform(0.5, 2.0, size=(n, 1))
        add(f"plain{n}", x, [1.0, 4.0] if n == 2 else None)
    a = _unit(rng, 1, D)
    add("near_duplicates", a + 2e-4 * _unit(rng, 5, D))                       # s = 1 - O(4e-8): pair_var cancels
    # two near-duplicates next to a row x that is the clear medoid: in the plane of (a, p), a at 0, x at 40, y at 80 degrees
    p = _unit(rng, 1, D)
    p = p - (p @ a.T) * a
    p /= np.linalg.norm(p)
    ang = lambda d: math.cos(math.radians(d)) * a + math.sin(math.radians(d)) * p  # noqa: E731
    add("near_pair_and_medoid", np.concatenate([a, a + 1e-4 * _unit(rng, 1, D), ang(40), ang(80)]), [1, 1, 1, 1])
    add("orthogonal", np.concatenate([a, p]), [1, 3])
    add("antipodal", np.concatenate([3 * a, -0.5 * a]), [2, 1])
    add("norms", np.concatenate([1e3 * _unit(rng, 1, D), 1e-20 * _unit(rng, 1, D), _unit(rng, 2, D) + 0.5 * a]), [1, 2, 3, 1])
    z = _unit(rng, SIM_SUB + 1, D) + 0.7 * a
    z[5] = 0.0
    add("zero_row", z)
    t = _unit(rng, 2, D)
    add("tie", np.concatenate([t[:1], t[:1], t[1:]]), [2, 2, 1])              # rows 0 and 1 are the same bits: the first must win
    e = np.concatenate(rows).astype(np.float32)
    return dict(e=e, offsets=np.asarray(offsets, dtype=np.int32), weights=np.concatenate(wts).astype(np.float32), names=names, D=D)


def expand_case(case):
    """the same groups with row i written w_i times and no weights"""
    w = case["weights"].astype(np.int64)
    idx = np.repeat(np.arange(len(w)), w)
    off = np.concatenate([[0], np.cumsum(w)])[case["offsets"]]
    return dict(e=case["e"][idx], offsets=off.astype(np.int32), weights=None, names=case["names"], D=case["D"], origin=idx)


def reference(case):
    """-> list of group_stats64 dicts, one per group"""
    off, w = case["offsets"], case["weights"]
    out = []
    for g in range(len(off) - 1):
        a, b = int(off[g]), int(off[g + 1])
        out.append(group_stats64(case["e"][a:b], w[a:b] if w is not None else np.ones(b - a)))
    return out


def medoid_compared(name, ref):
    """the issue's rule: compare the medoid where the two best row means differ in float64 by more than four times the bound"""
    return name not in MEDOID_EXEMPT and ref["medoid"] >= 0 and ref["gap"] > 4 * float(np.max(ref["row_mean_bound"], initial=0.0))


def matrix_inputs(D, seed=0):
    """a [70, D], b [131, D] for the matrix form (partial tiles on both sides, more than two tiles of columns), special rows included;
    and the paired pair (a2, b2) of 131 rows"""
    rng = np.random.default_rng(77 * D + seed)
    a = _unit(rng, SIM_TILE + 6, D) * rng.uniform(0.5, 2.0, size=(SIM_TILE + 6, 1))
    b = _unit(rng, 2 * SIM_TILE + 3, D) * rng.uniform(0.5, 2.0, size=(2 * SIM_TILE + 3, 1))
    a[1] = 0.0
    a[2] *= 1e3
    a[3] *= 1e-20
    b[0] = a[0] * 2.0                       # parallel
    b[1] = -a[4]                            # antipodal
    b[2] = a[5] + 1e-4 * b[2]               # near-duplicate
    a2 = np.concatenate([a, a[: len(b) - len(a)] * 0.5 + 0.1])
    return a.astype(np.float32), b.astype(np.float32), a2.astype(np.float32)


def worst(got, ref, bound):
    """max |got - ref| / bound (0 / 0 = 0), and whether every element is inside"""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), err.shape)
    ratio = np.where(err == 0, 0.0, err / np.where(bound > 0, bound, np.nan))
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    return float(ratio.max(initial=0.0))
