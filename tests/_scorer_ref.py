"""Host references of the CLIP and BLIP-2 scorer kernels that run outside the towers (csrc/clip.hip, csrc/blip2_itm.hip): the text
embeddings, the pooled heads and the score kernels, for tests/test_scorer_kernels_gpu.py.  Plain numpy in float64; every rounding
operation returns the expected values AND a bound on an fp32 kernel's absolute error, derived here from the order in which the
kernels sum (never from what they give).  The case lists and input builders of the GPU file live here too, so that
tests/test_scorer_ref_cpu.py can hold a sequential fp32 implementation to the same bounds on the same inputs where there is no GPU.
Never imported by the product package."""
import math

import numpy as np

from _elementwise_ref import U, layernorm64

F32_MIN_NORMAL = 2.0 ** -126
# test_kernels_gpu.py::test_layernorm's bound on ln_row (csrc/ln.h) against float64, which itm_embed_text runs; the copy the
# elementwise tests hold it to is test_elementwise_kernels_gpu.TOL_LN_F32 (test_scorer_ref_cpu.py asserts they are one number)
TOL_LN_F32 = 2e-5

# ---- how the kernels sum ------------------------------------------------------------------------------------------------------
# A dot product over n terms: lane l of a wave adds the terms l, l + 64, ... in one fma chain (ceil(n / 64) roundings: a fused
# multiply-add rounds once), then the 64 lane sums meet in wave_sum's 6-step tree.  A term is therefore touched by at most
# ceil(n / 64) + 6 roundings, and |fl(sum) - sum| <= ((1 + u)^k - 1) sum |term| for k roundings.  Every bound below writes that
# factor as (k + 1) u: k <= 64 here and (1 + u)^64 - 1 - 64 u < 1e-3 u, so the one extra u covers every second-order term.


def dot_roundings(n):
    return math.ceil(n / 64) + 6


# block_sum of the two heads: a thread adds the terms t, t + 256, ... (ceil(n / 256) roundings), then an 8-step tree over the 256
# thread sums in LDS.
def block_roundings(n):
    return math.ceil(n / 256) + 8


# The L2 normalisation of both heads, as MEAN_POOL_NORM_U (_elementwise_ref.py) has it for the sentence pooler: the squares are
# fused into the chain, so the sum of squares carries block_roundings(P) <= 12 roundings on non-negative terms (relative errors do
# not amplify); the root halves them (6 u) and adds its own, the division one more: 8 u.  10 u with the second-order terms and with
# those of the first-order carry (e_p + |o_p| ||e||_2) / ||y|| below, which are of order (||e|| / ||y||)^2.
HEAD_NORM_U = 10
# expf: OpenCL's and HIP's documented limit for single-precision exp is 3 ulp at the most = 6 u relative.
EXP_U = 6


def _normalise(y, e_y, floor):
    """rows y float64 [n, P] known to within e_y -> (y / max(||y||, floor), the bound).  Dividing by the norm of the computed vector
    carries e to (e_p + |o_p| ||e||_2) / ||y|| (o = y / ||y||: the first term is the numerator's error, the second the norm's,
    which moves by at most ||e||_2), plus HEAD_NORM_U u |o_p| for the norm's own arithmetic and the division."""
    nrm = np.maximum(np.sqrt((y * y).sum(-1, keepdims=True)), floor)
    out = y / nrm
    bound = (e_y + np.abs(out) * np.sqrt((e_y * e_y).sum(-1, keepdims=True))) / nrm + HEAD_NORM_U * U * np.abs(out)
    return out, bound


def within(got, ref, bound, what, label=None):
    """assert |got - ref| <= bound elementwise -> the worst error / bound; with a label, prints the figures first (the GPU file's
    MEASURE lines)"""
    got = np.asarray(got, dtype=np.float64)
    assert np.isfinite(bound).all() and (bound >= 0).all(), what
    assert np.isfinite(got).all(), f"{what}: not finite"
    err = np.abs(got - ref)
    ratio = np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0)
    if label:
        print(f"{label} {what}: max error {err.max():.3e}, worst error / bound {ratio.max():.3f}")
    assert (err <= bound).all(), f"{what}: error {err.max():.3e}, {ratio.max():.2f} x the bound"
    return float(ratio.max())


def embed_rows32(ids, L, table, pos):
    """table[clamp(ids[r], 0, V - 1)] + pos[r % L]: one fp32 addition per element, which rounds on the host as on the device"""
    ids = np.clip(np.asarray(ids, dtype=np.int64), 0, table.shape[0] - 1)
    return (table[ids] + pos[np.arange(len(ids)) % L]).astype(np.float32)


def clip_embed_text64(ids, L, tok, pos):
    """-> (the rows, a bound of zero: the kernel must give exactly these bits)"""
    y = embed_rows32(ids, L, tok, pos).astype(np.float64)
    return y, np.zeros_like(y)


def itm_embed_text64(ids, L, word, pos, gamma, beta, eps):
    """-> (LayerNorm in float64 of the fp32 sums, the bound this LayerNorm already has: test_layernorm's 2e-5)"""
    y = layernorm64(embed_rows32(ids, L, word, pos), gamma, beta, eps)
    return y, np.full_like(y, TOL_LN_F32)


def head_rows(B, rows_per, lens):
    """the row of x each of the B outputs reads: b * rows_per, + clamp(lens[b], 1, rows_per) - 1 when lens is given"""
    off = np.zeros(B, dtype=np.int64) if lens is None else np.clip(np.asarray(lens, dtype=np.int64)[:B], 1, rows_per) - 1
    return np.arange(B) * rows_per + off


def clip_head64(x, rows_per, lens, gamma, beta, eps, W):
    """x fp32 [B * rows_per, D], W fp32 [P, D] -> (float64 [B, P] = normalise(LayerNorm(x[row_b]) W^T), the bound).

    LayerNorm (block_sum, two passes), with nb = block_roundings(D) and s' = sqrt(var + eps):
      mean: nb roundings in the sum and one in the division: e_mu = (nb + 2) u mean|x|.
      rstd: the centred values carry u each (2 u on a square); their sum nb, the division by D and the addition of eps one each
        (non-negative terms throughout): (nb + 4) u on var + eps, halved by the root, + the root + the reciprocal, + 1 u second
        order: rho = ((nb + 4) / 2 + 3) u.  A mean off by e_mu moves sum (x - mean)^2 by exactly D e_mu^2 (the cross term is
        zero): e_mu^2 / (2 s'^2) more on rstd.
      z_d = (x_d - mean) rstd: the mean's error is the SAME number m, |m| <= e_mu, in every channel - it reaches the row as
        -m gamma_d / s' and y_p as -(m / s') sum_d w_pd gamma_d, a signed sum: e_mu / s' |sum_d w_pd gamma_d| bounds it (carrying
        it through sum_d |w_pd gamma_d| instead would hide a whole one-pass variance on a row whose mean is 50 times its spread).
        What differs by channel: u |c_d| from the subtraction, (rho + u) |z_d| from rstd and the product, times gamma_d
        (u |z_d gamma_d|), plus beta_d (u |ln_d|), one more u |z_d| for second order, and the same relative errors on the mean's
        share: e_d = |gamma_d| (rho + 4 u) (|z_d| + e_mu / s') + u |ln_d|
      (a compiler that contracts the product and the sum into one fma rounds less, not more).
    Projection: the per-channel errors reach y_p as sum_d |w_pd| e_d, the dot product of the computed row adds
    (dot_roundings(D) + 1) u sum_d |w_pd| (|ln_d| + e_d + |gamma_d| e_mu / s').  Then _normalise, without a floor (HF divides by the
    plain norm)."""
    x = np.asarray(x)
    P, D = W.shape
    B = x.shape[0] // rows_per
    xr = x[head_rows(B, rows_per, lens)].astype(np.float64)
    g, be, Wa = np.asarray(gamma, np.float64), np.asarray(beta, np.float64), np.abs(W.astype(np.float64))
    mu = xr.mean(-1, keepdims=True)
    c = xr - mu
    sd = np.sqrt((c * c).mean(-1, keepdims=True) + eps)
    z = c / sd
    ln = z * g + be
    nb = block_roundings(D)
    e_mu = (nb + 2) * U * np.abs(xr).mean(-1, keepdims=True)
    rho = ((nb + 4) / 2 + 3) * U + e_mu ** 2 / (2 * sd ** 2)
    shift = e_mu / sd                                             # the mean's error in units of the row's spread, [B, 1]
    e_ln = np.abs(g) * (rho + 4 * U) * (np.abs(z) + shift) + U * np.abs(ln)
    W64 = W.astype(np.float64)
    y = ln @ W64.T
    e_y = shift * np.abs(W64 @ g)[None, :] + e_ln @ Wa.T + (dot_roundings(D) + 1) * U * ((np.abs(ln) + e_ln + np.abs(g) * shift) @ Wa.T)
    return _normalise(y, e_y, 0.0)


def itc_head64(x, rows_per, W, bias):
    """x fp32 [n * rows_per, D] -> (float64 [n, P] = F.normalize(x[r * rows_per] W^T + bias), the bound).  The bias is one more term
    of each sum and its addition one more rounding on all of them: (dot_roundings(D) + 2) u (sum_d |x_d w_pd| + |bias_p|)."""
    x = np.asarray(x)
    n = x.shape[0] // rows_per
    xr = x[np.arange(n) * rows_per].astype(np.float64)
    W64, b64 = W.astype(np.float64), np.asarray(bias, np.float64)
    y = xr @ W64.T + b64
    e_y = (dot_roundings(W.shape[1]) + 2) * U * (np.abs(xr) @ np.abs(W64).T + np.abs(b64))
    return _normalise(y, e_y, 1e-12)


def _pair_dots(img, txt, paired):
    """img [Ni, ..., P], txt [Nt, P] float64 -> (dots, sums of |products|) of shape [Ni, ...] (paired) or [Ni, Nt, ...]"""
    if paired:
        t = txt.reshape((txt.shape[0],) + (1,) * (img.ndim - 2) + (txt.shape[1],))
        return (img * t).sum(-1), (np.abs(img) * np.abs(t)).sum(-1)
    d = np.einsum("i...p,jp->ij...", img, txt)
    a = np.einsum("i...p,jp->ij...", np.abs(img), np.abs(txt))
    return d, a


def clip_logits64(img, txt, logit_scale, paired):
    """-> (float64 exp(s) img . txt^T for the fp32 scale s, [Ni] paired or [Ni, Nt]; the bound).  The dot product is within
    (dot_roundings(P) + 1) u sum |products|; expf within EXP_U u relative, the product one rounding, one more u for second order."""
    img, txt = np.asarray(img, np.float64), np.asarray(txt, np.float64)
    E = math.exp(float(np.float32(logit_scale)))
    d, a = _pair_dots(img, txt, paired)
    return E * d, E * ((dot_roundings(img.shape[-1]) + 1) * U * a + (EXP_U + 2) * U * np.abs(d))


def itc_scores64(img, txt, paired):
    """img fp32 [Ni, nq, P] -> (float64 max over the nq rows of img . txt, the bound).  A maximum moves by no more than its
    arguments do (|max a - max b| <= max |a - b|) and rounds nothing itself: the largest of the nq dot-product bounds.
    Also returns the row at which the float64 maximum stands."""
    img, txt = np.asarray(img, np.float64), np.asarray(txt, np.float64)
    d, a = _pair_dots(img, txt, paired)
    return d.max(-1), (dot_roundings(img.shape[-1]) + 1) * U * a.max(-1), d.argmax(-1)


def itm_head64(x, W, bias):
    """x fp32 [B, nq, D], W fp32 [2, D], bias [2] -> (logits float64 [B, 2] = mean_q (x_q W^T + bias), their bound, prob [B] =
    softmax(logits)[1], its bound).

    Logits: a product passes dot_roundings(D) roundings in its wave, one in the addition of the bias, nq - 1 in the running sum
    over the rows and one in the division by nq: (dot_roundings(D) + nq + 2) u times the mean over q of sum_d |x_d w_d| + |bias|.
    prob = 1 / (1 + exp(-t)) with t = l1 - l0 (the kernel subtracts the larger logit, so one exponent is exactly 0): t is known to
    e_t = e_l0 + e_l1 + u |t| (the subtraction rounds once), exp(-|t|) to the relative r = e_t + EXP_U u, and d prob / d log x =
    prob (1 - prob) <= 1 / 4 everywhere, so prob moves by at most prob (1 - prob) (exp(r) - 1); the sum 1 + x, the division and the
    second order: 3 u prob.  An exponent below fp32's normal range may be rounded on the subnormal grid or flushed to 0: 2^-126."""
    x = np.asarray(x, np.float64)
    nq, D = x.shape[1], x.shape[2]
    W64, b64 = W.astype(np.float64), np.asarray(bias, np.float64)
    logits = (x @ W64.T + b64).mean(1)
    e_l = (dot_roundings(D) + nq + 2) * U * (np.abs(x) @ np.abs(W64).T + np.abs(b64)).mean(1)
    t = logits[:, 1] - logits[:, 0]
    x_ = np.exp(-np.abs(t))
    p_hi, p_lo = 1.0 / (1.0 + x_), x_ / (1.0 + x_)                      # sigmoid(|t|), sigmoid(-|t|): no cancellation either way
    prob = np.where(t >= 0, p_hi, p_lo)
    r = e_l.sum(-1) + U * np.abs(t) + EXP_U * U
    e_p = p_hi * p_lo * np.expm1(r) + 3 * U * prob + F32_MIN_NORMAL
    return logits, e_l, prob, e_p


# ---- the cases of tests/test_scorer_kernels_gpu.py and their inputs ---------------------------------------------------------------
EPS = 1e-5             # the CLIP towers' LayerNorm eps
ITM_EPS = 1e-12        # the Q-Former's
FAMILIES = ("gauss", "offset", "massive", "gains")

# (D, P, B, rows_per, lens given, family).  D: one thread; one lane short of / exactly / one lane into a second 64-stride; one
# thread short of / into a second 256-stride; CLIP's widths; a width that is no multiple of 8; the limit.  P: fewer outputs than
# waves (1, 3), one into a second round of four (5), around one block_sum stride (255, 257), CLIP's, the limit.
CLIP_HEAD_CASES = [
    (1, 1, 1, 1, False, "gauss"),
    (63, 3, 5, 7, True, "offset"),
    (64, 5, 5, 1, False, "massive"),
    (65, 255, 5, 7, True, "gains"),
    (255, 257, 1, 7, True, "gauss"),
    (257, 512, 5, 1, True, "offset"),
    (768, 512, 5, 7, True, "massive"),
    (1000, 1024, 5, 7, False, "gains"),
    (1024, 1024, 5, 7, True, "gauss"),
    (1024, 1, 1, 1, False, "offset"),
    (1, 1024, 5, 7, True, "massive"),
    (768, 3, 1, 7, True, "gains"),
    (255, 5, 5, 1, False, "offset"),
]

# (D, P, n, rows_per, bias): "random", or "zero" with row 3 of the input all zero
ITC_HEAD_CASES = [
    (1, 1, 1, 1, "random"),
    (63, 3, 5, 6, "random"),
    (64, 5, 5, 1, "zero"),
    (65, 255, 5, 6, "random"),
    (255, 257, 1, 6, "random"),
    (257, 512, 5, 1, "random"),
    (768, 512, 5, 6, "zero"),
    (1000, 1024, 5, 6, "random"),
    (1024, 1024, 5, 1, "random"),
    (1024, 1, 5, 6, "random"),
    (1, 1024, 5, 6, "zero"),
    (768, 3, 1, 1, "random"),
]

# (D, L, M): M = B L rows with M % 4 = 1, 2 or 3 (a last block of four waves that is not full)
CLIP_EMBED_CASES = [(1, 1, 5), (63, 5, 15), (65, 77, 154), (512, 5, 5), (1000, 77, 77), (512, 1, 7)]
# (D, L, M): widths around one float4 per lane (248, 256, 264) and around four (1016, 1024); M % 4 != 0, the last caption cut short
# where L = 32
ITM_EMBED_CASES = [(8, 1, 5), (248, 5, 15), (256, 32, 69), (264, 5, 7), (768, 32, 37), (1016, 1, 7), (1024, 5, 10)]
EMBED_V = 11

# (Ni, Nt, P, logit_scale): every shape is run as a matrix, (7, 7) and (1, 1) paired too
CLIP_LOGITS_CASES = [
    (1, 1, 1, 0.0),
    (3, 5, 63, math.log(100.0)),
    (2, 9, 65, -2.0),
    (7, 7, 256, math.log(100.0)),
    (7, 7, 1000, 0.0),
    (3, 5, 1000, -2.0),
    (2, 9, 1, math.log(100.0)),
    (7, 7, 63, -2.0),
    (1, 1, 256, 0.0),
]

# (Ni, Nt, P, nq, where the maximum is planted: "first" / "middle" / "last", sign of every score)
ITC_SCORES_CASES = [
    (1, 1, 1, 1, "first", 1),
    (3, 5, 63, 3, "first", 1),
    (2, 9, 65, 32, "middle", 1),
    (7, 7, 256, 32, "last", 1),
    (7, 7, 1000, 3, "middle", -1),
    (3, 5, 1000, 32, "first", -1),
    (2, 9, 1, 3, "last", -1),
    (7, 7, 63, 32, "first", -1),
    (1, 1, 256, 3, "last", 1),
    (3, 5, 65, 1, "first", -1),
]

# (B, nq, D, bias): "random", or "+200" / "-200": l1 - l0 = +-200 to within the products' share
ITM_HEAD_CASES = [
    (1, 1, 1, "random"),
    (5, 3, 63, "random"),
    (5, 32, 65, "random"),
    (1, 32, 768, "random"),
    (5, 3, 1000, "random"),
    (5, 1, 768, "random"),
    (1, 3, 1000, "random"),
    (5, 32, 1, "random"),
    (5, 3, 768, "+200"),
    (5, 32, 65, "-200"),
]


def _rng(tag, case):
    return np.random.default_rng([tag] + list(repr(tuple(case)).encode()))      # the case's own text: the same stream in every process


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def clip_head_inputs(case):
    """-> dict(x [B * rows_per, D] with NaN in every row the head must not read, rows_per, lens or None, gamma, beta, W)"""
    D, P, B, rows_per, has_lens, fam = case
    rng = _rng(1, case)
    rows = rng.standard_normal((B, D))
    if fam == "offset":                                           # a mean 50 times the row's spread: a one-pass variance would cancel
        spread = rng.uniform(0.5, 2.0, (B, 1))
        rows = rows * spread + 50.0 * spread
    if fam == "massive":                                          # one channel 300 times the others (ViT / CLIP outlier features)
        rows[:, D // 3] *= 300.0
    gamma, beta = rng.standard_normal(D), rng.standard_normal(D)
    if fam == "gains":                                            # log-uniform over [0.05, 20], either sign
        gamma = np.exp(rng.uniform(math.log(0.05), math.log(20.0), D)) * rng.choice([-1.0, 1.0], D)
    lens = None
    if has_lens:                                                  # clamped to [1, rows_per]: 0 -> first row, rows_per + 3 -> last
        lens = np.array([0, 1, rows_per, rows_per + 3, (rows_per + 1) // 2][:B] if B > 1 else [rows_per + 3], dtype=np.int32)
    x = np.full((B * rows_per, D), np.nan, dtype=np.float32)
    x[head_rows(B, rows_per, lens)] = rows
    W = rng.standard_normal((P, D)) / math.sqrt(D)
    return dict(x=x, rows_per=rows_per, lens=lens, gamma=_f32(gamma), beta=_f32(beta), W=_f32(W), B=B, D=D, P=P)


def itc_head_inputs(case):
    D, P, n, rows_per, bias_kind = case
    rng = _rng(2, case)
    x = np.full((n * rows_per, D), np.nan, dtype=np.float32)
    x[np.arange(n) * rows_per] = rng.standard_normal((n, D)) + 0.5
    bias = rng.standard_normal(P)
    if bias_kind == "zero":
        bias[:] = 0.0
        x[3 * rows_per] = 0.0                                     # F.normalize's eps: zeros, not NaN
    W = rng.standard_normal((P, D)) / math.sqrt(D)
    return dict(x=x, rows_per=rows_per, W=_f32(W), bias=_f32(bias), n=n, D=D, P=P)


def embed_inputs(case, tag):
    """-> dict(ids [M] with -3, 0, V - 1 and V + 5 among them, table [V, D], pos [L, D], gamma, beta)"""
    D, L, M = case
    rng = _rng(tag, case)
    ids = rng.integers(0, EMBED_V, M).astype(np.int32)
    bad = np.array([-3, 0, EMBED_V - 1, EMBED_V + 5], dtype=np.int32)
    ids[rng.permutation(M - 1)[:4]] = bad                         # (every case has M >= 5)
    ids[M - 1] = EMBED_V + 5                                      # the last row of the partial block reads the table's last row
    table = rng.standard_normal((EMBED_V, D)) * 3 + 1
    pos = rng.standard_normal((L, D))
    return dict(ids=ids, L=L, table=_f32(table), pos=_f32(pos), gamma=_f32(rng.standard_normal(D)), beta=_f32(rng.standard_normal(D)),
                M=M, D=D)


def _unit(a):
    return a / np.sqrt((a * a).sum(-1, keepdims=True))


def clip_logits_inputs(case):
    """unit rows as the heads give them; caption j < Ni leans towards image j (cosine about 0.3)"""
    Ni, Nt, P, scale = case
    rng = _rng(4, case)
    img = _unit(rng.standard_normal((Ni, P)))
    txt = rng.standard_normal((Nt, P)) / math.sqrt(P)
    k = min(Ni, Nt)
    txt[:k] += 0.3 * img[:k]
    return dict(img=_f32(img), txt=_f32(_unit(txt)), scale=float(np.float32(scale)), Ni=Ni, Nt=Nt, P=P)


def itc_scores_inputs(case):
    """img[i, q] = a_q base + nu noise_i, txt[j] = sign * unit(base + 0.3 g_j), all directions of unit length: the noise is shared by
    the nq rows of an image, so the order of its nq scores is the order of a_q (1 at the planted row and 0.5 elsewhere for
    positive scores; the planted row's -0.5 is the LEAST negative against -1 elsewhere), whatever nu is; nu = min(4, 0.15 sqrt(P))
    keeps every score's sign (noise . txt has deviation nu / sqrt(P) <= 0.15 against |a_q| cos >= 0.45) while the products of a
    score change sign, as they do between two embeddings that are not copies of each other."""
    Ni, Nt, P, nq, where, sign = case
    rng = _rng(5, case)
    base = np.ones(1) if P == 1 else _unit(rng.standard_normal(P))
    q_star = {"first": 0, "middle": nq // 2, "last": nq - 1}[where]
    a = np.full(nq, 0.5 if sign > 0 else -1.0)
    a[q_star] = 1.0 if sign > 0 else -0.5
    nu = min(4.0, 0.15 * math.sqrt(P))
    noise = _unit(rng.standard_normal((Ni, 1, P)))
    img = a[None, :, None] * base[None, None, :] + nu * noise
    txt = _unit(base[None, :] + 0.3 * _unit(rng.standard_normal((Nt, P))))
    return dict(img=_f32(img), txt=_f32(txt), Ni=Ni, Nt=Nt, P=P, nq=nq, q_star=q_star, sign=sign)


def itm_head_inputs(case):
    B, nq, D, bias_kind = case
    rng = _rng(6, case)
    x = rng.standard_normal((B, nq, D)) + 0.25
    W = rng.standard_normal((2, D)) / math.sqrt(D)
    bias = rng.standard_normal(2)
    if bias_kind != "random":                                     # logits near -+100: exp(+-200) has left fp32 on both sides
        s = 1.0 if bias_kind == "+200" else -1.0
        bias = np.array([-100.0 * s, 100.0 * s])
    return dict(x=_f32(x), W=_f32(W), bias=_f32(bias), B=B, nq=nq, D=D)
