"""The float64 attention reference of the kernel-by-kernel attention tests, its input classes and the bars derived from it.
Pure host code: torch on the CPU and numpy, nothing else.  tests/test_attention_kernels_gpu.py and
tests/test_vit_attention_classes_gpu.py judge kernels with it; tests/test_attention_ref_cpu.py shows on float64 emulations that
the classes and bars let an ideal kernel pass and catch a defective one.

The reference is softmax(scale q k^T + mask) v per (batch, head).  Inputs are rounded to the kernel's input type BEFORE the
reference sees them, so only the kernel's arithmetic is judged.

Bars (see _figures): the base is MARGIN x ref_err_fp32, ref_err_fp32 = max |the same formula in torch float32 on the CPU - float64|;
where that is 0 the family floor stands in.  On top of it only roundings that a kernel's source states:
  bf16 out        2^-8 |ref| elementwise: half a bf16 ulp of final rounding (ulp <= 2^-7 |x|).
  bf16 MFMA P     2^-8 p_abs elementwise, p_abs = softmax(..) @ |v|.  vit_attention_mfma / _flash / _flash_wide round P to bf16
                  before O^T = V^T.P^T (bf16_pv: `(bf16_t)p[8 * s2 + j]`) and sum the denominator from the unrounded p
                  (att_exp_sum).  The numerator is sum_j p_j (1 + d_j) v_j with |d_j| <= 2^-9 (round to nearest, 8 significant
                  bits), so it moves by at most 2^-9 sum_j p_j |v_j| = 2^-9 p_abs after the division.  The term allowed is
                  2^-8 p_abs, the 2^-8 of the final rounding's term: an ideal kernel stays at or below zero under it
                  (tests/test_attention_ref_cpu.py) and P rounded toward zero is caught by the bias check instead.
  G8 out          the container's own error for the case, max |g8_decode(g8_encode(ref32)) - ref32|.
The split-fp16 kernels (G8 q | k | v) drop the lo.lo term of both products (split_qk, split_pv: hi.lo + lo.hi + hi.hi); they stay within
the base bar with it dropped (profiles/vit_attention_classes_gpu_tolerances.txt), so no term stands for it."""
import math

import numpy as np
import torch

from _util import g8_decode, g8_encode

F32, BF16, SPLIT = 0, 1, 2
G8IN = 3                             # input rounding only: the kernel takes G8 q | k | v (its context is judged as SPLIT)
MARGIN = 8.0


def _rounded(x, dtype):
    """fp32 values as the kernel's input type holds them."""
    return x.to(torch.bfloat16).float() if dtype == BF16 else x.float()


def _rounded_g8(x):
    """fp32 values as a G8 container holds them: g8_decode(g8_encode(x)), groups of 8 along the last axis."""
    return torch.from_numpy(g8_decode(g8_encode(x.float().contiguous().numpy()))).view(x.shape)


def _round_in(x, rounding):
    return _rounded_g8(x) if rounding == G8IN else _rounded(x, rounding)


def _rows(x):
    """[B, H, L, hd] -> [B, L, H * hd], the row layout of every buffer here."""
    B, H, L, hd = x.shape
    return x.permute(0, 2, 1, 3).reshape(B, L, H * hd)


# ---------------------------------------------------------------------------------------------- the reference and the bars
def _attn(q, k, v, mask, scale, dt):
    """softmax(scale q k^T + mask) v per (batch, head) in dtype dt.  q [B, H, Lq, hd], k / v [B, H, Lk, hd], mask bool, broadcastable to
    [B, H, Lq, Lk], True = the query sees the key."""
    q, k, v = q.to(dt), k.to(dt), v.to(dt)
    s = (q @ k.transpose(-1, -2)) * torch.tensor(scale, dtype=dt)
    s = s.masked_fill(~mask, float("-inf"))
    return torch.softmax(s, -1) @ v


def _reference(prob):
    """(float64 reference [B, Lq, H * hd], ref_err_fp32)."""
    ref = _attn(prob["q"], prob["k"], prob["v"], prob["mask"], prob["scale"], torch.float64)
    r32 = _attn(prob["q"], prob["k"], prob["v"], prob["mask"], prob["scale"], torch.float32)
    return _rows(ref), (r32.double() - ref).abs().max().item()


def _p_abs(prob):
    """softmax(scale q k^T + mask) @ |v| in float64, [B, Lq, H * hd]: what a relative rounding of P can move the context by."""
    return _rows(_attn(prob["q"], prob["k"], prob["v"].abs(), prob["mask"], prob["scale"], torch.float64))


def _problem(cls, B, H, Lq, Lk, hd, seed, peaks=(), mask=None, scale=None, dtype=F32):
    """q, k, v of one input class, rounded to the input type of `dtype`.  peaked: slot s = b * H + h leads at key peaks[s % len]."""
    g = torch.Generator().manual_seed(seed)
    scale = 1.0 / math.sqrt(hd) if scale is None else scale
    rn = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    if cls == "randn":
        q, k, v = rn(B, H, Lq, hd) * 1.5, rn(B, H, Lk, hd) * 1.5, rn(B, H, Lk, hd) * 1.5
    else:
        u = rn(B, H, 1, hd)
        u = u / u.norm(dim=-1, keepdim=True) * math.sqrt(hd)          # u . u = hd: key beta u scores scale * beta * hd against query u
        v = rn(B, H, Lk, hd) * 1.5
        if cls == "rising":
            q, k = u + 0.1 * rn(B, H, Lq, hd), 0.02 * rn(B, H, Lk, hd)
            step = min(3.0, 96.0 / Lk)
            k = k + (step * torch.arange(Lk, dtype=torch.float32) / (scale * hd)).view(1, 1, Lk, 1) * u
        else:
            q, k = u + 0.5 * rn(B, H, Lq, hd), 0.5 * rn(B, H, Lk, hd)
            for s in range(B * H):
                b, h = divmod(s, H)
                k[b, h, peaks[s % len(peaks)]] += 20.0 / (scale * hd) * u[b, h, 0]
    if mask is None:
        mask = torch.ones(1, 1, 1, Lk, dtype=torch.bool)
    return {"q": _rounded(q, dtype), "k": _rounded(k, dtype), "v": _rounded(v, dtype), "mask": mask, "scale": scale}


def _problem_in(cls, B, H, Lq, Lk, hd, seed, peaks=(), mask=None, scale=None, rounding=F32):
    """_problem with the input roundings and the class the ViT kernels add.  rounding: F32, BF16 or G8IN (the reference sees
    g8_decode(g8_encode(x))).  positive: the randn class with v = |randn * 1.5| + 0.5, so every context element is at least 0.5
    and a relative error has a sign that a mean can show."""
    prob = _problem("randn" if cls == "positive" else cls, B, H, Lq, Lk, hd, seed, peaks, mask, scale, dtype=F32)
    if cls == "positive":
        prob["v"] = prob["v"].abs() + 0.5
    for name in "qkv":
        prob[name] = _round_in(prob[name], rounding)
    return prob


def _causal_mask(Lq, past=0):
    """query i sees the keys up to past + i, [1, 1, Lq, past + Lq]: the mask of the lq_causal family."""
    Lk = past + Lq
    i, j = torch.arange(Lq).view(Lq, 1), torch.arange(Lk).view(1, Lk)
    return (j <= i + past).view(1, 1, Lq, Lk)


def _sides(bounds, n):
    """first key, last key and both sides of every boundary inside (0, n)."""
    pos = {0, n - 1}
    for b in bounds:
        if 0 < b < n:
            pos.update((b - 1, b))
    return sorted(pos)


def _slots(cls, peaks, H):
    """batch size: peaked cases carry one (batch, head) slot per peak position, the others two batch rows."""
    return max(2, -(-len(peaks) // H)) if cls == "peaked" else 2


FAMILIES = {}            # family -> {"cases": [...], "problem": f(case, cls, dtype)}: each test module registers its own
_FLOOR = {}


def _floor(family):
    """smallest non-zero ref_err_fp32 over the family's randn cases (both input roundings): the bar's base where a case's own is 0."""
    if family not in _FLOOR:
        errs = []
        for case in FAMILIES[family]["cases"]:
            for dt in (F32, BF16):
                e = _reference(FAMILIES[family]["problem"](case, "randn", dt))[1]
                if e > 0:
                    errs.append(e)
        _FLOOR[family] = min(errs)
    return _FLOOR[family]


def _g8_container_err(ref):
    r32 = ref.float().numpy()
    r32 = r32.reshape(-1, r32.shape[-1])
    return float(np.abs(g8_decode(g8_encode(r32)) - r32).max())


def _figures(family, cls, dtype, out, prob, keep=None, ref=None, p_abs=None):
    """out [B, Lq, H * hd] fp32 CPU against the float64 reference; keep: bool [B, Lq] of the rows the contract defines.
    ref: a (reference, ref_err_fp32) pair computed before; p_abs: _p_abs(prob) for a bf16 kernel that rounds P to bf16.
    -> {"max", "worst" (the judged figure), "bar", "err32", "out", "ref"}."""
    ref, err32 = _reference(prob) if ref is None else ref
    base = err32 if err32 > 0 else _floor(family)
    bar = MARGIN * base
    if keep is not None:
        out, ref = out[keep], ref[keep]
        p_abs = p_abs[keep] if p_abs is not None else None
    assert torch.isfinite(out).all(), (family, cls, "non-finite output")
    diff = (out.double() - ref).abs()
    if dtype == BF16:
        left = diff - 2.0 ** -8 * ref.abs()                          # what is left after the final rounding's half ulp
        if p_abs is not None:
            left = left - 2.0 ** -8 * p_abs                           # and after P's rounding to bf16
        worst = left.max().item()
    elif dtype == SPLIT:
        bar += _g8_container_err(ref)
        worst = diff.max().item()
    else:
        worst = diff.max().item()
    return {"max": diff.max().item(), "worst": worst, "bar": bar, "err32": err32, "out": out, "ref": ref}


def _judge(tag, family, case, cls, dtype, out, prob, keep=None, ref=None, p_abs=None):
    """_figures, printed as `max / judged / bar`, asserted.  Returns the figures."""
    f = _figures(family, cls, dtype, out, prob, keep, ref, p_abs)
    print(f"{tag:<58s} {cls:<6s} max {f['max']:.3e}  judged {f['worst']: .3e}  bar {f['bar']:.3e}  ref_err_fp32 {f['err32']:.3e}")
    assert f["worst"] <= f["bar"], (tag, cls, f["worst"], f["bar"])
    return f


# ---------------------------------------------------------------------------------------------- the bias check
BIAS_SIGMAS = 6.0


def _bias(f, dtype, mfma=False):
    """(mean relative error, threshold) of a `positive` case judged by _figures: every reference element is >= 0.5, so an
    elementwise error within the bar is a relative error within r, and the mean of n such errors without a common sign stays
    within 6 r / sqrt(n).  r: bar / 0.5 (f["bar"] holds the container term for a G8 context), plus the relative rounding of the
    output type - 2^-8 for a bf16 context, 2^-7 where P was rounded to bf16 too (2^-8 |ref| + 2^-8 p_abs, p_abs = |ref| here)."""
    ref, out = f["ref"], f["out"].double()
    assert (ref >= 0.5).all(), "the bias check is defined on the positive class only"
    r = f["bar"] / 0.5
    if dtype == BF16:
        r += 2.0 ** -7 if mfma else 2.0 ** -8
    return ((out - ref) / ref).mean().item(), BIAS_SIGMAS * r / math.sqrt(ref.numel())
