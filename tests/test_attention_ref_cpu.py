"""CPU: the input classes and bars of tests/_attention_ref.py bite before any GPU is involved.  float64 emulations of an attention
row set stand in for a kernel: the ideal ones pass every class, each listed defect fails at least one class at N = 197 and at
N = 577, truncated P fails the bias check, and in every peaked case of tests/test_vit_attention_classes_gpu.py the slot's leading
key decides every query row that sees it by more than 100 bars."""
import pytest
import torch

import test_vit_attention_classes_gpu as V
from _attention_ref import BF16, F32, G8IN, SPLIT, _attn, _bias, _figures, _rows

H, HD = 2, 64
CLASSES = V.CLASSES
DEFECT_N = [197, 577]


def _bf16_rn(x):
    return x.float().to(torch.bfloat16).double()


def _bf16_rz(x):
    """toward zero: the low 16 bits of the fp32 image cleared"""
    return (x.float().view(torch.int32) & -65536).view(torch.float32).double()


def _scores(prob):
    s = (prob["q"].double() @ prob["k"].double().transpose(-1, -2)) * prob["scale"]
    return s.masked_fill(~prob["mask"], float("-inf"))


def _emulate(prob, p_round=_bf16_rn, out_round=_bf16_rn, hide=None, pad_copy=False, den_miss=None):
    """the bf16 MFMA kernels in float64: P rounded to bf16, the denominator summed from the unrounded p, one output rounding.
    hide: bool [B, H, 1, Lk] of keys the kernel loses; pad_copy: one padding key counted as a copy of key N - 1; den_miss: a key the
    denominator misses."""
    s, v = _scores(prob), prob["v"].double()
    if hide is not None:
        s = s.masked_fill(hide, float("-inf"))
    if pad_copy:
        s, v = torch.cat([s, s[..., -1:]], -1), torch.cat([v, v[..., -1:, :]], -2)
    p = torch.exp(s - s.max(-1, keepdim=True).values)
    den = p.sum(-1, keepdim=True)
    if den_miss is not None:
        den = den - p[..., den_miss:den_miss + 1]
    return _rows(out_round(p_round(p) @ v / den))


def _emulate_chunks_not_rescaled(prob, chunk=160):
    """online softmax over chunks of `chunk` keys whose denominator stays where it was when the maximum moves"""
    s, v = _scores(prob), prob["v"].double()
    m = torch.full(s.shape[:-1] + (1,), float("-inf"), dtype=torch.float64)
    den = torch.zeros_like(m)
    o = torch.zeros(s.shape[:-1] + (v.shape[-1],), dtype=torch.float64)
    for c0 in range(0, s.shape[-1], chunk):
        sc = s[..., c0:c0 + chunk]
        mn = torch.maximum(m, sc.max(-1, keepdim=True).values)
        p = torch.exp(sc - mn)
        den = den + p.sum(-1, keepdim=True)                         # the defect: den * exp(m - mn) is what an online softmax needs
        o = o * torch.exp(m - mn) + _bf16_rn(p) @ v[..., c0:c0 + chunk, :]
        m = mn
    return _rows(_bf16_rn(o / den))


def _fp32_reversed(prob):
    """torch float32 with the keys in reverse order: another summation order of the same formula"""
    mask = prob["mask"].expand(1, 1, prob["q"].shape[2], prob["k"].shape[2]).flip(-1)
    return _rows(_attn(prob["q"], prob["k"].flip(-2), prob["v"].flip(-2), mask, prob["scale"], torch.float32)).float()


def _bf16_case(N, cls):
    case = V._case(N, HD, cls, BF16, False)
    return case[0], case[1], case[2]


def _passes(out, cls, dtype, prob, ref, pa=None):
    f = _figures("vit_mfma7", cls, dtype, out.float(), prob, ref=ref, p_abs=pa)
    return f["worst"] <= f["bar"], f


@pytest.mark.parametrize("N", [33, 197, 577])
def test_ideal_emulations_pass_every_class(N):
    for cls in CLASSES:
        prob, ref, pa = _bf16_case(N, cls)
        ok, f = _passes(_emulate(prob), cls, BF16, prob, ref, pa)
        assert ok, ("bf16 MFMA", N, cls, f["worst"], f["bar"])
        assert f["worst"] <= 0.0, ("the two stated roundings alone stay below the margin", N, cls, f["worst"])
        p32, r32, _ = V._case(N, HD, cls, F32, False)
        ok, f = _passes(_fp32_reversed(p32), cls, F32, p32, r32)
        assert ok, ("fp32, keys reversed", N, cls, f["worst"], f["bar"])


def _failing_classes(N, defect):
    failed = []
    for cls in CLASSES:
        prob, ref, pa = _bf16_case(N, cls)
        if not _passes(defect(prob), cls, BF16, prob, ref, pa)[0]:
            failed.append(cls)
    return failed


def _hide_key(prob, j):
    hide = torch.zeros(1, 1, 1, prob["k"].shape[2], dtype=torch.bool)
    hide[..., j] = True
    return hide


DEFECTS = {
    "key N - 1 is dropped": lambda prob: _emulate(prob, hide=_hide_key(prob, -1)),
    "a padding key counts as a copy of key N - 1": lambda prob: _emulate(prob, pad_copy=True),
    "the denominator misses key N - 1": lambda prob: _emulate(prob, den_miss=prob["k"].shape[2] - 1),
    "a chunk's denominator is not rescaled": _emulate_chunks_not_rescaled,
}


@pytest.mark.parametrize("N", DEFECT_N)
@pytest.mark.parametrize("defect", list(DEFECTS))
def test_defect_fails_a_class(defect, N):
    failed = _failing_classes(N, DEFECTS[defect])
    assert failed, (defect, N)


@pytest.mark.parametrize("N", DEFECT_N)
def test_dropping_the_peaked_key_fails_at_every_peak_position(N):
    prob, ref, pa = _bf16_case(N, "peaked")
    peaks = V._peaks(N)
    B = prob["k"].shape[0]
    hide = torch.zeros(B, H, 1, N, dtype=torch.bool)
    for s in range(B * H):
        hide[s // H, s % H, 0, peaks[s % len(peaks)]] = True
    out = _emulate(prob, hide=hide)
    f = _figures("vit_mfma7", "peaked", BF16, out.float(), prob, ref=ref, p_abs=pa)
    left = (out - f["ref"]).abs() - 2.0 ** -8 * f["ref"].abs() - 2.0 ** -8 * pa              # [B, N, H * hd]
    per_slot = left.view(B, N, H, HD).amax(dim=(1, 3))                                      # [B, H]
    assert (per_slot > f["bar"]).all(), [peaks[s % len(peaks)] for s in range(B * H) if per_slot[s // H, s % H] <= f["bar"]]


@pytest.mark.parametrize("N", [33, 197, 257, 577])
def test_truncated_p_fails_the_bias_check_and_rounded_p_passes(N):
    prob, ref, pa = _bf16_case(N, "positive")
    for p_round, biased in ((_bf16_rn, False), (_bf16_rz, True)):
        f = _figures("vit_mfma7", "positive", BF16, _emulate(prob, p_round=p_round).float(), prob, ref=ref, p_abs=pa)
        mean, limit = _bias(f, BF16, mfma=True)
        assert (abs(mean) > limit) == biased, (N, "truncated" if biased else "to nearest", mean, limit)
        if biased:
            assert mean < 0


def _peaked_cases():
    cases = set()
    for row in V.ROWS.values():
        for hd in row["hds"]:
            for N in row["Ns"]:
                for impl in row["impls"]:
                    for dtype in row["dtypes"]:
                        cases.add((N, hd, V._rounding(row, dtype), bool(impl & 8) and bool(row.get("hd_entry")), dtype, 0))
    cases.update((N, 64, G8IN, False, SPLIT, V.PW_B) for N in V.PW_N)
    return sorted(c for c in cases if c[0] > 1)          # a one-key row has no other key to fall back on


PEAKED = _peaked_cases()


@pytest.mark.parametrize("N,hd,rounding,causal,dtype,B", PEAKED)
def test_leading_key_decides_every_row_of_its_slot(N, hd, rounding, causal, dtype, B):
    prob, ref, _ = V._case(N, hd, "peaked", rounding, causal, B or None)
    bar = _figures("vit_mfma7", "peaked", dtype, ref[0].float(), prob, ref=ref)["bar"]
    peaks = V._peaks(N)
    B = prob["k"].shape[0]
    lead = torch.tensor([peaks[s % len(peaks)] for s in range(B * H)]).view(B, H, 1, 1)
    j = torch.arange(N).view(1, 1, 1, N)
    mask = prob["mask"] & (j != lead)                                                       # [B, H, N or 1, N]
    visible = (prob["mask"] & (j == lead)).expand(B, H, N, N).any(-1) & mask.expand(B, H, N, N).any(-1)      # [B, H, N]
    mask = mask | ~mask.expand(B, H, N, N).any(-1, keepdim=True)                            # (a row left without a key is not judged)
    without = _attn(prob["q"], prob["k"], prob["v"], mask, prob["scale"], torch.float64)
    moved = (without - ref[0].view(B, N, H, hd).permute(0, 2, 1, 3)).abs().amax(-1)          # [B, H, N]
    assert visible.any()
    assert (moved[visible] > 100.0 * bar).all(), (moved[visible].min().item(), bar)
