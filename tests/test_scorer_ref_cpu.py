"""CPU: the float64 references of tests/_scorer_ref.py (the CLIP / BLIP-2 scorer embedding, head and score kernels).

Two things are pinned where there is no GPU.  The references compute what the library functions they restate compute
(F.layer_norm, F.linear, F.normalize, x / x.norm, torch.softmax, HF's exp(s) * img @ txt.T, max over the query axis).  And the
derived error bounds are not too tight: on every case of the GPU file's lists, a straightforward fp32 numpy implementation that sums
SEQUENTIALLY (np.cumsum: another order than the kernels' lane chains and trees, and up to 1024 roundings on a term instead of 23)
stays inside them - so no bound was made to fit the code under test."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _scorer_ref as S

f32 = np.float32


def _t(a):
    return torch.from_numpy(np.asarray(a)).double()


def _close(got, want, tol=1e-12):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= tol * max(1.0, np.abs(want).max())


def seq_sum32(a):
    """the last axis summed left to right in fp32"""
    return np.cumsum(np.asarray(a, dtype=f32), axis=-1, dtype=f32)[..., -1]


def seq_matmul32(x, W):
    """x [n, D] . W [P, D]^T: fp32 products, then the sequential sum"""
    return seq_sum32(x[:, None, :].astype(f32) * W[None, :, :].astype(f32))


_inside = S.within


# ---- the references against the library functions -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.CLIP_HEAD_CASES)
def test_clip_head64_is_layer_norm_linear_and_the_plain_norm(case):
    a = S.clip_head_inputs(case)
    rows = S.head_rows(a["B"], a["rows_per"], a["lens"])
    if a["lens"] is not None and a["B"] == 5:                     # 0 and 1 -> the first row, rows_per and rows_per + 3 -> the last
        rp = a["rows_per"]
        assert rows.tolist() == [0, rp, 2 * rp + rp - 1, 3 * rp + rp - 1, 4 * rp + (rp + 1) // 2 - 1]
    x = _t(a["x"])[torch.from_numpy(rows)]
    assert not torch.isnan(x).any() and int(np.isnan(a["x"]).all(-1).sum()) == a["x"].shape[0] - a["B"]
    y = F.linear(F.layer_norm(x, (a["D"],), _t(a["gamma"]), _t(a["beta"]), S.EPS), _t(a["W"]))
    ref, bound = S.clip_head64(a["x"], a["rows_per"], a["lens"], a["gamma"], a["beta"], S.EPS, a["W"])
    _close(ref, (y / y.norm(dim=-1, keepdim=True)).numpy(), 1e-10)
    assert bound.max() < 1e-2 and (bound > 0).all()


@pytest.mark.parametrize("case", S.ITC_HEAD_CASES)
def test_itc_head64_is_linear_and_F_normalize(case):
    a = S.itc_head_inputs(case)
    x = _t(a["x"])[::a["rows_per"]]
    ref, bound = S.itc_head64(a["x"], a["rows_per"], a["W"], a["bias"])
    _close(ref, F.normalize(F.linear(x, _t(a["W"]), _t(a["bias"])), dim=-1).numpy(), 1e-10)
    if case[4] == "zero":
        assert not ref[3].any() and not bound[3].any() and np.isfinite(ref).all()
    assert bound.max() < 1e-3


@pytest.mark.parametrize("case", S.CLIP_EMBED_CASES)
def test_clip_embed_text64_is_an_embedding_lookup_plus_positions(case):
    a = S.embed_inputs(case, 3)
    ids = torch.from_numpy(a["ids"]).long().clamp(0, S.EMBED_V - 1)
    for must in (-3, 0, S.EMBED_V - 1, S.EMBED_V + 5):
        assert must in a["ids"]
    assert a["M"] % 4 != 0
    want = F.embedding(ids, torch.from_numpy(a["table"])) + torch.from_numpy(a["pos"])[torch.arange(a["M"]) % a["L"]]
    ref, bound = S.clip_embed_text64(a["ids"], a["L"], a["table"], a["pos"])
    assert np.array_equal(ref.astype(f32).view(np.int32), want.numpy().view(np.int32)) and not bound.any()


@pytest.mark.parametrize("case", S.ITM_EMBED_CASES)
def test_itm_embed_text64_is_F_layer_norm_of_the_fp32_sum(case):
    a = S.embed_inputs(case, 7)
    assert a["M"] % 4 != 0 and a["D"] % 8 == 0
    y = torch.from_numpy(S.embed_rows32(a["ids"], a["L"], a["table"], a["pos"])).double()
    ref, bound = S.itm_embed_text64(a["ids"], a["L"], a["table"], a["pos"], a["gamma"], a["beta"], S.ITM_EPS)
    _close(ref, F.layer_norm(y, (a["D"],), _t(a["gamma"]), _t(a["beta"]), S.ITM_EPS).numpy(), 1e-10)
    assert (bound == S.TOL_LN_F32).all()


def test_the_layernorm_bound_is_the_one_the_elementwise_tests_use():
    import test_elementwise_kernels_gpu as G
    assert S.TOL_LN_F32 == G.TOL_LN_F32


@pytest.mark.parametrize("case", S.CLIP_LOGITS_CASES)
def test_clip_logits64_is_hf_logits_per_image(case):
    a = S.clip_logits_inputs(case)
    want = (torch.exp(torch.tensor(a["scale"], dtype=torch.float64)) * _t(a["img"]) @ _t(a["txt"]).T).numpy()
    ref, _ = S.clip_logits64(a["img"], a["txt"], a["scale"], False)
    _close(ref, want)
    if a["Ni"] == a["Nt"]:
        pr, pb = S.clip_logits64(a["img"], a["txt"], a["scale"], True)
        _close(pr, np.diagonal(want))
        assert pr.shape == pb.shape == (a["Ni"],)


@pytest.mark.parametrize("case", S.ITC_SCORES_CASES)
def test_itc_scores64_is_the_max_over_the_query_axis(case):
    a = S.itc_scores_inputs(case)
    sim = torch.einsum("iqp,jp->ijq", _t(a["img"]), _t(a["txt"]))
    ref, bound, at = S.itc_scores64(a["img"], a["txt"], False)
    _close(ref, sim.max(-1).values.numpy())
    assert (at == a["q_star"]).all(), "the maximum stands at the planted row"
    assert (np.sign(ref) == a["sign"]).all(), "every score has the case's sign"
    if a["sign"] < 0:
        assert (ref + bound < 0).all()                            # a maximum that starts from 0 gives 0: outside the bound
    if a["Ni"] == a["Nt"]:
        pr, _, pat = S.itc_scores64(a["img"], a["txt"], True)
        _close(pr, np.diagonal(ref))
        assert (pat == a["q_star"]).all()


@pytest.mark.parametrize("case", S.ITM_HEAD_CASES)
def test_itm_head64_is_the_mean_of_a_linear_head_and_softmax(case):
    a = S.itm_head_inputs(case)
    per = F.linear(_t(a["x"]), _t(a["W"]), _t(a["bias"]))        # [B, nq, 2]
    want = per.mean(1)
    logits, e_l, prob, e_p = S.itm_head64(a["x"], a["W"], a["bias"])
    _close(logits, want.numpy())
    _close(prob, torch.softmax(want, dim=-1)[:, 1].numpy(), 1e-15)
    assert e_l.shape == (a["B"], 2) and e_p.shape == (a["B"],) and e_p.max() < 1e-4
    if case[3] == "+200":
        assert (prob == 1.0).all() and (logits[:, 1] - logits[:, 0] > 190).all()
    if case[3] == "-200":
        assert (prob < 1e-80).all() and (e_p < 2 ** -125).all()


# ---- the bounds against a sequential fp32 implementation -----------------------------------------------------------------------
def _normalise32(y, floor):
    nrm = np.maximum(np.sqrt(seq_sum32(y * y)), f32(floor))[:, None]
    return (y / nrm).astype(f32)


def test_clip_head_bound_holds_a_sequential_fp32_head():
    worst = 0.0
    for case in S.CLIP_HEAD_CASES:
        a = S.clip_head_inputs(case)
        D = f32(a["D"])
        x = a["x"][S.head_rows(a["B"], a["rows_per"], a["lens"])]
        mean = (seq_sum32(x) / D)[:, None]
        c = (x - mean).astype(f32)
        rstd = (f32(1) / np.sqrt(seq_sum32(c * c) / D + f32(S.EPS)))[:, None].astype(f32)
        ln = (c * rstd * a["gamma"] + a["beta"]).astype(f32)
        got = _normalise32(seq_matmul32(ln, a["W"]), 0.0)
        ref, bound = S.clip_head64(a["x"], a["rows_per"], a["lens"], a["gamma"], a["beta"], S.EPS, a["W"])
        worst = max(worst, _inside(got, ref, bound, f"clip_head {case}"))
    print(f"clip_head: sequential fp32 worst error / bound {worst:.3f}")


def test_itc_head_bound_holds_a_sequential_fp32_head():
    worst = 0.0
    for case in S.ITC_HEAD_CASES:
        a = S.itc_head_inputs(case)
        y = (seq_matmul32(a["x"][::a["rows_per"]], a["W"]) + a["bias"]).astype(f32)
        ref, bound = S.itc_head64(a["x"], a["rows_per"], a["W"], a["bias"])
        worst = max(worst, _inside(_normalise32(y, 1e-12), ref, bound, f"itc_head {case}"))
    print(f"itc_head: sequential fp32 worst error / bound {worst:.3f}")


def test_clip_logits_bound_holds_a_sequential_fp32_product():
    worst = 0.0
    for case in S.CLIP_LOGITS_CASES:
        a = S.clip_logits_inputs(case)
        got = (np.exp(f32(a["scale"])) * seq_matmul32(a["img"], a["txt"])).astype(f32)
        ref, bound = S.clip_logits64(a["img"], a["txt"], a["scale"], False)
        worst = max(worst, _inside(got, ref, bound, f"clip_logits {case}"))
        if a["Ni"] == a["Nt"]:
            ref, bound = S.clip_logits64(a["img"], a["txt"], a["scale"], True)
            _inside(np.diagonal(got), ref, bound, f"clip_logits paired {case}")
    print(f"clip_logits: sequential fp32 worst error / bound {worst:.3f}")


def test_itc_scores_bound_holds_a_sequential_fp32_product():
    worst = 0.0
    for case in S.ITC_SCORES_CASES:
        a = S.itc_scores_inputs(case)
        img = a["img"].reshape(a["Ni"] * a["nq"], a["P"])
        got = seq_matmul32(img, a["txt"]).reshape(a["Ni"], a["nq"], a["Nt"]).max(1)
        ref, bound, _ = S.itc_scores64(a["img"], a["txt"], False)
        worst = max(worst, _inside(got, ref, bound, f"itc_scores {case}"))
    print(f"itc_scores: sequential fp32 worst error / bound {worst:.3f}")


def test_itm_head_bound_holds_a_sequential_fp32_head():
    worst_l = worst_p = 0.0
    for case in S.ITM_HEAD_CASES:
        a = S.itm_head_inputs(case)
        B, nq, D = a["B"], a["nq"], a["D"]
        per = (seq_matmul32(a["x"].reshape(B * nq, D), a["W"]) + a["bias"]).astype(f32).reshape(B, nq, 2)
        logits = (seq_sum32(per.transpose(0, 2, 1)) / f32(nq)).astype(f32)
        e = np.exp(logits - logits.max(-1, keepdims=True)).astype(f32)
        prob = (e[:, 1] / (e[:, 0] + e[:, 1])).astype(f32)
        ref_l, e_l, ref_p, e_p = S.itm_head64(a["x"], a["W"], a["bias"])
        worst_l = max(worst_l, _inside(logits, ref_l, e_l, f"itm_head logits {case}"))
        worst_p = max(worst_p, _inside(prob, ref_p, e_p, f"itm_head prob {case}"))
        if case[3] != "random":
            assert np.array_equal(prob, np.full(B, 1.0 if case[3] == "+200" else 0.0, dtype=f32))
    print(f"itm_head: sequential fp32 worst error / bound: logits {worst_l:.3f}, prob {worst_p:.3f}")


def test_itm_embed_text_bound_holds_a_sequential_fp32_layernorm():
    for case in S.ITM_EMBED_CASES:
        a = S.embed_inputs(case, 7)
        y = S.embed_rows32(a["ids"], a["L"], a["table"], a["pos"])
        D = f32(a["D"])
        c = (y - (seq_sum32(y) / D)[:, None]).astype(f32)
        rstd = (f32(1) / np.sqrt(seq_sum32(c * c) / D + f32(S.ITM_EPS)))[:, None].astype(f32)
        ref, bound = S.itm_embed_text64(a["ids"], a["L"], a["table"], a["pos"], a["gamma"], a["beta"], S.ITM_EPS)
        _inside((c * rstd * a["gamma"] + a["beta"]).astype(f32), ref, bound, f"itm_embed_text {case}")


def test_the_case_lists_hold_the_shapes_the_kernels_branch_on():
    assert {c[0] for c in S.CLIP_HEAD_CASES} == {c[0] for c in S.ITC_HEAD_CASES} == {1, 63, 64, 65, 255, 257, 768, 1000, 1024}
    assert {c[1] for c in S.CLIP_HEAD_CASES} == {c[1] for c in S.ITC_HEAD_CASES} == {1, 3, 5, 255, 257, 512, 1024}
    assert {c[2] for c in S.CLIP_HEAD_CASES} == {1, 5} and {c[3] for c in S.CLIP_HEAD_CASES} == {1, 7}
    assert {c[5] for c in S.CLIP_HEAD_CASES} == set(S.FAMILIES) and {c[3] for c in S.ITC_HEAD_CASES} == {1, 6}
    assert {c[0] for c in S.CLIP_EMBED_CASES} == {1, 63, 65, 512, 1000} and {c[1] for c in S.CLIP_EMBED_CASES} == {1, 5, 77}
    assert {c[2] % 4 for c in S.CLIP_EMBED_CASES} == {1, 2, 3}
    assert {c[0] for c in S.ITM_EMBED_CASES} == {8, 248, 256, 264, 768, 1016, 1024} and {c[1] for c in S.ITM_EMBED_CASES} == {1, 5, 32}
    for cases in (S.CLIP_LOGITS_CASES, S.ITC_SCORES_CASES):
        assert {c[:2] for c in cases} == {(1, 1), (3, 5), (2, 9), (7, 7)} and {c[2] for c in cases} == {1, 63, 65, 256, 1000}
        assert any(c[0] * c[1] % 4 for c in cases)
    assert {round(c[3], 4) for c in S.CLIP_LOGITS_CASES} == {0.0, 4.6052, -2.0}
    assert {c[3] for c in S.ITC_SCORES_CASES} == {1, 3, 32} and {c[4] for c in S.ITC_SCORES_CASES} == {"first", "middle", "last"}
    assert {c[0] for c in S.ITM_HEAD_CASES} == {1, 5} and {c[1] for c in S.ITM_HEAD_CASES} == {1, 3, 32}
    assert {c[2] for c in S.ITM_HEAD_CASES} == {1, 63, 65, 768, 1000}


def test_clip_head_bound_catches_a_one_pass_variance_on_the_offset_rows():
    """the other direction: E[x^2] - mean^2 in fp32 (numpy's pairwise sums, more accurate than a sequential one) cancels on a row
    whose mean is 50 times its spread, and the bound sees it at every offset case that has more than one output to normalise"""
    seen = 0
    for case in S.CLIP_HEAD_CASES:
        if case[5] != "offset" or case[1] == 1:
            continue
        a = S.clip_head_inputs(case)
        D = f32(a["D"])
        x = a["x"][S.head_rows(a["B"], a["rows_per"], a["lens"])]
        mean = (x.sum(-1, dtype=f32) / D)[:, None]
        var = ((x * x).sum(-1, dtype=f32) / D)[:, None] - mean * mean
        ln = ((x - mean) / np.sqrt(var + f32(S.EPS)) * a["gamma"] + a["beta"]).astype(f32)
        y = (ln.astype(np.float64) @ a["W"].astype(np.float64).T)        # everything after the variance exact
        got = y / np.sqrt((y * y).sum(-1, keepdims=True))
        ref, bound = S.clip_head64(a["x"], a["rows_per"], a["lens"], a["gamma"], a["beta"], S.EPS, a["W"])
        err = np.abs(got - ref)
        assert not (err <= bound).all(), f"{case}: a one-pass variance stays inside the bound (worst {np.nanmax(err / bound):.2f})"
        seen += 1
    assert seen == 3
