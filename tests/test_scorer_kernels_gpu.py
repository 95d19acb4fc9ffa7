"""GPU: the kernels of the CLIP and BLIP-2 scorers that run outside the towers (csrc/clip.hip, csrc/blip2_itm.hip), one launch at a
time: the two text embeddings, the CLIP pooled head, the ITC and ITM heads (through their cap_op_* hooks) and the two score kernels
(cap_clip_logits, cap_blip2_itc_scores).  The HF goldens of test_clip_gpu.py / test_blip2_itm_gpu.py reach them at two or three
widths that are multiples of 64, with a whole tower's tolerance and well-formed ids and lengths; here every stride, tail and
idle-wave path runs alone: widths of 1, 63 .. 65, 255 / 257, 1000 and the limit 1024, projections with fewer outputs than waves,
row counts that leave a block of four waves partial, lens and ids outside their range.

Every output lives in a buffer of sentinels (test_elementwise_kernels_gpu.py's Buf: guards on both sides) that is one row longer than
the kernel owns, and the WHOLE buffer is compared; rows of the input the kernel must not read hold NaN; every input is compared
with its host copy after the call.  Expectations and bounds come from tests/_scorer_ref.py: float64, with error bounds derived there
from the kernels' summation order (tests/test_scorer_ref_cpu.py holds a sequential fp32 implementation to them), bit patterns where
the kernel adds once (clip_embed_text) or runs the project's one LayerNorm (itm_embed_text against cap_op_layernorm).  No tolerance
here is tuned to the kernels; every rounding test prints its worst error / bound (MEASURE) before it asserts."""
import numpy as np
import pytest
import torch

import _elementwise_ref as E
import _scorer_ref as S
from test_elementwise_kernels_gpu import DTYPES, TAG, Buf, _dev, _layernorm, _ok, _p, _refused, _rows_then_sentinel, _same, _stream

pytestmark = pytest.mark.gpu

NAN32 = np.int32(E.NAN32)


@pytest.fixture(scope="module")
def lib():
    from embodied_captioning_amd import _native
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _native.load_library()


class Inputs:
    """host arrays on the device, kept alive for the launches and compared bit for bit with their host copies afterwards"""

    def __init__(self, **arrays):
        self.host = {k: np.ascontiguousarray(v) for k, v in arrays.items() if v is not None}
        self.dev = {k: _dev(v) for k, v in self.host.items()}

    def p(self, name, offset_bytes=0):
        return self.dev[name].data_ptr() + offset_bytes if name in self.dev else None

    def unchanged(self):
        torch.cuda.synchronize()
        for k, v in self.host.items():
            got = self.dev[k].cpu().numpy()
            assert got.tobytes() == v.tobytes(), f"the kernel changed its input {k}"


def _owned(buf, rows, what):
    """the first `rows` rows of a float32 Buf as float64, after checking that every later row still holds the sentinel"""
    bits = buf.bits()
    assert (bits[rows:] == NAN32).all(), f"{what}: written past row {rows}"
    assert (bits[:rows] != NAN32).all(), f"{what}: an owned element was not written"
    return buf.values()[:rows]


def _within(got, ref, bound, what):
    S.within(got, ref, bound, what, label="MEASURE")


# ---- clip_head -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.CLIP_HEAD_CASES, ids=str)
def test_clip_head(lib, case):
    a = S.clip_head_inputs(case)
    B, D, P, rp = a["B"], a["D"], a["P"], a["rows_per"]
    i = Inputs(x=a["x"], lens=a["lens"], gamma=a["gamma"], beta=a["beta"], W=a["W"])

    def call(out, b0, n):
        return lib.cap_op_clip_head(i.p("x", b0 * rp * D * 4), rp, i.p("lens", b0 * 4), i.p("gamma"), i.p("beta"), S.EPS, i.p("W"), out.ptr, n,
                                    D, P, _stream())

    out = Buf("f32", B + 1, P)
    _ok(lib, call(out, 0, B))
    ref, bound = S.clip_head64(a["x"], rp, a["lens"], a["gamma"], a["beta"], S.EPS, a["W"])
    _within(_owned(out, B, f"clip_head {case}"), ref, bound, f"clip_head {case}")
    for b in range(B):                                            # a row alone has the bits it has in the batch
        one = Buf("f32", 2, P)
        _ok(lib, call(one, b, 1))
        _same(one, np.concatenate([out.bits()[b:b + 1], out.bits()[B:]]), f"clip_head {case} row {b} alone")
    i.unchanged()


# ---- itc_head ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.ITC_HEAD_CASES, ids=str)
def test_itc_head(lib, case):
    a = S.itc_head_inputs(case)
    n, D, P, rp = a["n"], a["D"], a["P"], a["rows_per"]
    i = Inputs(x=a["x"], W=a["W"], bias=a["bias"])

    def call(out, r0, rows):
        return lib.cap_op_itc_head(i.p("x", r0 * rp * D * 4), rp, i.p("W"), i.p("bias"), out.ptr, rows, D, P, _stream())

    out = Buf("f32", n + 1, P)
    _ok(lib, call(out, 0, n))
    ref, bound = S.itc_head64(a["x"], rp, a["W"], a["bias"])
    got = _owned(out, n, f"itc_head {case}")
    _within(got, ref, bound, f"itc_head {case}")
    if case[4] == "zero":
        assert not got[3].any(), "an all-zero row with a zero bias gives zeros (F.normalize's eps)"
    for r in range(n):
        one = Buf("f32", 2, P)
        _ok(lib, call(one, r, 1))
        _same(one, np.concatenate([out.bits()[r:r + 1], out.bits()[n:]]), f"itc_head {case} row {r} alone")
    i.unchanged()


# ---- clip_embed_text -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.CLIP_EMBED_CASES, ids=str)
def test_clip_embed_text(lib, case):
    a = S.embed_inputs(case, 3)
    M, D, L = a["M"], a["D"], a["L"]
    i = Inputs(ids=a["ids"], tok=a["table"], pos=a["pos"])
    x = Buf("f32", M + 1, D)
    _ok(lib, lib.cap_op_clip_embed_text(i.p("ids"), L, i.p("tok"), i.p("pos"), x.ptr, M, D, S.EMBED_V, _stream()))
    want = E.encode("f32", S.embed_rows32(a["ids"], L, a["table"], a["pos"]))
    _same(x, _rows_then_sentinel("f32", want, M + 1), f"clip_embed_text {case} vs the host's fp32 sum")
    i.unchanged()


# ---- itm_embed_text ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.ITM_EMBED_CASES, ids=str)
@pytest.mark.parametrize("dt", DTYPES)
def test_itm_embed_text(lib, dt, case):
    kind = E.KIND[dt]
    a = S.embed_inputs(case, 7)
    M, D, L = a["M"], a["D"], a["L"]
    i = Inputs(ids=a["ids"], word=a["table"], pos=a["pos"], gamma=a["gamma"], beta=a["beta"])
    x_f, x_t = Buf("f32", M + 1, D), Buf(kind, M + 1, D)
    _ok(lib, lib.cap_op_itm_embed_text(TAG[dt], i.p("ids"), L, i.p("word"), i.p("pos"), i.p("gamma"), i.p("beta"), S.ITM_EPS, x_f.ptr, x_t.ptr,
                                       M, D, S.EMBED_V, _stream()))
    what = f"itm_embed_text {dt} {case}"
    y32 = S.embed_rows32(a["ids"], L, a["table"], a["pos"])
    ref_t, ref_f = _layernorm(lib, dt, y32, i.dev["gamma"], i.dev["beta"], S.ITM_EPS)
    _same(x_f, _rows_then_sentinel("f32", ref_f, M + 1), what + " x_f vs cap_op_layernorm of the host's fp32 sum")
    _same(x_t, _rows_then_sentinel(kind, ref_t, M + 1), what + " x_t vs cap_op_layernorm")
    got_f = x_f.values()[:M]
    _same(x_t, _rows_then_sentinel(kind, E.encode(kind, got_f.astype(np.float32)), M + 1), what + " x_t is x_f stored in the operand type")
    ref, bound = S.itm_embed_text64(a["ids"], L, a["table"], a["pos"], a["gamma"], a["beta"], S.ITM_EPS)
    _within(got_f, ref, bound, what + " x_f")
    _within(x_t.values()[:M], ref, bound + E.store_error(kind, np.abs(ref) + bound), what + " x_t")
    i.unchanged()


# ---- clip_logits ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.CLIP_LOGITS_CASES, ids=str)
def test_clip_logits(lib, case):
    a = S.clip_logits_inputs(case)
    Ni, Nt, P = a["Ni"], a["Nt"], a["P"]
    i = Inputs(img=a["img"], txt=a["txt"])

    def call(out, paired):
        return lib.cap_clip_logits(i.p("img"), i.p("txt"), Ni, Nt, paired, a["scale"], out.ptr, P, _stream())

    out = Buf("f32", Ni * Nt + 3)
    _ok(lib, call(out, 0))
    ref, bound = S.clip_logits64(a["img"], a["txt"], a["scale"], False)
    _within(_owned(out, Ni * Nt, f"clip_logits {case}").reshape(Ni, Nt), ref, bound, f"clip_logits {case}")
    if Ni == Nt:                                                  # paired[i] has the bits of matrix[i, i]
        pair = Buf("f32", Ni + 3)
        _ok(lib, call(pair, 1))
        diag = np.diagonal(out.bits()[:Ni * Nt].reshape(Ni, Nt))
        _same(pair, np.concatenate([diag, np.full(3, NAN32)]), f"clip_logits {case} paired vs the matrix's diagonal")
    i.unchanged()


# ---- itc_scores ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.ITC_SCORES_CASES, ids=str)
def test_itc_scores(lib, case):
    a = S.itc_scores_inputs(case)
    Ni, Nt, P, nq = a["Ni"], a["Nt"], a["P"], a["nq"]
    i = Inputs(img=a["img"], txt=a["txt"])

    def call(out, paired):
        return lib.cap_blip2_itc_scores(i.p("img"), i.p("txt"), Ni, Nt, paired, out.ptr, nq, P, _stream())

    out = Buf("f32", Ni * Nt + 3)
    _ok(lib, call(out, 0))
    ref, bound, at = S.itc_scores64(a["img"], a["txt"], False)
    assert (at == a["q_star"]).all() and (np.sign(ref) == a["sign"]).all()
    got = _owned(out, Ni * Nt, f"itc_scores {case}").reshape(Ni, Nt)
    _within(got, ref, bound, f"itc_scores {case}")
    assert (np.sign(got) == a["sign"]).all()
    if Ni == Nt:
        pair = Buf("f32", Ni + 3)
        _ok(lib, call(pair, 1))
        diag = np.diagonal(out.bits()[:Ni * Nt].reshape(Ni, Nt))
        _same(pair, np.concatenate([diag, np.full(3, NAN32)]), f"itc_scores {case} paired vs the matrix's diagonal")
    i.unchanged()


# ---- itm_head ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.ITM_HEAD_CASES, ids=str)
def test_itm_head(lib, case):
    a = S.itm_head_inputs(case)
    B, nq, D = a["B"], a["nq"], a["D"]
    i = Inputs(x=a["x"], W=a["W"], bias=a["bias"])

    def call(logits, prob, b0, n):
        return lib.cap_op_itm_head(i.p("x", b0 * nq * D * 4), i.p("W"), i.p("bias"), logits.ptr, prob.ptr if prob else None, n, nq, D, _stream())

    logits, prob = Buf("f32", B + 1, 2), Buf("f32", B + 1)
    _ok(lib, call(logits, prob, 0, B))
    ref_l, e_l, ref_p, e_p = S.itm_head64(a["x"], a["W"], a["bias"])
    _within(_owned(logits, B, f"itm_head {case} logits"), ref_l, e_l, f"itm_head {case} logits")
    got_p = _owned(prob, B, f"itm_head {case} prob")
    _within(got_p, ref_p, e_p, f"itm_head {case} prob")
    if case[3] != "random":                                       # l1 - l0 = +-200: exactly 1 or 0, and finite
        assert np.array_equal(got_p, np.full(B, 1.0 if case[3] == "+200" else 0.0)), got_p.tolist()
    alone = Buf("f32", B + 1, 2)                                  # without prob: the same logits
    _ok(lib, call(alone, None, 0, B))
    _same(alone, logits.bits(), f"itm_head {case} logits without prob")
    for b in range(B):                                            # a pair alone has the bits it has in the batch
        l1, p1 = Buf("f32", 2, 2), Buf("f32", 2)
        _ok(lib, call(l1, p1, b, 1))
        _same(l1, np.concatenate([logits.bits()[b:b + 1], logits.bits()[B:]]), f"itm_head {case} pair {b} alone: logits")
        _same(p1, np.concatenate([prob.bits()[b:b + 1], prob.bits()[B:]]), f"itm_head {case} pair {b} alone: prob")
    i.unchanged()


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_heads_refuse_widths_beyond_their_shared_memory_and_empty_rows(lib):
    z = torch.zeros(2 * 1025, device="cuda")
    lens = torch.ones(2, dtype=torch.int32, device="cuda")
    out = Buf("f32", 2, 1025)
    for D, P, rp in ((1025, 8, 1), (8, 1025, 1), (8, 8, 0)):
        needles = ("no rows",) if rp == 0 else (f"width {D} / projection {P}", "1024 / 1024")
        rc = lib.cap_op_clip_head(_p(z), rp, _p(lens), _p(z), _p(z), S.EPS, _p(z), out.ptr, 2, D, P, _stream())
        _refused(lib, rc, "clip_head:", *needles)
        rc = lib.cap_op_itc_head(_p(z), rp, _p(z), _p(z), out.ptr, 2, D, P, _stream())
        _refused(lib, rc, "itc_head:", *needles)
    assert out.untouched()


@pytest.mark.parametrize("dt", DTYPES)
def test_itm_embed_text_refuses_rows_that_are_no_whole_groups_of_8_or_too_wide(lib, dt):
    kind = E.KIND[dt]
    z = torch.zeros(4 * 1032, device="cuda")
    ids = torch.zeros(4, dtype=torch.int32, device="cuda")
    x_f, x_t = Buf("f32", 4, 1032), Buf(kind, 4, 1032)
    for D, L in ((12, 2), (1032, 2), (8, 0)):
        rc = lib.cap_op_itm_embed_text(TAG[dt], _p(ids), L, _p(z), _p(z), _p(z), _p(z), S.ITM_EPS, x_f.ptr, x_t.ptr, 4, D, 4, _stream())
        _refused(lib, rc, "itm_embed_text: bad shape", f"L={L}", f"D={D}", "a multiple of 8 up to 1024")
    assert x_f.untouched() and x_t.untouched()


def test_embeddings_and_scores_refuse_bad_counts(lib):
    z = torch.zeros(64, device="cuda")
    ids = torch.zeros(4, dtype=torch.int32, device="cuda")
    out = Buf("f32", 16)
    _refused(lib, lib.cap_op_clip_embed_text(_p(ids), 0, _p(z), _p(z), out.ptr, 4, 2, 4, _stream()), "clip_embed_text: bad shape", "L=0")
    _refused(lib, lib.cap_op_clip_embed_text(_p(ids), 2, _p(z), _p(z), out.ptr, 4, 2, 0, _stream()), "clip_embed_text: bad shape", "V=0")
    _refused(lib, lib.cap_clip_logits(_p(z), _p(z), 2, 3, 1, 0.0, out.ptr, 4, _stream()), "cap_clip_logits: bad shape Ni=2 Nt=3", "paired needs Ni == Nt")
    _refused(lib, lib.cap_blip2_itc_scores(_p(z), _p(z), 2, 3, 1, out.ptr, 2, 4, _stream()), "cap_blip2_itc_scores: bad shape Ni=2 Nt=3",
             "paired needs Ni == Nt")
    _refused(lib, lib.cap_blip2_itc_scores(_p(z), _p(z), 2, 2, 0, out.ptr, 0, 4, _stream()), "cap_blip2_itc_scores: bad shape", "queries=0")
    _refused(lib, lib.cap_op_itm_head(_p(z), _p(z), _p(z), out.ptr, out.ptr + 32, 2, 0, 4, _stream()), "itm_head: bad shape B=2 queries=0 D=4")
    _refused(lib, lib.cap_op_itm_head(_p(z), _p(z), _p(z), out.ptr, None, 0, 2, 4, _stream()), "itm_head: bad shape B=0")
    assert out.untouched()


def test_the_hooks_refuse_null_pointers_by_name(lib):
    z = torch.zeros(64, device="cuda")
    ids = torch.zeros(4, dtype=torch.int32, device="cuda")
    out = Buf("f32", 64)
    zp, ip, op, s = _p(z), _p(ids), out.ptr, _stream()

    def each_null(name, args, required):
        """the call with one required pointer (positions `required`) at a time replaced by NULL"""
        fn = getattr(lib, name)
        for k in required:
            _refused(lib, fn(*args[:k], None, *args[k + 1:]), f"{name}: null pointer")

    each_null("cap_op_clip_embed_text", (ip, 2, zp, zp, op, 4, 2, 4, s), (0, 2, 3, 4))
    each_null("cap_op_clip_head", (zp, 1, ip, zp, zp, S.EPS, zp, op, 2, 4, 4, s), (0, 3, 4, 6, 7))          # 2: lens may be NULL
    for dt in DTYPES:
        each_null("cap_op_itm_embed_text", (TAG[dt], ip, 2, zp, zp, zp, zp, S.ITM_EPS, op, op + 128, 4, 8, 4, s), (1, 3, 4, 5, 6, 8, 9))
    each_null("cap_op_itc_head", (zp, 1, zp, zp, op, 2, 4, 4, s), (0, 2, 3, 4))
    each_null("cap_op_itm_head", (zp, zp, zp, op, op + 32, 2, 2, 4, s), (0, 1, 2, 3))                          # 4: prob may be NULL
    assert out.untouched()
