"""GPU: the attention kernels of the BLIP-2, Q-Former, CoCa-pooler, image-text-scorer and sentence-encoder paths, kernel by kernel,
against ONE float64 reference - softmax(scale q k^T + mask) v per (batch, head) - through the C ABI's single-kernel entry points.

Inputs are rounded to the kernel's input type BEFORE the reference sees them, so only the kernel's arithmetic is judged.  Three
input classes per case:

  randn   randn * 1.5, the project's standing choice;
  rising  every key's score exceeds the previous key's (by 3 units on short rows; the whole climb is held to 96 units on long ones,
          beyond which the fp32 reference's own score rounding - and with it the bar - grows past anything worth asserting), so every
          step of an online softmax rescales its state;
  peaked  one key leads the rest by ~20 units (20 (1 +- 0.5 / sqrt(head_dim)) over a case's queries).  One (batch, head) slot per peak position: the first key, the last key and both sides
          of every boundary the kernel has.  Dropping such a key changes the output by O(1).

Bars (derived, never taken from the kernel's output):
  fp32 out   8 x ref_err_fp32, ref_err_fp32 = max |the same formula in torch float32 on the CPU - float64|: the reference's own
             rounding, with the margin tests/test_blip2_itm_gpu.py gives another fp32 implementation with another summation order.
             Where that is 0 (a one-key row is exact in both) the smallest non-zero ref_err_fp32 of the family's randn cases stands in.
  bf16 out   elementwise |out - ref| <= 2^-8 |ref| + the fp32 bar (half a bf16 ulp of final rounding).
  G8 out     the fp32 bar + the container's own error for the case, max |g8_decode(g8_encode(ref32)) - ref32|.
The peaked class at 257 .. 1 025 keys is what found the lane = query kernels' denominator losing 2^-24 of the row per key (up to 6.4e-5;
softmax_denominator_add in csrc/attention.hip is the fix): every case is held to the bars above, none is raised.
The reference, the classes and the bars live in tests/_attention_ref.py, shared with tests/test_vit_attention_classes_gpu.py.
Run with -s for the table of maxima and bars (profiles/attention_kernels_gpu_tolerances.txt is that output)."""
import ctypes as C
import math

import pytest
import torch

from _attention_ref import BF16, F32, FAMILIES, SPLIT, _judge, _problem, _rounded, _rows, _sides, _slots
from _util import g8_decode

pytestmark = pytest.mark.gpu

DTYPES = [F32, BF16, SPLIT]
DT_NAME = {F32: "f32", BF16: "bf16", SPLIT: "f32s"}
CLASSES = ("randn", "rising", "peaked")
NAN = float("nan")
GUARD, CANARY = 256, 77.0            # canary bands of GUARD elements either side of every buffer a kernel writes

@pytest.fixture(scope="module")
def lib():
    from embodied_captioning_amd import _native
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _native.load_library()


def _p(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _check(lib, rc):
    assert rc == 0, lib.cap_last_error().decode()


def _refused(lib, rc, word):
    msg = lib.cap_last_error().decode()
    assert rc != 0 and word in msg, (rc, msg)


def _in_t(dtype):
    return torch.bfloat16 if dtype == BF16 else torch.float32


def _out_t(dtype):
    return torch.bfloat16 if dtype == BF16 else torch.float32      # a G8 container is float32-typed, one element per value


def _banded(values, tdtype):
    """values (CPU, any shape) -> (full, body): a device buffer with canary bands either side, body viewed in values' shape."""
    n = values.numel()
    full = torch.full((n + 2 * GUARD,), CANARY, dtype=tdtype, device="cuda")
    body = full[GUARD:GUARD + n].view(values.shape)
    body.copy_(values.to(tdtype))
    return full, body


def _bands_intact(full):
    return bool((full[:GUARD] == CANARY).all().item() and (full[-GUARD:] == CANARY).all().item())


def _nan_out(shape, dtype):
    return _banded(torch.full(shape, NAN), _out_t(dtype))


def _read(body, dtype):
    """Device output -> fp32 CPU values."""
    if dtype == SPLIT:
        return torch.from_numpy(g8_decode(body.cpu().numpy()))
    return body.float().cpu()


# ---------------------------------------------------------------------------------------------- OPT decode step
OPT_HD = [80, 64, 128, 40, 96]                 # HD8 = 10, 8, 16 and the runtime-width form (40, 96)
OPT_PAST = [0, 1, 3, 11, 12, 13, 15, 16, 52, 63, 64, 65, 127, 128, 500, 1023]
OPT_H = 2


def _opt_peaks(Lk):
    # j == past is the last key; lanes stride keys by 64; P.V runs in trips of 16 keys and a tail: every key of the last 20 covers it
    return sorted(set(_sides(range(64, Lk, 64), Lk)) | set(range(max(0, Lk - 20), Lk)))


def _opt_problem(case, cls, dtype):
    hd, past = case
    Lk = past + 1
    peaks = _opt_peaks(Lk)
    return _problem(cls, _slots(cls, peaks, OPT_H), OPT_H, 1, Lk, hd, 1000 * hd + past, peaks, dtype=dtype)


def _opt_buffers(prob, past, Lmax, dtype):
    """fused q|k|v rows of the new position, caches holding the positions below `past` and NaN from `past` on."""
    rq, rk, rv = _rows(prob["q"]), _rows(prob["k"]), _rows(prob["v"])
    B, _, T = rq.shape
    qkv = torch.cat([rq[:, 0], rk[:, past], rv[:, past]], -1)
    kc, vc = torch.full((B, Lmax, T), NAN), torch.full((B, Lmax, T), NAN)
    kc[:, :past], vc[:, :past] = rk[:, :past], rv[:, :past]
    return qkv, kc, vc


def _opt_run(lib, dtype, prob, past, Lmax):
    qkv, kc, vc = _opt_buffers(prob, past, Lmax, dtype)
    B, T = qkv.shape[0], qkv.shape[1] // 3
    it = _in_t(dtype)
    qd = qkv.to(it).cuda()
    kfull, kd = _banded(kc, it)
    vfull, vd = _banded(vc, it)
    ofull, od = _nan_out((B, T), dtype)
    _check(lib, lib.cap_op_opt_decode_attention(dtype, _p(qd), _p(kd), _p(vd), _p(od), B, T, OPT_H, Lmax, past, _stream()))
    torch.cuda.synchronize()
    assert _bands_intact(kfull) and _bands_intact(vfull) and _bands_intact(ofull), "a write outside kc / vc / out"
    for name, cd, img, col in (("k", kd, kc, 1), ("v", vd, vc, 2)):
        got = cd.float().cpu()
        assert torch.equal(cd[:, past], qd[:, col * T:(col + 1) * T]), f"cache row `past` is not the row's {name}, bit for bit"
        assert torch.equal(got[:, :past], img[:, :past].to(it).float()), f"{name} cache rows below `past` changed"
        assert torch.isnan(got[:, past + 1:]).all(), f"{name} cache rows above `past` were written"
    return _read(od, dtype).view(B, 1, T)


@pytest.mark.parametrize("past", OPT_PAST)
@pytest.mark.parametrize("hd", OPT_HD)
@pytest.mark.parametrize("dtype", DTYPES)
def test_opt_decode_step(lib, dtype, hd, past):
    for cls in CLASSES:
        prob = _opt_problem((hd, past), cls, dtype)
        out = _opt_run(lib, dtype, prob, past, past + 3)
        _judge(f"opt_decode {DT_NAME[dtype]} hd {hd} past {past}", "opt", (hd, past), cls, dtype, out, prob)


@pytest.mark.parametrize("past", [12, 65, 1023])
@pytest.mark.parametrize("hd", OPT_HD)
@pytest.mark.parametrize("dtype", DTYPES)
def test_opt_decode_step_row_alone_equals_row_in_a_batch_of_32(lib, dtype, hd, past):
    B, Lmax = 32, past + 2
    prob = _problem("randn", B, OPT_H, 1, past + 1, hd, 77 + hd + past, dtype=dtype)
    qkv, kc, vc = _opt_buffers(prob, past, Lmax, dtype)
    it, T = _in_t(dtype), OPT_H * hd

    def run(rows):
        qd, kd, vd = qkv[rows].to(it).cuda(), kc[rows].to(it).cuda(), vc[rows].to(it).cuda()
        _, od = _nan_out((len(rows), T), dtype)
        _check(lib, lib.cap_op_opt_decode_attention(dtype, _p(qd), _p(kd), _p(vd), _p(od), len(rows), T, OPT_H, Lmax, past, _stream()))
        torch.cuda.synchronize()
        return od.clone()

    whole = run(list(range(B)))
    assert not torch.isnan(whole.float()).any()
    for b in (0, 13, 31):
        assert torch.equal(run([b])[0], whole[b]), b


def test_opt_decode_step_refuses_what_it_cannot_hold(lib):
    T, H = 160, 2
    qkv = torch.zeros(1, 3 * T, device="cuda")
    kc = torch.zeros(1, 1030, T, device="cuda")
    out = torch.zeros(1, T, device="cuda")
    call = lambda Lmax, past, t=T, h=H: lib.cap_op_opt_decode_attention(F32, _p(qkv), _p(kc), _p(kc), _p(out), 1, t, h, Lmax, past, _stream())  # noqa: E731
    _refused(lib, call(1030, 1024), "past=1024")
    _refused(lib, call(8, 8), "past=8 Lmax=8")
    _refused(lib, call(8, 9), "past=9")
    _refused(lib, call(8, -1), "past=-1")
    _refused(lib, call(8, 1, 152, 2), "T=152")          # head_dim 76 is not a multiple of 8


# the fallback of the step: kv_append + generic attention with one query (generic_decode_attention_kernel up to 1024 keys, the
# lane = query kernel beyond), the layout opt_attention passes
OPT_FALLBACK_LK = [1, 63, 64, 65, 1024, 1025]


@pytest.mark.parametrize("Lk", OPT_FALLBACK_LK)
@pytest.mark.parametrize("hd", OPT_HD)
@pytest.mark.parametrize("dtype", DTYPES)
def test_opt_decode_fallback_kv_append_then_one_query_attention(lib, dtype, hd, Lk):
    past, Lmax, it = Lk - 1, Lk + 2, _in_t(dtype)
    for cls in CLASSES:
        prob = _opt_problem((hd, past), cls, dtype)
        qkv, kc, vc = _opt_buffers(prob, past, Lmax, dtype)
        B, T = qkv.shape[0], OPT_H * hd
        qd = qkv.to(it).cuda()
        kfull, kd = _banded(kc, it)
        vfull, vd = _banded(vc, it)
        ofull, od = _nan_out((B, T), dtype)
        _check(lib, lib.cap_op_kv_append(dtype, _p(qd), _p(kd), _p(vd), B, 1, T, Lmax, past, _stream()))
        _check(lib, lib.cap_op_attention(dtype, _p(qd), 3 * T, 3 * T, _p(kd), T, Lmax * T, _p(vd), T, Lmax * T, _p(od), T, T, B, 1, Lk,
                                         OPT_H, hd, past, _stream()))
        torch.cuda.synchronize()
        assert _bands_intact(kfull) and _bands_intact(vfull) and _bands_intact(ofull)
        assert torch.equal(kd[:, past], qd[:, T:2 * T]) and torch.equal(vd[:, past], qd[:, 2 * T:])
        assert torch.isnan(kd[:, Lk:].float()).all() and torch.isnan(vd[:, Lk:].float()).all()
        _judge(f"opt_fallback {DT_NAME[dtype]} hd {hd} Lk {Lk}", "opt", (hd, past), cls, dtype, _read(od, dtype).view(B, 1, T), prob)


# ---------------------------------------------------------------------------------------------- kv_append
@pytest.mark.parametrize("L,pos0", [(33, 0), (5, 40)])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_kv_append_is_an_exact_copy_and_moves_nothing_else(lib, dtype, L, pos0):
    B, T, Lmax, it = 3, 160, 48, _in_t(dtype)
    g = torch.Generator().manual_seed(L)
    qkv = (torch.randn(B * L, 3 * T, generator=g) * 1.5).to(it).cuda()
    before = torch.randn(B, Lmax, T, generator=g)
    kfull, kd = _banded(before, it)
    vfull, vd = _banded(-before, it)
    k0, v0 = kd.clone(), vd.clone()
    _check(lib, lib.cap_op_kv_append(dtype, _p(qkv), _p(kd), _p(vd), B, L, T, Lmax, pos0, _stream()))
    torch.cuda.synchronize()
    assert _bands_intact(kfull) and _bands_intact(vfull)
    rows = qkv.view(B, L, 3 * T)
    k0[:, pos0:pos0 + L], v0[:, pos0:pos0 + L] = rows[:, :, T:2 * T], rows[:, :, 2 * T:]
    assert torch.equal(kd, k0) and torch.equal(vd, v0)
    _refused(lib, lib.cap_op_kv_append(dtype, _p(qkv), _p(kd), _p(vd), B, L, T, Lmax, Lmax - L + 1, _stream()), "do not fit")


# ---------------------------------------------------------------------------------------------- four-wave kernel (the Q-Former)
KP_H = 2
KP_HD = [64, 32, 40]                       # 40: the d < hd padding of HDP 64
KP_SELF_N = [16, 17, 32, 33, 64]
KP_CROSS = [(Lq, Lk) for Lk in (257, 677, 16, 19, 129, 15) for Lq in (7, 32, 64)]       # 15 keys: the lane = query kernel


def _kp_peaks(Lk):
    # wave w walks keys w * per .. in staging chunks of 32: the segment ends and every chunk start inside a segment
    per = (Lk + 3) // 4
    return _sides([w * per + c for w in range(4) for c in range(0, per, 32)], Lk)


def _kp_problem(case, cls, dtype):
    hd, Lq, Lk = case
    peaks = _kp_peaks(Lk)
    return _problem(cls, _slots(cls, peaks, KP_H), KP_H, Lq, Lk, hd, 31 * hd + 7 * Lq + Lk, peaks, dtype=dtype)


def _kp_self_run(lib, dtype, prob, entry="attention"):
    """self-attention through fused q|k|v rows [B * N, 3 D]."""
    rq, rk, rv = _rows(prob["q"]), _rows(prob["k"]), _rows(prob["v"])
    B, N, D = rq.shape
    H, hd, it = prob["q"].shape[1], prob["q"].shape[3], _in_t(dtype)
    qkv = torch.cat([rq, rk, rv], -1).to(it).cuda()
    ofull, od = _nan_out((B, N, D), dtype)
    e = qkv.element_size()
    if entry == "attention":
        q, k, v = (C.c_void_p(qkv.data_ptr() + i * D * e) for i in range(3))
        _check(lib, lib.cap_op_attention(dtype, q, 3 * D, N * 3 * D, k, 3 * D, N * 3 * D, v, 3 * D, N * 3 * D, _p(od), D, N * D, B, N, N, H,
                                         hd, -1, _stream()))
    else:
        _check(lib, lib.cap_op_generic_attention(dtype, _p(qkv), _p(od), B, N, H, hd, _stream()))
    torch.cuda.synchronize()
    assert _bands_intact(ofull)
    return od


def _kp_cross_run(lib, dtype, prob):
    """q in [B * Lq, D], k | v interleaved in [B * Lk, 2 D] (run_qformer's layout)."""
    rq, rk, rv = _rows(prob["q"]), _rows(prob["k"]), _rows(prob["v"])
    B, Lq, D = rq.shape
    Lk, H, hd, it = rk.shape[1], prob["q"].shape[1], prob["q"].shape[3], _in_t(dtype)
    qd = rq.to(it).cuda()
    kv = torch.cat([rk, rv], -1).to(it).cuda()
    ofull, od = _nan_out((B, Lq, D), dtype)
    v = C.c_void_p(kv.data_ptr() + D * kv.element_size())
    _check(lib, lib.cap_op_attention(dtype, _p(qd), D, Lq * D, _p(kv), 2 * D, Lk * 2 * D, v, 2 * D, Lk * 2 * D, _p(od), D, Lq * D, B, Lq, Lk,
                                     H, hd, -1, _stream()))
    torch.cuda.synchronize()
    assert _bands_intact(ofull)
    return od


@pytest.mark.parametrize("N", KP_SELF_N)
@pytest.mark.parametrize("hd", KP_HD)
@pytest.mark.parametrize("dtype", DTYPES)
def test_four_wave_self_attention(lib, dtype, hd, N):
    for cls in CLASSES:
        prob = _kp_problem((hd, N, N), cls, dtype)
        out = _read(_kp_self_run(lib, dtype, prob), dtype)
        _judge(f"kp_self {DT_NAME[dtype]} hd {hd} N {N}", "kp", (hd, N, N), cls, dtype, out, prob)


@pytest.mark.parametrize("Lq,Lk", KP_CROSS)
@pytest.mark.parametrize("hd", KP_HD)
@pytest.mark.parametrize("dtype", DTYPES)
def test_four_wave_cross_attention(lib, dtype, hd, Lq, Lk):
    for cls in CLASSES:
        prob = _kp_problem((hd, Lq, Lk), cls, dtype)
        out = _read(_kp_cross_run(lib, dtype, prob), dtype)
        _judge(f"kp_cross {DT_NAME[dtype]} hd {hd} Lq {Lq} Lk {Lk}", "kp", (hd, Lq, Lk), cls, dtype, out, prob)


@pytest.mark.parametrize("dtype", DTYPES)
def test_qformer_self_attention_entry_point(lib, dtype):
    """cap_op_generic_attention at N = 64, 12 heads of 64: the Q-Former's own call."""
    peaks = _kp_peaks(64)
    for cls in CLASSES:
        prob = _problem(cls, 2, 12, 64, 64, 64, 4242, peaks, dtype=dtype)
        out = _read(_kp_self_run(lib, dtype, prob, entry="generic"), dtype)
        _judge(f"kp_generic_entry {DT_NAME[dtype]} hd 64 N 64 H 12", "kp", (64, 64, 64), cls, dtype, out, prob)


@pytest.mark.parametrize("Lq,Lk", [(32, 32), (32, 257), (64, 677)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_four_wave_row_alone_equals_row_in_a_batch(lib, dtype, Lq, Lk):
    prob = _problem("randn", 8, KP_H, Lq, Lk, 64, 5 + Lk, dtype=dtype)
    whole = _kp_cross_run(lib, dtype, prob).clone()
    assert not torch.isnan(whole.float()).any()
    for b in (0, 5, 7):
        one = {k: (t[b:b + 1] if k in "qkv" else t) for k, t in prob.items()}
        assert torch.equal(_kp_cross_run(lib, dtype, one)[0], whole[b]), b


# ---------------------------------------------------------------------------------------------- lane = query kernel
LQ_WIDE = [(BF16, 88, 677), (BF16, 88, 65), (BF16, 88, 300)] + [(dt, hd, N) for dt in (F32, BF16) for hd in (104, 128) for N in (65, 300)]
LQ_CAUSAL = [(hd, Lq, past) for hd in (80, 64) for Lq in (5, 33, 70) for past in (1, 31, 32, 40)]
LQ_H = 2


def _lq_wide_problem(case, cls, dtype):
    hd, N = case
    peaks = _sides(range(32, N, 32), N)                      # the LDS staging chunk
    return _problem(cls, _slots(cls, peaks, LQ_H), LQ_H, N, N, hd, 13 * hd + N, peaks, dtype=dtype)


def _lq_causal_problem(case, cls, dtype):
    hd, Lq, past = case
    Lk = past + Lq
    peaks = _sides(list(range(32, Lk, 32)) + [past, past + 1], Lk)
    i, j = torch.arange(Lq).view(Lq, 1), torch.arange(Lk).view(1, Lk)
    return _problem(cls, _slots(cls, peaks, LQ_H), LQ_H, Lq, Lk, hd, 17 * hd + 3 * Lq + past, peaks, mask=(j <= i + past).view(1, 1, Lq, Lk),
                    dtype=dtype)


@pytest.mark.parametrize("dtype,hd,N", LQ_WIDE)
def test_lane_per_query_wide_heads(lib, dtype, hd, N):
    """generic_attention_kernel at HDP 96 in bf16 (ViT-g's 88-wide heads) and HDP 128 (hd 104, 128): cap_op_vit_attention_hd, impl 1."""
    for cls in CLASSES:
        prob = _lq_wide_problem((hd, N), cls, dtype)
        rq, rk, rv = _rows(prob["q"]), _rows(prob["k"]), _rows(prob["v"])
        B, _, D = rq.shape
        qkv = torch.cat([rq, rk, rv], -1).to(_in_t(dtype)).cuda()
        ofull, od = _nan_out((B, N, D), dtype)
        _check(lib, lib.cap_op_vit_attention_hd(dtype, _p(qkv), _p(od), B, N, LQ_H, hd, 1, _stream()))
        torch.cuda.synchronize()
        assert _bands_intact(ofull)
        _judge(f"lane_query {DT_NAME[dtype]} hd {hd} N {N}", "lq_wide", (hd, N), cls, dtype, _read(od, dtype), prob)


@pytest.mark.parametrize("hd,Lq,past", LQ_CAUSAL)
@pytest.mark.parametrize("dtype", DTYPES)
def test_lane_per_query_prompt_continuation_against_the_cache(lib, dtype, hd, Lq, past):
    """causal_off = past: Lq new rows (fused q|k|v) against past + Lq cached keys; cache rows [B][Lmax][T], NaN beyond the keys."""
    Lk, it = past + Lq, _in_t(dtype)
    Lmax = Lk + 3
    for cls in CLASSES:
        prob = _lq_causal_problem((hd, Lq, past), cls, dtype)
        rq, rk, rv = _rows(prob["q"]), _rows(prob["k"]), _rows(prob["v"])
        B, _, T = rq.shape
        qkv = torch.cat([rq, torch.full_like(rq, NAN), torch.full_like(rq, NAN)], -1).to(it).cuda()     # k | v are read from the cache
        kc, vc = torch.full((B, Lmax, T), NAN), torch.full((B, Lmax, T), NAN)
        kc[:, :Lk], vc[:, :Lk] = rk, rv
        kd, vd = kc.to(it).cuda(), vc.to(it).cuda()
        ofull, od = _nan_out((B, Lq, T), dtype)
        _check(lib, lib.cap_op_attention(dtype, _p(qkv), 3 * T, Lq * 3 * T, _p(kd), T, Lmax * T, _p(vd), T, Lmax * T, _p(od), T, Lq * T, B, Lq,
                                         Lk, LQ_H, hd, past, _stream()))
        torch.cuda.synchronize()
        assert _bands_intact(ofull)
        _judge(f"lane_query_causal {DT_NAME[dtype]} hd {hd} Lq {Lq} past {past}", "lq_causal", (hd, Lq, past), cls, dtype, _read(od, dtype), prob)


# ---------------------------------------------------------------------------------------------- ITM two-segment self-attention
ITM_SHAPES = [(32, 32), (32, 1), (32, 7), (0, 32), (0, 1), (32, 0), (5, 9)]
ITM_H = 2


def _itm_lens(L, B):
    base = [1, L, 0, L + 3, (L + 1) // 2, max(1, L - 1)]          # 0 is clamped to 1, L + 3 to L
    return [base[b % len(base)] for b in range(B)]


def _itm_problem(case, cls, dtype, B=None, lens=None):
    nq, L = case
    nk = nq + L
    peaks = _sides([nq, 32], nk)
    B = _slots(cls, peaks, ITM_H) if B is None else B
    B = max(B, 6)
    lens = _itm_lens(L, B) if lens is None else lens
    eff = torch.tensor([min(max(n, 1), L) if L > 0 else 0 for n in lens])
    j = torch.arange(nk).view(1, nk)
    seen = (j < nq) | (j - nq < eff.view(B, 1))                     # [B, nk]: HF's key mask [1 x nq | attention_mask]
    # a peak lands on a key every pair sees: the position is folded into the pair's own key count
    prob = _problem(cls, B, ITM_H, nk, nk, 64, 100 * nq + L, [0], mask=seen.view(B, 1, 1, nk), dtype=dtype)
    if cls == "peaked":
        prob = _itm_peaked(prob, peaks, nq, eff, dtype, 100 * nq + L)
    prob["seen"], prob["eff"] = seen, eff
    return prob


def _itm_peaked(prob, peaks, nq, eff, dtype, seed):
    B, H, nk, hd = prob["k"].shape
    g = torch.Generator().manual_seed(seed)
    u = torch.randn(B, H, 1, hd, generator=g)
    u = u / u.norm(dim=-1, keepdim=True) * math.sqrt(hd)
    q, k = u + 0.5 * torch.randn(B, H, nk, hd, generator=g), 0.5 * torch.randn(B, H, nk, hd, generator=g)
    for s in range(B * H):
        b, h = divmod(s, H)
        k[b, h, min(peaks[s % len(peaks)], nq + int(eff[b]) - 1)] += 20.0 / (prob["scale"] * hd) * u[b, h, 0]
    prob["q"], prob["k"] = _rounded(q, dtype), _rounded(k, dtype)
    return prob


def _itm_run(lib, dtype, prob, nq, L):
    """-> (ctx_q [B, nq, W] or None, ctx_t [B, L, W] or None) device outputs.  K / V of text rows the pair does not see are NaN."""
    rq, rk, rv = _rows(prob["q"]), _rows(prob["k"]), _rows(prob["v"])
    B, nk, W = rq.shape
    hide = ~prob["seen"].view(B, nk, 1).expand(B, nk, W)
    rk, rv = rk.masked_fill(hide, NAN), rv.masked_fill(hide, NAN)
    rows = torch.cat([rq, rk, rv], -1).to(_in_t(dtype))
    qq = rows[:, :nq].contiguous().cuda() if nq else None
    qt = rows[:, nq:].contiguous().cuda() if L else None
    lens = torch.tensor(prob["lens"], dtype=torch.int32).cuda() if L else None
    fq, cq = _nan_out((B, nq, W), dtype) if nq else (None, None)
    ft, ct = _nan_out((B, L, W), dtype) if L else (None, None)
    _check(lib, lib.cap_op_itm_self_attention(dtype, _p(qq), _p(qt), _p(lens), _p(cq), _p(ct), B, nq, L, ITM_H, _stream()))
    torch.cuda.synchronize()
    assert (fq is None or _bands_intact(fq)) and (ft is None or _bands_intact(ft))
    return cq, ct


def _itm_out(cq, ct, dtype):
    parts = [_read(c, dtype) for c in (cq, ct) if c is not None]
    return torch.cat(parts, 1)


def _itm_keep(prob, nq, L):
    """query rows and the text rows below the pair's length; the rows beyond it are read by nobody, here neither."""
    B = prob["seen"].shape[0]
    i = torch.arange(nq + L).view(1, nq + L)
    return (i < nq) | (i - nq < prob["eff"].view(B, 1))


@pytest.mark.parametrize("nq,L", ITM_SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_itm_two_segment_self_attention(lib, dtype, nq, L):
    for cls in CLASSES:
        prob = _itm_problem((nq, L), cls, dtype)
        prob["lens"] = _itm_lens(L, prob["q"].shape[0])
        cq, ct = _itm_run(lib, dtype, prob, nq, L)
        _judge(f"itm_self {DT_NAME[dtype]} nq {nq} L {L}", "itm", (nq, L), cls, dtype, _itm_out(cq, ct, dtype), prob, keep=_itm_keep(prob, nq, L))


@pytest.mark.parametrize("dtype", DTYPES)
def test_itm_pair_alone_equals_pair_in_a_batch_of_64_and_padded_to_32(lib, dtype):
    nq, L, B = 32, 32, 64
    lens = [1 + (5 * b) % 32 for b in range(B)]
    prob = _itm_problem((nq, L), "randn", dtype, B=B, lens=lens)
    prob["lens"] = lens
    cq, ct = _itm_run(lib, dtype, prob, nq, L)
    cq, ct = cq.clone(), ct.clone()
    for b in (0, 17, 63):
        n = lens[b]
        one = {k: (t[b:b + 1] if k in ("q", "k", "v", "mask", "seen", "eff") else t) for k, t in prob.items()}
        one["lens"] = [n]
        aq, at = _itm_run(lib, dtype, one, nq, L)
        assert torch.equal(aq[0], cq[b]) and torch.equal(at[0, :n], ct[b, :n]), ("alone", b)
        # the same pair with its text rows cut to its own length
        keys = list(range(nq + n))
        cut = {"q": one["q"][:, :, keys], "k": one["k"][:, :, keys], "v": one["v"][:, :, keys], "seen": one["seen"][:, keys],
               "eff": one["eff"], "scale": one["scale"], "lens": [n]}
        sq, st = _itm_run(lib, dtype, cut, nq, n)
        assert torch.equal(sq[0], cq[b]) and torch.equal(st[0], ct[b, :n]), ("L = lens[b]", b)


def test_itm_self_attention_refuses_what_it_cannot_hold(lib):
    x = torch.zeros(64, 3 * 128, device="cuda")
    o = torch.zeros(64, 128, device="cuda")
    lens = torch.ones(1, dtype=torch.int32, device="cuda")
    _refused(lib, lib.cap_op_itm_self_attention(F32, _p(x), _p(x), _p(lens), _p(o), _p(o), 1, 33, 8, 2, _stream()), "nq=33")
    _refused(lib, lib.cap_op_itm_self_attention(F32, _p(x), _p(x), _p(lens), _p(o), _p(o), 1, 8, 33, 2, _stream()), "L=33")
    _refused(lib, lib.cap_op_itm_self_attention(F32, _p(x), _p(x), _p(None), _p(o), _p(o), 1, 8, 8, 2, _stream()), "itm_self_attention")


# ---------------------------------------------------------------------------------------------- sentence-encoder attention
TEXT_L = {32: [1, 24, 63, 64, 65, 128, 200, 256, 400, 512], 64: [1, 24, 63, 64, 65, 128, 200, 256]}      # the launcher's whole range
TEXT_CASES = [(hd, L) for hd in (32, 64) for L in TEXT_L[hd]]
TEXT_H = 2


def _text_lens(L, B):
    base = [L, 1, 0, L + 3, (L + 1) // 2, max(1, L - 1)]
    return [base[b % len(base)] for b in range(B)]


def _text_problem(case, cls, dtype, B=None, lens=None):
    hd, L = case
    peaks = _sides([64 * i for i in range(1, 8)], L)
    B = max(6, _slots(cls, peaks, TEXT_H)) if B is None else B
    lens = _text_lens(L, B) if lens is None else lens
    eff = torch.tensor([min(max(n, 1), L) for n in lens])
    seen = torch.arange(L).view(1, L) < eff.view(B, 1)
    scale = 0.17677669529663687 if hd == 32 else 0.125
    folded = [[min(p, int(e) - 1) for p in peaks] for e in eff]
    prob = _problem("randn" if cls == "peaked" else cls, B, TEXT_H, L, L, hd, 9 * hd + L, mask=seen.view(B, 1, 1, L), scale=scale, dtype=dtype)
    if cls == "peaked":
        g = torch.Generator().manual_seed(9 * hd + L)
        u = torch.randn(B, TEXT_H, 1, hd, generator=g)
        u = u / u.norm(dim=-1, keepdim=True) * math.sqrt(hd)
        q, k = u + 0.5 * torch.randn(B, TEXT_H, L, hd, generator=g), 0.5 * torch.randn(B, TEXT_H, L, hd, generator=g)
        for s in range(B * TEXT_H):
            b, h = divmod(s, TEXT_H)
            k[b, h, folded[b][s % len(peaks)]] += 20.0 / (scale * hd) * u[b, h, 0]
        prob["q"], prob["k"] = _rounded(q, dtype), _rounded(k, dtype)
    prob["seen"], prob["eff"], prob["lens"] = seen, eff, lens
    return prob


def _text_run(lib, dtype, prob):
    rq, rk, rv = _rows(prob["q"]), _rows(prob["k"]), _rows(prob["v"])
    B, L, D = rq.shape
    hide = ~prob["seen"].view(B, L, 1).expand(B, L, D)
    qkv = torch.cat([rq, rk.masked_fill(hide, NAN), rv.masked_fill(hide, NAN)], -1).to(_in_t(dtype)).cuda()
    lens = torch.tensor(prob["lens"], dtype=torch.int32).cuda()
    ofull, od = _nan_out((B, L, D), dtype)
    _check(lib, lib.cap_op_text_attention(dtype, _p(qkv), _p(lens), _p(od), B, L, TEXT_H, prob["q"].shape[3], _stream()))
    torch.cuda.synchronize()
    assert _bands_intact(ofull)
    return od


@pytest.mark.parametrize("hd,L", TEXT_CASES)
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_text_attention(lib, dtype, hd, L):
    for cls in CLASSES:
        prob = _text_problem((hd, L), cls, dtype)
        out = _read(_text_run(lib, dtype, prob), dtype)
        _judge(f"text_attention {DT_NAME[dtype]} hd {hd} L {L}", "text", (hd, L), cls, dtype, out, prob, keep=prob["seen"])


@pytest.mark.parametrize("hd,L", [(32, 24), (32, 512), (64, 65), (64, 256)])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_text_attention_sentence_alone_equals_in_a_batch_and_padded_longer(lib, dtype, hd, L):
    B = 16
    lens = [1 + (7 * b) % L for b in range(B)]
    prob = _text_problem((hd, L), "randn", dtype, B=B, lens=lens)
    whole = _text_run(lib, dtype, prob).clone()
    for b in (0, 9, 15):
        n = lens[b]
        one = {k: (t[b:b + 1] if k in ("q", "k", "v", "mask", "seen", "eff") else t) for k, t in prob.items()}
        one["lens"] = [n]
        assert torch.equal(_text_run(lib, dtype, one)[0, :n], whole[b, :n]), ("alone", b)
        cut = {"q": one["q"][:, :, :n], "k": one["k"][:, :, :n], "v": one["v"][:, :, :n], "seen": one["seen"][:, :n], "lens": [n]}
        assert torch.equal(_text_run(lib, dtype, cut)[0], whole[b, :n]), ("L = lens[b]", b)


def test_text_attention_refuses_lengths_its_lds_cannot_hold(lib):
    """2 * L * head_dim * 4 bytes of LDS, at most 128 KB: 512 tokens at head_dim 32, 256 at 64 - at the launcher and at cap_create."""
    from embodied_captioning_amd import _native as N
    x = torch.zeros(8, device="cuda")
    lens = torch.ones(1, dtype=torch.int32, device="cuda")
    for hd, L in [(32, 513), (64, 257), (64, 512), (32, 0), (48, 8)]:
        _refused(lib, lib.cap_op_text_attention(F32, _p(x), _p(lens), _p(x), 1, L, 1, hd, _stream()), "text_attention")
    _refused(lib, lib.cap_op_text_attention(SPLIT, _p(x), _p(lens), _p(x), 1, 8, 1, 32, _stream()), "CAP_F32 or CAP_BF16")

    def create(heads, max_len):
        cfg = N.CapConfig()
        cfg.struct_size = C.sizeof(N.CapConfig)
        cfg.arch, cfg.compute_dtype = 2, N.CAP_F32
        cfg.t_hidden, cfg.t_layers, cfg.t_heads, cfg.t_ffn = 128, 1, heads, 128
        cfg.vocab, cfg.max_pos, cfg.t_eps = 64, 512, 1e-12
        cfg.max_batch, cfg.max_beams, cfg.max_len = 2, 1, max_len
        h = C.c_void_p()
        rc = lib.cap_create(C.byref(cfg), C.byref(h))
        if rc == 0:
            assert lib.cap_destroy(h) == 0
        return rc

    _refused(lib, create(2, 257), "max_len 257")           # head_dim 64
    _refused(lib, create(2, 512), "max_len 512")
    assert create(2, 256) == 0, lib.cap_last_error().decode()
    assert create(4, 512) == 0, lib.cap_last_error().decode()      # head_dim 32


# ---------------------------------------------------------------------------------------------- CoCa pooler
POOL_SHAPES = [(257, 256), (577, 256), (257, 1), (33, 65), (1, 3), (32, 64)]
POOL_CASES = [(hd, N, Q) for hd in (64, 96) for N, Q in POOL_SHAPES]
POOL_H = 2


def _pool_problem(case, cls, dtype):
    hd, N, Q = case
    peaks = _sides(range(32, N, 32), N)                       # K / V tiles of 32 keys
    prob = _problem(cls, _slots(cls, peaks, POOL_H), POOL_H, Q, N, hd, 5 * hd + 3 * N + Q, peaks, dtype=dtype)
    # the learned queries are shared by the batch and stay fp32 whatever the type of k | v
    g = torch.Generator().manual_seed(5 * hd + 3 * N + Q)
    if cls == "randn":
        prob["q"] = (torch.randn(1, POOL_H, Q, hd, generator=g) * 1.5).expand(prob["k"].shape[0], -1, -1, -1).contiguous()
    return prob


@pytest.mark.parametrize("hd,N,Q", POOL_CASES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_pool_attention(lib, dtype, hd, N, Q):
    for cls in CLASSES:
        prob = _pool_problem((hd, N, Q), cls, dtype)
        if cls != "randn":           # one query table for the batch: every slot's queries are slot 0's, the keys follow their own u
            prob = _pool_shared_queries(prob, cls, dtype, hd, N, Q)
        B, E = prob["k"].shape[0], POOL_H * hd
        qp = _rows(prob["q"][:1])[0].contiguous().cuda()                              # [Q, E] fp32
        kv = torch.cat([_rows(prob["k"]), _rows(prob["v"])], -1).to(_in_t(dtype)).cuda()      # [B, N, 2 E]: K then V
        ofull, od = _nan_out((B, Q, E), dtype)
        _check(lib, lib.cap_op_pool_attention(dtype, _p(qp), _p(kv), _p(od), B, N, Q, E, POOL_H, _stream()))
        torch.cuda.synchronize()
        assert _bands_intact(ofull), "the clamped query lane wrote beyond out"
        _judge(f"pool_attention {DT_NAME[dtype]} hd {hd} N {N} Q {Q}", "pool", (hd, N, Q), cls, dtype, _read(od, dtype), prob)


def _pool_shared_queries(prob, cls, dtype, hd, N, Q):
    """rising / peaked with ONE query table: the direction u is per head only, so every batch slot's keys line up with the same queries."""
    B = prob["k"].shape[0]
    peaks = _sides(range(32, N, 32), N)
    g = torch.Generator().manual_seed(hd + N + Q)
    u = torch.randn(1, POOL_H, 1, hd, generator=g)
    u = u / u.norm(dim=-1, keepdim=True) * math.sqrt(hd)
    scale = prob["scale"]
    if cls == "rising":
        q, k = u + 0.1 * torch.randn(1, POOL_H, Q, hd, generator=g), 0.02 * torch.randn(B, POOL_H, N, hd, generator=g)
        k = k + (min(3.0, 96.0 / N) * torch.arange(N, dtype=torch.float32) / (scale * hd)).view(1, 1, N, 1) * u
    else:
        q, k = u + 0.5 * torch.randn(1, POOL_H, Q, hd, generator=g), 0.5 * torch.randn(B, POOL_H, N, hd, generator=g)
        for s in range(B * POOL_H):
            b, h = divmod(s, POOL_H)
            k[b, h, peaks[s % len(peaks)]] += 20.0 / (scale * hd) * u[0, h, 0]
    prob["q"], prob["k"] = q.expand(B, -1, -1, -1).contiguous(), _rounded(k, dtype)
    return prob


def test_pool_attention_refuses_bad_widths(lib):
    x = torch.zeros(1024, device="cuda")
    _refused(lib, lib.cap_op_pool_attention(F32, _p(x), _p(x), _p(x), 1, 2, 2, 160, 2, _stream()), "head_dim 80")
    _refused(lib, lib.cap_op_pool_attention(F32, _p(x), _p(x), _p(x), 1, 0, 2, 128, 2, _stream()), "pool_attention")


FAMILIES.update({
    "opt": {"cases": [(hd, p) for hd in OPT_HD for p in OPT_PAST], "problem": _opt_problem},
    "kp": {"cases": [(hd, n, n) for hd in KP_HD for n in KP_SELF_N] + [(hd, lq, lk) for hd in KP_HD for lq, lk in KP_CROSS], "problem": _kp_problem},
    "lq_wide": {"cases": sorted({(hd, n) for _, hd, n in LQ_WIDE}), "problem": _lq_wide_problem},
    "lq_causal": {"cases": LQ_CAUSAL, "problem": _lq_causal_problem},
    "itm": {"cases": ITM_SHAPES, "problem": _itm_problem},
    "text": {"cases": TEXT_CASES, "problem": _text_problem},
    "pool": {"cases": POOL_CASES, "problem": _pool_problem},
})
