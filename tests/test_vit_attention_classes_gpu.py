"""GPU: the seven MFMA ViT attention kernels (csrc/attention.hip on csrc/vit_attn_frag.h) and vit_attention_scalar, kernel by kernel,
against the float64 reference of tests/_attention_ref.py, through cap_op_vit_attention and cap_op_vit_attention_hd.

Four input classes per class case - randn, rising (every chunk of an online softmax rescales), peaked (one (image, head) slot per
peak position: key 0, key N - 1, both sides of every multiple of 32 below N - which are all the chunk (96 / 128 / 160 keys),
query-group (128 / 256 queries) and key-tile (128) boundaries these kernels have - and every key of the first and of the last key
block, i.e. all 16 accumulator elements of both lane halves and every padding count) and positive (randn with v >= 0.5, for the
bias check).  Sweep cases run randn at every N of a range, so that every padding count 0 .. 31 of the last key block occurs.

Bars: _attention_ref._figures, derived from the reference alone.  fp32 context: 8 x ref_err_fp32.  G8 context: + the container's
error.  bf16 context: |out - ref| - 2^-8 |ref| (- 2^-8 p_abs for the MFMA kernels, which round P to bf16) elementwise.  The bias
check holds the mean relative error of a positive case to 6 r / sqrt(n).
Every context buffer starts as NaN between canary bands, q | k | v sit between bands too; a refused launch fails the test.
Run with -s for the table (profiles/vit_attention_classes_gpu_tolerances.txt is that output)."""
import ctypes as C
import functools

import pytest
import torch

from _attention_ref import (BF16, F32, FAMILIES, G8IN, SPLIT, _bias, _causal_mask, _judge, _p_abs, _problem_in, _reference, _rows,
                            _slots)
from _util import g8_decode, g8_encode

pytestmark = pytest.mark.gpu

H = 2
CLASSES = ("randn", "rising", "peaked", "positive")
DT_NAME = {F32: "f32", BF16: "bf16", SPLIT: "g8"}
NAN = float("nan")
GUARD, CANARY = 256, 77.0            # canary bands of GUARD elements either side of every buffer
WORST = {}                           # (kernel, context type, class) -> worst judged / bar


@pytest.fixture(scope="module")
def lib():
    from embodied_captioning_amd import _native
    assert torch.cuda.is_available(), "these tests need the MI355X"
    yield _native.load_library()
    print("\n# worst judged / bar per kernel, context type and class")
    for (kernel, ctx, cls), ratio in sorted(WORST.items()):
        print(f"# {kernel:<28s} {ctx:<5s} {cls:<8s} {ratio: .3f}")


def _p(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _banded(values, tdtype):
    """values (CPU, any shape) -> (full, body): a device buffer with canary bands either side, body viewed in values' shape."""
    n = values.numel()
    full = torch.full((n + 2 * GUARD,), CANARY, dtype=tdtype, device="cuda")
    body = full[GUARD:GUARD + n].view(values.shape)
    body.copy_(values.to(tdtype))
    return full, body


def _bands_intact(full):
    return bool((full[:GUARD] == CANARY).all().item() and (full[-GUARD:] == CANARY).all().item())


def _read(body, dtype):
    """Device context -> fp32 CPU values."""
    if dtype == SPLIT:
        return torch.from_numpy(g8_decode(body.cpu().numpy()))
    return body.float().cpu()


# ---------------------------------------------------------------------------------------------- the table
# The dispatch rules of launch_vit_attention (csrc/attention.hip), kb = ceil(N / 32); _dispatch below is those rules in Python and
# every launch is checked against it.
def _f32_mfma_name(N, hd):
    return f"f32_mfma<{(N + 31) // 32}>"


def _wide_name(N, hd):
    return f"f32_mfma_wide<3,{(hd + 31) // 32}>"


ROWS = {
    # bf16, head_dim 64, impl 2: kb 1 / 2 / 7 / 9 -> vit_attention_mfma<kb>, kb 19 -> vit_attention_flash<19, 5> (chunks of 160 keys)
    "mfma1": dict(kernel="mfma<1>", dtypes=[BF16], impls=[2], hds=[64], Ns=[1, 17, 32], sweep=(1, 32, 64)),
    "mfma2": dict(kernel="mfma<2>", dtypes=[BF16], impls=[2], hds=[64], Ns=[33, 50, 64], sweep=(33, 64, 64)),
    "mfma7": dict(kernel="mfma<7>", dtypes=[BF16], impls=[2], hds=[64], Ns=[193, 197, 224], sweep=(193, 224, 64)),
    "mfma9": dict(kernel="mfma<9>", dtypes=[BF16], impls=[2], hds=[64], Ns=[257, 288], sweep=(257, 288, 64)),
    "flash19": dict(kernel="flash<19,5>", dtypes=[BF16], impls=[2], hds=[64], Ns=[577, 593, 608], sweep=(577, 608, 64)),
    # bf16, 64 < head_dim <= 128 (a multiple of 8), impl != 1: kb 9 -> vit_attention_flash_wide<9, 5> (chunks of 160 keys),
    # N <= 64 -> <2, 2>; impl bit 8 of cap_op_vit_attention_hd = the causal mask
    "fwide9": dict(kernel="flash_wide<9,5>", hd_entry=True, dtypes=[BF16], impls=[0], hds=[72, 88, 128], Ns=[257, 288], sweep=(257, 288, 88)),
    "fwide2": dict(kernel="flash_wide<2,2>", hd_entry=True, dtypes=[BF16], impls=[0, 8], hds=[72, 80, 128], Ns=[1, 33, 64],
                   sweep=(1, 64, 80), sweep_impl=8),
    # fp32 q | k | v, head_dim 64, impl != 1, kb 1 / 7 / 9 -> vit_attention_f32_mfma<kb, float or g8_t> (dtype SPLIT: G8 context)
    "f32mfma": dict(kernel=_f32_mfma_name, dtypes=[F32, SPLIT], impls=[0], hds=[64], Ns=[17, 32, 193, 197, 224, 257, 288],
                    sweeps=[(1, 32, 64), (193, 224, 64), (257, 288, 64)]),
    # fp32 q | k | v, head_dim != 64, a multiple of 8 up to 96, not causal, impl != 1 -> vit_attention_f32_mfma_wide<3, ceil(hd / 32)>:
    # chunks of 96 keys, workgroups of 4 query tiles (N = 129: one live wave of four in the second workgroup)
    "f32wide": dict(kernel=_wide_name, hd_entry=True, dtypes=[F32, SPLIT], impls=[0], hds=[8, 32, 40, 56, 72, 88, 96],
                    Ns=[1, 95, 96, 97, 128, 129, 257], sweep=(65, 96, 88)),
    # G8 q | k | v (dtype SPLIT, impl 3 or 5): N <= 64 -> vit_attention_split<2, true>; 193 .. 224 -> <7, true, true> (with impl 3 and
    # more than 256 units: vit_attention_split_pw<7>, below); other N <= 224 -> <7, true>; beyond -> <4, false> (chunks of 128 keys,
    # workgroups of 8 query tiles: 256 / 257 is that boundary)
    "split2": dict(kernel="split<2,true>", g8in=True, dtypes=[SPLIT], impls=[3], hds=[64], Ns=[1, 33, 64], sweep=(1, 64, 64)),
    "split7": dict(kernel="split<7,true>", g8in=True, dtypes=[SPLIT], impls=[3], hds=[64], Ns=[65, 96, 160, 192], sweep=(161, 192, 64)),
    "split7x": dict(kernel="split<7,true,true>", g8in=True, dtypes=[SPLIT], impls=[5], hds=[64], Ns=[193, 197, 224], sweep=(193, 224, 64)),
    "split4": dict(kernel="split<4,false>", g8in=True, dtypes=[SPLIT], impls=[3], hds=[64], Ns=[225, 256, 257, 384, 385, 577]),
    # impl 1, head_dim 64: vit_attention_scalar<bf16>, <float> and <float, g8_t>; key tiles of 128, query blocks of 256
    "scalar": dict(kernel="scalar", dtypes=[BF16, F32, SPLIT], impls=[1], hds=[64], Ns=[1, 128, 129, 256, 257, 300]),
}
PW_N = [193, 197, 224]               # vit_attention_split_pw<7>: B = 129, H = 2 = 258 units on 256 CUs, some workgroups walk two units
PW_B = 129
MFMA_BF16 = ("mfma", "flash")        # the bf16 kernels that round P to bf16 before P.V


def _dispatch(row, dtype, impl, B, N, hd):
    """launch_vit_attention's choice for this call, as the name the table uses."""
    kb = (N + 31) // 32
    if not row.get("hd_entry") and dtype == SPLIT and impl in (3, 5):          # cap_op_vit_attention: G8 q | k | v
        if N <= 64:
            return "split<2,true>"
        if 192 < N <= 224:
            return "split_pw<7>" if impl != 5 and B * H > 256 else "split<7,true,true>"
        return "split<7,true>" if N <= 224 else "split<4,false>"
    causal, impl = (bool(impl & 8), impl & 7) if row.get("hd_entry") else (False, impl)
    if 64 < hd <= 128 and hd % 8 == 0 and dtype == BF16 and impl != 1:
        if kb == 9:
            return "flash_wide<9,5>"
        if N <= 64:
            return "flash_wide<2,2>"
    if dtype != BF16 and not causal and impl != 1 and hd != 64 and hd % 8 == 0 and hd <= 96:
        return f"f32_mfma_wide<3,{(hd + 31) // 32}>"
    if hd != 64 or causal:
        return "generic"
    mfma_ok = dtype == BF16 and kb in (1, 2, 7, 9, 19)
    if impl == 2 and not mfma_ok:
        return "refused"
    if dtype != BF16 and impl != 1 and kb in (1, 7, 9):
        return f"f32_mfma<{kb}>"
    if impl == 0:
        impl = 2 if mfma_ok else 1
    if impl == 2:
        return "flash<19,5>" if kb == 19 else f"mfma<{kb}>"
    return "scalar"


def _kernel(row, N, hd):
    k = row["kernel"]
    return k(N, hd) if callable(k) else k


def _rounding(row, dtype):
    return G8IN if row.get("g8in") else BF16 if dtype == BF16 else F32


# ---------------------------------------------------------------------------------------------- problems and references
def _peaks(N):
    pos = {0, N - 1} | set(range(min(32, N))) | set(range(32 * ((N - 1) // 32), N))
    for b in range(32, N, 32):
        pos.update((b - 1, b))
    return sorted(pos)


def _seed(N, hd, causal):
    return 1000 * hd + 2 * N + int(causal)


@functools.lru_cache(maxsize=4)
def _case(N, hd, cls, rounding, causal, B=None):
    """(problem, (reference, ref_err_fp32), p_abs or None) of one case, computed once and shared by the kernels and context types
    that take it; the reference is formed 8 batch rows at a time."""
    peaks = _peaks(N)
    B = _slots(cls, peaks, H) if B is None else B
    prob = _problem_in(cls, B, H, N, N, hd, _seed(N, hd, causal), peaks, _causal_mask(N) if causal else None, rounding=rounding)
    refs, errs, pas = [], [], []
    for b0 in range(0, B, 8):
        part = {k: (t[b0:b0 + 8] if k in "qkv" else t) for k, t in prob.items()}
        r, e = _reference(part)
        refs.append(r)
        errs.append(e)
        if rounding == BF16:
            pas.append(_p_abs(part))
    return prob, (torch.cat(refs), max(errs)), (torch.cat(pas) if pas else None)


def _family_problem(case, cls, dtype):
    N, hd, causal = case
    return _problem_in(cls, 2, H, N, N, hd, _seed(N, hd, causal), (), _causal_mask(N) if causal else None, rounding=dtype)


FAMILIES.update({"vit_" + name: {"cases": [(N, hd, bool(impl & 8) and bool(row.get("hd_entry")))
                                           for N in row["Ns"] for hd in row["hds"] for impl in row["impls"]],
                                 "problem": _family_problem} for name, row in ROWS.items()})
FAMILIES["vit_pw"] = {"cases": [(N, 64, False) for N in PW_N], "problem": _family_problem}


# ---------------------------------------------------------------------------------------------- launch and judge
def _launch(lib, row, dtype, impl, prob, rounding, expect):
    """q | k | v rows [B * N, 3 * H * hd] between bands -> the context [B, N, H * hd] (device), NaN before the launch."""
    rq, rk, rv = _rows(prob["q"]), _rows(prob["k"]), _rows(prob["v"])
    B, N, D = rq.shape
    hd = D // H
    assert _dispatch(row, dtype, impl, B, N, hd) == expect, (_dispatch(row, dtype, impl, B, N, hd), expect)
    qkv = torch.cat([rq, rk, rv], -1)
    if rounding == G8IN:
        qkv = torch.from_numpy(g8_encode(qkv.numpy()))
    qfull, qd = _banded(qkv, torch.bfloat16 if rounding == BF16 else torch.float32)
    ofull, od = _banded(torch.full((B, N, D), NAN), torch.bfloat16 if dtype == BF16 else torch.float32)
    if row.get("hd_entry"):
        rc = lib.cap_op_vit_attention_hd(dtype, _p(qd), _p(od), B, N, H, hd, impl, _stream())
    else:
        rc = lib.cap_op_vit_attention(dtype, _p(qd), _p(od), B, N, H, impl, _stream())
    assert rc == 0, lib.cap_last_error().decode()
    torch.cuda.synchronize()
    assert _bands_intact(ofull), "a write outside the context"
    assert _bands_intact(qfull), "a write into the bands of q | k | v"
    return od


def _held(kernel, dtype, impl, N, hd, cls, out, case):
    """judge one context against the case's bars, the bias check on the positive class"""
    prob, ref, pa = case
    mfma = kernel.startswith(MFMA_BF16)
    tag = f"{kernel} {DT_NAME[dtype]}{' causal' if impl & 8 else ''} N {N} hd {hd}"
    errors = []
    try:
        f = _judge(tag, "vit_" + _ROW_OF[kernel], (N, hd), cls, dtype, out, prob, ref=ref, p_abs=pa if mfma else None)
    except AssertionError as e:
        if "non-finite" in str(e):
            raise
        errors.append(str(e))
        f = None
    if f is not None:
        key = (kernel, DT_NAME[dtype], cls)
        WORST[key] = max(WORST.get(key, float("-inf")), f["worst"] / f["bar"])
        if cls == "positive":
            mean, limit = _bias(f, dtype, mfma)
            print(f"{tag:<58s} bias   mean (out - ref) / ref {mean: .3e}  limit {limit:.3e}")
            if abs(mean) > limit:
                errors.append(f"bias {tag}: {mean} beyond {limit}")
    return errors


_ROW_OF = {}
for _name, _row in ROWS.items():
    for _N in _row["Ns"]:
        for _hd in _row["hds"]:
            _ROW_OF[_kernel(_row, _N, _hd)] = _name
_ROW_OF["split_pw<7>"] = "pw"

CLASS_CASES = [(name, hd, N) for name, row in ROWS.items() for hd in row["hds"] for N in row["Ns"]]


@pytest.mark.parametrize("name,hd,N", CLASS_CASES, ids=[f"{n}-hd{hd}-N{N}" for n, hd, N in CLASS_CASES])
def test_class_cases(lib, name, hd, N):
    row, errors = ROWS[name], []
    kernel = _kernel(row, N, hd)
    for cls in CLASSES:
        for impl in row["impls"]:
            for dtype in row["dtypes"]:
                rounding = _rounding(row, dtype)
                case = _case(N, hd, cls, rounding, bool(impl & 8) and bool(row.get("hd_entry")))
                od = _launch(lib, row, dtype, impl, case[0], rounding, kernel)
                errors += _held(kernel, dtype, impl, N, hd, cls, _read(od, dtype), case)
    assert not errors, errors


SWEEPS = [(name, sw) for name, row in ROWS.items() for sw in row.get("sweeps", [row["sweep"]] if "sweep" in row else [])]


@pytest.mark.parametrize("name,sweep", SWEEPS, ids=[f"{n}-N{s[0]}..{s[1]}-hd{s[2]}" for n, s in SWEEPS])
def test_sweep_every_padding_count(lib, name, sweep):
    """randn at every N of the range: every number of padding keys in the last key block, 0 .. 31."""
    row, errors = ROWS[name], []
    lo, hi, hd = sweep
    impl = row.get("sweep_impl", row["impls"][0])
    for N in range(lo, hi + 1):
        for dtype in row["dtypes"]:
            rounding = _rounding(row, dtype)
            case = _case(N, hd, "randn", rounding, bool(impl & 8) and bool(row.get("hd_entry")))
            kernel = _kernel(row, N, hd)
            od = _launch(lib, row, dtype, impl, case[0], rounding, kernel)
            errors += _held(kernel, dtype, impl, N, hd, "randn", _read(od, dtype), case)
    assert not errors, errors


@pytest.mark.parametrize("N", PW_N)
def test_persistent_split_kernel_and_its_tie_to_the_per_unit_kernel(lib, N):
    """vit_attention_split_pw<7> (G8 q | k | v, impl 3, more than 256 units) on 258 units; in the peaked class unit u leads at
    peaks[u % len(peaks)], so a K or V image left over from the unit a workgroup walked before gives a wrong answer.  Its container
    words equal those of vit_attention_split<7, true, true> (impl 5) on the same inputs."""
    row, errors = ROWS["split7x"], []
    for cls in CLASSES:
        case = _case(N, 64, cls, G8IN, False, PW_B)
        pw = _launch(lib, row, SPLIT, 3, case[0], G8IN, "split_pw<7>")
        errors += _held("split_pw<7>", SPLIT, 3, N, 64, cls, _read(pw, SPLIT), case)
        unit = _launch(lib, row, SPLIT, 5, case[0], G8IN, "split<7,true,true>")
        if not torch.equal(pw.view(torch.int32), unit.view(torch.int32)):
            errors.append(f"split_pw<7> and split<7,true,true> differ in bits: N {N} {cls}")
    assert not errors, errors
