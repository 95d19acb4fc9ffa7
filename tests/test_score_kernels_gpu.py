"""GPU: the two kernels of caption scoring alone.  target_logprob - the head consumer (csrc/elementwise.hip, target_logprob_kernel) through cap_op_target_logprob: per
live row the log-softmax at a GIVEN id, log max softmax and the arg-max, against float64 on the same fp32 logits.

Bar (per value), that of tests/test_logprob_kernel_gpu.py: the larger of 8 x the maximal error of torch float32 on the CPU
(`log_softmax`) against float64 over the same rows, and 4 spacings of fp32 at the value's magnitude.  The arg-max is exact
(lowest index among equal maxima).  The padding columns between V and ld hold a large finite value that must never be read.
Run with -s for the table of reference error, bar and kernel error per shape."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS = (1, 5, 67)
VOCABS = (7, 512, 30524, 50272)
BIG = 3.0e38
KINDS = ("first", "last", "max", "tie2", "dead")


def _p(t):
    return C.c_void_p(t.data_ptr())


def _run(rows, ld, targets, live):
    """rows fp32 [n, V] host -> (target log-prob, top log-prob, top id) host tensors [n] of one launch over [n, ld] device rows."""
    from embodied_captioning_amd import _native
    lib = _native.load_library()
    n, V = rows.shape
    buf = torch.full((n, ld), BIG, dtype=torch.float32)
    buf[:, :V] = rows
    dev = buf.cuda()
    tg = torch.tensor(targets, dtype=torch.int32, device="cuda")
    lv = torch.tensor(live, dtype=torch.int32, device="cuda")
    tlp = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
    top = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
    tid = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    rc = lib.cap_op_target_logprob(_p(dev), ld, V, n, _p(tg), _p(lv), _p(tlp), _p(top), _p(tid),
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, _native.last_error()
    torch.cuda.synchronize()
    return tlp.cpu(), top.cpu(), tid.cpu()


def _bar(want, ref_err):
    return np.maximum(8.0 * ref_err, 4.0 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64))


def _case(V, R, shift, seed):
    """R rows whose kind cycles through KINDS from `shift`: the target at column 0, at column V - 1, at the maximum, at the second
    of two equal maxima (the arg-max is the first), and a dead row (NaN logits, never read)."""
    g = torch.Generator().manual_seed(seed)
    rows = torch.randn((R, V), generator=g, dtype=torch.float32) * 2.0
    targets, live, kinds = [], [], []
    for r in range(R):
        kind = KINDS[(r + shift) % len(KINDS)]
        kinds.append(kind)
        live.append(0 if kind == "dead" else 1)
        if kind == "first":
            targets.append(0)
        elif kind == "last":
            targets.append(V - 1)
        elif kind == "max":
            targets.append(int(rows[r].argmax()))
        elif kind == "tie2":
            i, k = sorted(int(x) for x in torch.randperm(V, generator=g)[:2])
            rows[r, i] = rows[r, k] = rows[r].max() + 0.75
            targets.append(k)
        else:
            rows[r] = float("nan")
            targets.append(V // 2)
    return rows, targets, live, kinds


@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("V", VOCABS)
def test_target_logprob_against_float64(V, R):
    ld = (V + 3) & ~3
    worst = worst_top = ref_worst = 0.0
    for shift in range(len(KINDS)):
        rows, targets, live, kinds = _case(V, R, shift, 5000 + 31 * V + 7 * R + shift)
        tlp, top, tid = _run(rows, ld, targets, live)
        on = [r for r in range(R) if live[r]]
        for r in range(R):
            if not live[r]:
                assert float(tlp[r]) == 0.0 and float(top[r]) == 0.0 and int(tid[r]) == 0, (V, R, r)
        if not on:
            continue
        x = rows[on]
        t = torch.tensor([targets[r] for r in on])
        want_all = torch.log_softmax(x.double(), dim=-1)
        ref_all = torch.log_softmax(x, dim=-1).double()
        want = want_all.gather(1, t[:, None])[:, 0].numpy()
        ref_err = float(np.abs(ref_all.gather(1, t[:, None])[:, 0].numpy() - want).max())
        want_top = want_all.max(dim=-1).values.numpy()
        ref_err_top = float(np.abs(ref_all.max(dim=-1).values.numpy() - want_top).max())
        bar, bar_top = _bar(want, ref_err), _bar(want_top, ref_err_top)
        amax = np.argmax(x.numpy(), axis=1)                       # the first maximal index
        for k, r in enumerate(on):
            assert int(tid[r]) == int(amax[k]), (V, R, r, kinds[r], int(tid[r]), int(amax[k]))
            if kinds[r] == "tie2":
                assert int(tid[r]) < targets[r] and rows[r, int(tid[r])] == rows[r, targets[r]]
            if kinds[r] in ("max", "tie2"):
                assert float(tlp[r]) == float(top[r]), (V, R, r, kinds[r])          # z_target - z_max is an exact 0
            err, err_top = abs(float(tlp[r]) - want[k]), abs(float(top[r]) - want_top[k])
            worst, worst_top, ref_worst = max(worst, err / bar[k]), max(worst_top, err_top / bar_top[k]), max(ref_worst, ref_err)
            assert err <= bar[k], (V, R, r, kinds[r], float(tlp[r]), want[k], bar[k])
            assert err_top <= bar_top[k], (V, R, r, kinds[r], float(top[r]), want_top[k], bar_top[k])
    print(f"target_logprob V={V:6d} R={R:2d} ref_err_fp32_max={ref_worst:.3e} target_err_over_bar_max={worst:.3f} "
          f"top_err_over_bar_max={worst_top:.3f}")


@pytest.mark.parametrize("V", (7, 30524))
def test_value_does_not_depend_on_the_rows_position_or_its_neighbours(V):
    g = torch.Generator().manual_seed(6000 + V)
    row = torch.randn((1, V), generator=g, dtype=torch.float32) * 2.0
    others = torch.randn((67, V), generator=g, dtype=torch.float32) * 2.0
    ld = ((V + 3) & ~3) + 4                                      # a wider leading dimension: more padding never read
    tgt = V - 2
    a = _run(row, ld, [tgt], [1])
    for pos in (0, 33, 66):
        x = others.clone()
        x[pos] = row[0]
        live = [1] * 67
        live[(pos + 1) % 67] = 0
        b = _run(x, ld, [tgt] * 67, live)
        for u, v in zip(a, b):
            assert torch.equal(u, v[pos:pos + 1]), (V, pos)


def test_refusals():
    from embodied_captioning_amd import _native
    lib = _native.load_library()
    x = torch.zeros((2, 8), dtype=torch.float32, device="cuda")
    i = torch.zeros(2, dtype=torch.int32, device="cuda")
    f = torch.zeros(2, dtype=torch.float32, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.cap_op_target_logprob(_p(x), 6, 6, 2, _p(i), _p(i), _p(f), _p(f), _p(i), s) != 0          # ld % 4
    assert "ld" in _native.last_error()
    assert lib.cap_op_target_logprob(_p(x), 8, 9, 2, _p(i), _p(i), _p(f), _p(f), _p(i), s) != 0          # ld < V
    assert lib.cap_op_target_logprob(_p(x), 8, 7, 2, None, _p(i), _p(f), _p(f), _p(i), s) != 0           # null buffer
    assert "null" in _native.last_error()


# ================================================================================================ opt_prefix_attention
# cap_op_opt_prefix_attention alone (csrc/attention.hip): n new positions per caption behind an image's cached prefix of P keys, against
# the same formula in float64.  Bars, those of tests/test_attention_kernels_gpu.py, derived from the reference and never from the kernel:
#   fp32 out  8 x ref_err_fp32 (the formula in torch float32 on the CPU against float64; where that is 0, one fp32 spacing of the
#             largest reference value stands in);  bf16 out  elementwise |out - ref| <= 2^-8 |ref| + the fp32 bar.
# Families: randn, and peaked with the peak (~20 units above the rest) on the first prefix key, the last prefix key, the caption's first
# own key and the row's own position - the two sides of the boundary between the two key sources.
PA_B, PA_H = 2, 2
CANARY = 77.0


def _pa_problem(hd, P, n, Cn, family, bf16, seed):
    g = torch.Generator().manual_seed(seed)
    N, T = PA_B * Cn, PA_H * hd
    amp = 1.0 if family == "randn" else 0.3
    q = torch.randn((N, n, PA_H, hd), generator=g) * amp
    k = torch.randn((N, n, PA_H, hd), generator=g) * amp
    v = torch.randn((N, n, PA_H, hd), generator=g)
    pk = torch.randn((PA_B, P, PA_H, hd), generator=g) * amp
    pv = torch.randn((PA_B, P, PA_H, hd), generator=g)
    if family != "randn":
        s = math.sqrt(20.0 * math.sqrt(hd))                        # s * s / sqrt(hd) = 20
        u = torch.nn.functional.normalize(torch.randn((n, PA_H, hd), generator=g), dim=-1)
        if family == "own":
            q += s * u[None]
            k += s * u[None]                                       # position t's own key leads for the query of position t
        else:
            q += s * u[0][None, None]
            if family == "prefix_first":
                pk[:, 0] += s * u[0]
            elif family == "prefix_last":
                pk[:, P - 1] += s * u[0]
            else:                                                  # cap_first
                k[:, 0] += s * u[0]
    if bf16:
        q, k, v, pk, pv = (x.bfloat16().float() for x in (q, k, v, pk, pv))
    n_pos = torch.tensor([(n, max(n - 1, 0), 0, n // 2, n, 1)[i % 6] for i in range(N)], dtype=torch.int32)      # ragged, an absent slot
    if N > 1:
        n_pos[1 if n_pos[0] == n else 0] = 0
    return q, k, v, pk, pv, n_pos


def _pa_reference(q, k, v, pk, pv, Cn, dt):
    N, n, H, hd = q.shape
    P = pk.shape[1]
    img = torch.arange(N) // Cn
    keys = torch.cat([pk[img], k], 1).to(dt)                       # [N, P + n, H, hd]
    vals = torch.cat([pv[img], v], 1).to(dt)
    sc = torch.einsum("nthd,njhd->nhtj", q.to(dt), keys) / math.sqrt(hd)
    mask = torch.arange(P + n)[None, :] > (P + torch.arange(n))[:, None]
    sc = sc.masked_fill(mask[None, None], float("-inf"))
    return torch.einsum("nhtj,njhd->nthd", torch.softmax(sc, -1), vals).reshape(N, n, H * hd)



@pytest.mark.parametrize("n", (1, 2, 17, 31))
@pytest.mark.parametrize("P", (1, 9, 33))
@pytest.mark.parametrize("hd", (16, 64, 80, 128))
@pytest.mark.parametrize("dtype", ("f32", "bf16"))
def test_opt_prefix_attention_against_float64(dtype, hd, P, n):
    from embodied_captioning_amd import _native
    lib = _native.load_library()
    bf16 = dtype == "bf16"
    tdt = torch.bfloat16 if bf16 else torch.float32
    T, Lmax = PA_H * hd, P + n + 3
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    worst = 0.0
    for Cn in (1, 3):
        N = PA_B * Cn
        for family in ("randn", "prefix_first", "prefix_last", "cap_first", "own"):
            q, k, v, pk, pv, n_pos = _pa_problem(hd, P, n, Cn, family, bf16, 7000 + 13 * hd + 5 * P + n + Cn)
            ref = _pa_reference(q, k, v, pk, pv, Cn, torch.float64)
            err32 = float((_pa_reference(q, k, v, pk, pv, Cn, torch.float32).double() - ref).abs().max())
            bar = 8.0 * (err32 if err32 > 0 else float(np.spacing(np.float32(ref.abs().max()))))
            qkv = torch.cat([q.reshape(N * n, T), k.reshape(N * n, T), v.reshape(N * n, T)], 1).to(tdt).cuda()
            kc = torch.full((PA_B, Lmax, T), float("nan"), dtype=tdt)      # positions behind the prefix are never read
            vc = kc.clone()
            kc[:, :P], vc[:, :P] = pk.reshape(PA_B, P, T).to(tdt), pv.reshape(PA_B, P, T).to(tdt)
            kc, vc, npd = kc.cuda(), vc.cuda(), n_pos.cuda()
            out = torch.full((N * n, T), CANARY, dtype=tdt, device="cuda")
            rc = lib.cap_op_opt_prefix_attention(int(bf16), _p(qkv), _p(kc), _p(vc), _p(out), N, n, 0, Cn, _p(npd), T, PA_H, Lmax, P, stream)
            assert rc == 0, _native.last_error()
            torch.cuda.synchronize()
            got = out.float().cpu().reshape(N, n, T)
            keep = torch.arange(n)[None, :] < n_pos[:, None].long()
            assert bool((got[~keep] == CANARY).all()), (dtype, hd, P, n, Cn, family)            # rows behind a caption's end are left alone
            assert torch.isfinite(got[keep]).all()
            diff = (got[keep].double() - ref[keep]).abs()
            judged = float((diff - (2.0 ** -8 * ref[keep].abs() if bf16 else 0.0)).max()) if keep.any() else 0.0
            worst = max(worst, judged / bar)
            assert judged <= bar, (dtype, hd, P, n, Cn, family, judged, bar, err32)
            if Cn == 3:      # the captions from the 4th on as a pass of their own (cap0 = 3: image 1's), and without lengths: same bits
                out2 = torch.full((N * n, T), CANARY, dtype=tdt, device="cuda")
                rc = lib.cap_op_opt_prefix_attention(int(bf16), _p(qkv[3 * n:]), _p(kc), _p(vc), _p(out2[3 * n:]), N - 3, n, 3, Cn, None, T, PA_H,
                                                     Lmax, P, stream)
                assert rc == 0, _native.last_error()
                torch.cuda.synchronize()
                got2 = out2.float().cpu().reshape(N, n, T)
                assert torch.equal(got2[3:][keep[3:]], got[3:][keep[3:]]) and bool((got2[:3] == CANARY).all())
                assert float((got2[3:].double() - ref[3:]).abs().max()) <= bar + (2.0 ** -8 * float(ref[3:].abs().max()) if bf16 else 0.0)
    print(f"opt_prefix_attention {dtype} hd={hd:3d} P={P:2d} n={n:2d}: worst judged / bar {worst:.3f}")


def _same_bits(a, b):
    it = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


# The two kernels share one walk (opt_decode_attention_body) and differ in where key j is read from, so row (caption, t) of a prefix pass
# must have the BITS of decode step past = P + t of a row whose cache holds the image's prompt and the caption's earlier keys: two
# images x two captions each (caption index != image index), the runtime head width (16) and the unrolled one (80: HD8 = 10), and
# (P, n) with 1 key, a few, and 61 .. 68 keys - across the lanes' 64-key trip of the score loop and several 16-key trips of P.V, with
# the boundary between the two key sources beside it.  dtype codes: 0 fp32, 1 bf16, 2 split (fp32 in, G8 out: an fp32-sized container).
@pytest.mark.parametrize("P,n", ((1, 1), (9, 5), (60, 8)))
@pytest.mark.parametrize("hd", (16, 80))
@pytest.mark.parametrize("dtype", (0, 1, 2), ids=("f32", "bf16", "f32s"))
def test_opt_prefix_attention_rows_have_the_bits_of_the_decode_steps(dtype, hd, P, n):
    from embodied_captioning_amd import _native
    lib = _native.load_library()
    Cn, N, T, Lmax = 2, PA_B * 2, PA_H * hd, P + n + 2
    it = torch.bfloat16 if dtype == 1 else torch.float32
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator().manual_seed(9000 + 97 * hd + 7 * P + n)
    qkv = (torch.randn((N, n, 3 * T), generator=g) * 1.5).to(it).cuda()          # caption-major rows of the pass
    pk, pv = ((torch.randn((PA_B, P, T), generator=g) * 1.5).to(it).cuda() for _ in range(2))
    img = torch.arange(N, device="cuda") // Cn

    def caches(rows, prompt):      # [rows, Lmax, T]: the prompt, and NaN wherever nothing is stored
        c = torch.full((rows, Lmax, T), float("nan"), dtype=it, device="cuda")
        c[:, :P] = prompt
        return c

    kci, vci = caches(PA_B, pk), caches(PA_B, pv)                                # per image, read only
    out_p = torch.full((N, n, T), float("nan"), dtype=it if dtype == 1 else torch.float32, device="cuda")
    rc = lib.cap_op_opt_prefix_attention(dtype, _p(qkv), _p(kci), _p(vci), _p(out_p), N, n, 0, Cn, None, T, PA_H, Lmax, P, stream)
    assert rc == 0, _native.last_error()
    kc, vc = caches(N, pk[img]), caches(N, pv[img])                              # per caption, appended to by the steps
    for t in range(n):
        row = qkv[:, t].contiguous()
        out_t = torch.full((N, T), float("nan"), dtype=out_p.dtype, device="cuda")
        rc = lib.cap_op_opt_decode_attention(dtype, _p(row), _p(kc), _p(vc), _p(out_t), N, T, PA_H, Lmax, P + t, stream)
        assert rc == 0, _native.last_error()
        torch.cuda.synchronize()
        assert _same_bits(out_t, out_p[:, t]), (dtype, hd, P, n, t)
    if dtype == 2:
        from _util import g8_decode
        assert np.isfinite(g8_decode(out_p.cpu().numpy())).all()
    else:
        assert torch.isfinite(out_p.float()).all()                               # every row was written, and from keys that exist
    assert _same_bits(kc[:, P:P + n], qkv[:, :, T:2 * T]) and _same_bits(vc[:, P:P + n], qkv[:, :, 2 * T:])
    assert _same_bits(kc[:, :P], pk[img]) and _same_bits(vc[:, :P], pv[img])
    assert torch.isnan(kc[:, P + n:]).all() and torch.isnan(kci[:, P:]).all() and torch.isnan(vci[:, P:]).all()


def test_opt_prefix_attention_refusals():
    from embodied_captioning_amd import _native
    lib = _native.load_library()
    x = torch.zeros((4, 3 * 32), device="cuda")
    c = torch.zeros((1, 8, 32), device="cuda")
    o = torch.zeros((4, 32), device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.cap_op_opt_prefix_attention(0, _p(x), _p(c), _p(c), _p(o), 2, 2, 0, 1, None, 32, 4, 8, 9, s) != 0       # prefix beyond Lmax
    assert "opt_prefix_attention" in _native.last_error()
    assert lib.cap_op_opt_prefix_attention(0, _p(x), _p(c), _p(c), _p(o), 2, 2, 0, 1, None, 32, 8, 8, 4, s) != 0       # head_dim 4
    assert lib.cap_op_opt_prefix_attention(0, _p(x), None, _p(c), _p(o), 2, 2, 0, 1, None, 32, 4, 8, 4, s) != 0        # null cache
