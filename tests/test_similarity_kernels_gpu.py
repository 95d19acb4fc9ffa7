"""GPU: the caption-similarity kernels (csrc/similarity.hip) through the C ABI - cap_group_similarity, its workspace query and
cap_cosine_matrix - one call per width (D = 8, 100, 384) over the group sizes at which the tiling can go wrong: 0, 1, 2, 3, 63, 64, 65,
one below / at / above the accumulator's 32 rows (SIM_SUB) and the tile's 64 (SIM_TILE), a group of more than two tiles a side,
and the special groups of tests/_similarity_ref.py (near-duplicates whose variance cancels, an orthogonal and an antipodal pair,
rows of norm 1e3 and 1e-20, a zero row, two bit-identical rows), all with integer counts up to 5.

Expectations are float64 and every bound is derived in _similarity_ref.py from the kernels' summation order
(tests/test_similarity_ref_cpu.py holds a sequential fp32 implementation to them); nothing here is tuned to what the kernels give.
Every rounding test prints its worst error / bound (MEASURE) before it asserts; the figures are kept in
profiles/caption_similarity_gpu_tolerances.txt.

MEASURE figures on the MI355X (worst error / bound per width): see profiles/caption_similarity_gpu_tolerances.txt."""
import ctypes as C

import numpy as np
import pytest
import torch

import _similarity_ref as S

pytestmark = pytest.mark.gpu

FLOAT_OUTS = ("disagreement", "pair_mean", "pair_var")


@pytest.fixture(scope="module")
def lib():
    from embodied_captioning_amd import _native
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _native.load_library()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _guarded(n, dtype):
    """n owned elements and one sentinel element after them"""
    fill = float("nan") if dtype.is_floating_point else -77
    return torch.full((n + 1,), fill, dtype=dtype, device="cuda")


def _owned(t, n, what):
    h = t.cpu().numpy()
    tail = h[n]
    assert np.isnan(tail) if h.dtype.kind == "f" else tail == -77, f"{what}: written past its end"
    return h[:n].copy()


def group_call(lib, e, offsets, weights):
    """one cap_group_similarity call on host arrays -> dict of host arrays (every output checked for writes past its end)"""
    e = np.ascontiguousarray(e, dtype=np.float32)
    off = np.ascontiguousarray(offsets, dtype=np.int32)
    N, D, G = e.shape[0], e.shape[1], len(off) - 1
    need = lib.cap_group_similarity_workspace(N, G, D, off.ctypes.data_as(C.c_void_p))
    assert need > 0, lib.cap_last_error().decode()
    ed = _dev(e) if N else torch.empty((4,), dtype=torch.float32, device="cuda")
    wd = _dev(np.asarray(weights, dtype=np.float32)) if weights is not None else None
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda")        # a workspace that holds junk, not zeros
    o = dict(disagreement=_guarded(G, torch.float32), pair_mean=_guarded(G, torch.float32), pair_var=_guarded(G, torch.float32),
             pairs=_guarded(G, torch.int64), medoid=_guarded(G, torch.int32), row_mean=_guarded(N, torch.float32))
    rc = lib.cap_group_similarity(ed.data_ptr(), off.ctypes.data_as(C.c_void_p), wd.data_ptr() if wd is not None else None, N, G, D,
                                  o["disagreement"].data_ptr(), o["pair_mean"].data_ptr(), o["pair_var"].data_ptr(),
                                  o["pairs"].data_ptr(), o["medoid"].data_ptr(), o["row_mean"].data_ptr(), ws.data_ptr(),
                                  C.c_size_t(need), _stream())
    assert rc == 0, lib.cap_last_error().decode()
    torch.cuda.synchronize()
    assert ed.cpu().numpy()[:e.size].tobytes() == e.tobytes() if N else True, "the call changed its input"
    return {k: _owned(v, N if k == "row_mean" else G, k) for k, v in o.items()}


def matrix_call(lib, a, b, paired):
    Na, Nb, D = len(a), len(b), a.shape[1]
    ad, bd = _dev(a), _dev(b)
    n = Na if paired else Na * Nb
    out = _guarded(n, torch.float32)
    ws = torch.full((Na + Nb,), float("nan"), dtype=torch.float32, device="cuda")
    rc = lib.cap_cosine_matrix(ad.data_ptr(), bd.data_ptr(), Na, Nb, D, int(paired), out.data_ptr(), ws.data_ptr(),
                               C.c_size_t(4 * (Na + Nb)), _stream())
    assert rc == 0, lib.cap_last_error().decode()
    torch.cuda.synchronize()
    got = _owned(out, n, "cosine matrix")
    return got if paired else got.reshape(Na, Nb)


@pytest.fixture(scope="module", params=S.DIMS)
def main(request, lib):
    case = S.build_case(request.param)
    return case, S.reference(case), group_call(lib, case["e"], case["offsets"], case["weights"])


def _measure(what, worst):
    print(f"MEASURE {what} worst error / bound {worst:.3f}")


def test_every_output_is_within_its_bound_of_float64(main):
    case, ref, got = main
    off = case["offsets"]
    worst = dict.fromkeys(FLOAT_OUTS + ("row_mean",), 0.0)
    for g, r in enumerate(ref):
        for k in FLOAT_OUTS:
            worst[k] = max(worst[k], S.worst(got[k][g], r[k], r[k + "_bound"]))
        worst["row_mean"] = max(worst["row_mean"], S.worst(got["row_mean"][off[g]:off[g + 1]], r["row_mean"], r["row_mean_bound"]))
    for k, v in worst.items():
        _measure(f"D={case['D']} {k}", v)
    for g, (name, r) in enumerate(zip(case["names"], ref)):
        for k in FLOAT_OUTS:
            assert S.worst(got[k][g], r[k], r[k + "_bound"]) <= 1.0, (name, k, got[k][g], r[k], r[k + "_bound"])
        assert S.worst(got["row_mean"][off[g]:off[g + 1]], r["row_mean"], r["row_mean_bound"]) <= 1.0, (name, "row_mean")
        assert got["pairs"][g] == r["pairs"], name
        if r["medoid"] < 0:
            assert got["medoid"][g] == -1, name
        elif S.medoid_compared(name, r):
            assert got["medoid"][g] == off[g] + r["medoid"], name
        else:
            assert off[g] <= got["medoid"][g] < off[g + 1], name
    # the variance of the near-duplicates cancels: it is reported as a small non-negative number, never negative
    assert (got["pair_var"] >= 0).all()


def test_two_rows_of_the_same_bits_tie_and_the_first_wins(main):
    case, ref, got = main
    g = case["names"].index("tie")
    a = case["offsets"][g]
    assert got["row_mean"][a].tobytes() == got["row_mean"][a + 1].tobytes()
    assert got["medoid"][g] == a


def test_a_weighted_call_equals_the_expanded_call_within_the_bounds(main, lib):
    case, ref, got = main
    ex = S.expand_case(case)
    gx = group_call(lib, ex["e"], ex["offsets"], None)
    off, xoff = case["offsets"], ex["offsets"]
    first = np.concatenate([[0], np.cumsum(case["weights"].astype(np.int64))[:-1]])     # the first copy of every original row
    for g, (name, r) in enumerate(zip(case["names"], ref)):
        assert gx["pairs"][g] == got["pairs"][g] == r["pairs"], name
        for k in FLOAT_OUTS:                       # both calls are within the bound of one float64 value: twice the bound apart at most
            assert S.worst(gx[k][g], r[k], r[k + "_bound"]) <= 1.0, (name, k)
            assert abs(float(gx[k][g]) - float(got[k][g])) <= 2 * r[k + "_bound"], (name, k)
        rows = slice(off[g], off[g + 1])
        assert S.worst(gx["row_mean"][first[rows]], r["row_mean"], r["row_mean_bound"]) <= 1.0, name
        if r["medoid"] >= 0 and (S.medoid_compared(name, r) or name == "tie"):
            assert gx["medoid"][g] == first[off[g] + r["medoid"]], name
            assert xoff[g] <= gx["medoid"][g] < xoff[g + 1]


def test_a_group_has_the_same_bits_alone_first_last_and_between_other_groups(main, lib):
    case, ref, got = main
    off, e, w = case["offsets"], case["e"], case["weights"]
    names = case["names"]
    rng = np.random.default_rng(5)

    def filler(n):
        return rng.standard_normal((n, case["D"])).astype(np.float32), rng.integers(1, 6, size=n).astype(np.float32)

    for name in ("plain3", f"plain{S.SIM_TILE + 1}", f"plain{2 * S.SIM_TILE + 2}", "near_duplicates", "norms"):
        g = names.index(name)
        ge, gw = e[off[g]:off[g + 1]], w[off[g]:off[g + 1]]
        n = len(ge)
        want = {k: got[k][g] for k in FLOAT_OUTS + ("pairs",)}
        want_rows, want_medoid = got["row_mean"][off[g]:off[g + 1]], got["medoid"][g] - off[g]
        (f1, w1), (f2, w2) = filler(7), filler(S.SIM_TILE + 5)
        layouts = {"alone": ([ge], [gw], 0), "first": ([ge, f1, f2], [gw, w1, w2], 0), "last": ([f2, f1, ge], [w2, w1, gw], 2),
                   "between": ([f1, ge, f2], [w1, gw, w2], 1)}
        for where, (parts, wparts, at) in layouts.items():
            o = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int32)
            r = group_call(lib, np.concatenate(parts), o, np.concatenate(wparts))
            for k, v in want.items():
                assert r[k][at].tobytes() == v.tobytes(), (name, where, k)
            assert r["row_mean"][o[at]:o[at] + n].tobytes() == want_rows.tobytes(), (name, where, "row_mean")
            assert r["medoid"][at] - o[at] == want_medoid, (name, where, "medoid")


@pytest.mark.parametrize("D", S.DIMS)
def test_the_matrix_form_is_within_its_bound_and_the_paired_form_is_its_diagonal(lib, D):
    a, b, a2 = S.matrix_inputs(D)
    ref, bound = S.cosine64(a, b)
    got = matrix_call(lib, a, b, paired=False)
    _measure(f"D={D} cosine matrix", S.worst(got, ref, bound))
    assert S.worst(got, ref, bound) <= 1.0
    assert (got[1] == 0).all()                                   # the zero row: cosine 0 with everything
    full = matrix_call(lib, a2, b, paired=False)
    pair = matrix_call(lib, a2, b, paired=True)
    assert pair.tobytes() == np.ascontiguousarray(np.diag(full)).tobytes()
    ref2, bound2 = S.cosine64(a2, b)
    assert S.worst(pair, np.diag(ref2), np.diag(bound2)) <= 1.0
    # a group's pair statistics are those of this matrix: the mean over i < j of the matrix of a against itself
    sq = matrix_call(lib, a, a, paired=False).astype(np.float64)
    st = group_call(lib, a, [0, len(a)], None)
    iu = np.triu_indices(len(a), 1)
    r = S.group_stats64(a, np.ones(len(a)))                      # both are within their own bound of one float64 mean
    assert abs(st["pair_mean"][0] - sq[iu].mean()) <= r["pair_mean_bound"] + S.cosine64(a, a)[1][iu].mean()
    assert np.array_equal(sq, sq.T)                              # an entry depends on its two rows alone


def test_refusals_name_what_is_wrong(lib):
    e = torch.zeros((8, 8), dtype=torch.float32, device="cuda")
    out = torch.zeros((64,), dtype=torch.float32, device="cuda")
    i64 = torch.zeros((8,), dtype=torch.int64, device="cuda")
    i32 = torch.zeros((8,), dtype=torch.int32, device="cuda")
    ws = torch.zeros((1 << 16,), dtype=torch.uint8, device="cuda")

    def off(*v):
        a = np.asarray(v, dtype=np.int32)
        return a, a.ctypes.data_as(C.c_void_p)

    def refused(rc, *needles):
        msg = lib.cap_last_error().decode()
        assert rc != 0, "the call was accepted"
        for n in needles:
            assert n in msg, msg

    def group(offp, N=8, G=2, D=8, ep=e.data_ptr(), wsp=ws.data_ptr(), wsb=1 << 16, dis=out.data_ptr()):
        return lib.cap_group_similarity(ep, offp, None, N, G, D, dis, out.data_ptr(), out.data_ptr(), i64.data_ptr(), i32.data_ptr(),
                                        out.data_ptr(), wsp, C.c_size_t(wsb), _stream())

    good, goodp = off(0, 3, 8)
    assert group(goodp) == 0, lib.cap_last_error().decode()
    for bad, needle in (((1, 3, 8), "offsets do not start at 0"), ((0, 5, 3), "offsets decrease"), ((0, 3, 7), "offsets do not end at N")):
        keep, p = off(*bad)
        refused(group(p, N=8 if bad != (0, 5, 3) else 3), "cap_group_similarity", needle)
        assert lib.cap_group_similarity_workspace(8 if bad != (0, 5, 3) else 3, 2, 8, p) == 0
        assert needle in lib.cap_last_error().decode()
    refused(group(None), "cap_group_similarity", "null offsets")
    refused(group(goodp, D=6), "D % 4 != 0")
    refused(group(goodp, D=1028), "D > 1024")
    refused(group(goodp, N=-1), "negative counts")
    refused(group(goodp, G=-1), "negative counts")
    refused(group(goodp, ep=None), "null buffer")
    refused(group(goodp, wsp=None), "null buffer")
    refused(group(goodp, dis=None), "null buffer")
    need = lib.cap_group_similarity_workspace(8, 2, 8, goodp)
    assert need > 0
    refused(group(goodp, wsb=need - 1), "workspace too small")
    assert group(goodp, wsb=need) == 0

    def matrix(Na=8, Nb=8, D=8, paired=0, ap=e.data_ptr(), wsb=64, wsp=ws.data_ptr()):
        return lib.cap_cosine_matrix(ap, e.data_ptr(), Na, Nb, D, paired, out.data_ptr(), wsp, C.c_size_t(wsb), _stream())

    assert matrix() == 0, lib.cap_last_error().decode()
    refused(matrix(ap=None), "cap_cosine_matrix", "null buffer")
    refused(matrix(wsp=None), "null buffer")
    refused(matrix(D=6), "D % 4 != 0")
    refused(matrix(D=1028), "D > 1024")
    refused(matrix(Na=-1), "negative counts")
    refused(matrix(Na=4, paired=1), "paired needs Na == Nb")
    refused(matrix(wsb=63), "workspace too small")
    torch.cuda.synchronize()
