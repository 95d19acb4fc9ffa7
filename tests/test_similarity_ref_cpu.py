"""CPU: the reference and the bounds of tests/_similarity_ref.py stand on their own.  A sequential fp32 implementation that sums in
the kernels' order (csrc/similarity.hip: the lanes' fma chains, the butterfly, the MFMA's k order, a lane's 16 accumulator
registers, the 64-row chunks of the sum vector, fp64 above) is held to the derived bounds on the GPU file's own inputs; the
weighted closed forms are held to the literally expanded groups; the case list is checked to be what the GPU file relies on; and
the host helpers of the feature (`similarity.caption_groups`, `distributed.medoid_caption`) are tested."""
import numpy as np
import pytest

import _similarity_ref as S

F32, F64 = np.float32, np.float64


def fma32(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 values is exact in fp64"""
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


def wave_dot(x, y):
    """one wave per row: lane l owns the float4s at columns 4 l + 256 q; a chain per lane, then v += shfl_xor(v, o), o = 32 .. 1"""
    n, D = x.shape
    acc = np.zeros((n, 64), F32)
    for q in range(0, D, 256):
        for j in range(4):
            cols = np.arange(q + j, min(q + 256, D), 4)
            lanes = (cols - q) // 4
            acc[:, lanes] = fma32(x[:, cols], y[:, cols], acc[:, lanes])
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = (acc + acc[:, lane ^ o]).astype(F32)
    return acc[:, 0]


def normalise32(e):
    ss = wave_dot(e, e)
    inv = (F32(1.0) / np.maximum(np.sqrt(ss, dtype=F32), F32(1e-12))).astype(F32)
    return (e * inv[:, None]).astype(F32)


def gram32(ah, bh):
    """the MFMA's chain: k-step ks takes the pairs (8 ks + j, 8 ks + 4 + j), j = 0 .. 3"""
    D = ah.shape[1]
    s = np.zeros((ah.shape[0], bh.shape[0]), F32)
    for ks in range(0, D, 8):
        for j in range(4):
            for k in (ks + j, ks + 4 + j):
                if k < D:
                    s = fma32(ah[:, k, None], bh[None, :, k], s)
    return s


def group32(e, w):
    n, D = e.shape
    T = S.SIM_TILE
    out = dict(row_mean=np.zeros(n, F32))
    if n == 0:
        out.update(disagreement=F32(0), pair_mean=F32(0), pair_var=F32(0), pairs=0, medoid=-1)
        return out
    eh = normalise32(e)
    W = float(w.astype(F64).sum())
    m64 = np.zeros(D, F64)
    for c in range(0, n, T):
        acc = np.zeros(D, F32)
        for j in range(c, min(c + T, n)):
            acc = fma32(w[j], eh[j], acc)
        m64 += acc.astype(F64)
    m = m64.astype(F32)
    if W > 1:
        t, sii = wave_dot(eh, np.broadcast_to(m, eh.shape)), wave_dot(eh, eh)
        out["row_mean"] = ((t.astype(F64) - sii.astype(F64)) / (W - 1)).astype(F32)
    out["medoid"] = int(np.argmax(out["row_mean"]))
    mm = (m.astype(F64) ** 2).sum()
    out["disagreement"] = F32(1.0 - mm / (W * W))
    s = gram32(eh, eh)
    pw = S._pair_weights(w.astype(F64)).astype(F32)
    nt = -(-n // T)
    sp = np.zeros((nt * T, nt * T), F32)
    wp = np.zeros_like(sp)
    sp[:n, :n] = s
    wp[:n, :n] = pw                                       # zero below the diagonal and outside the group
    s1 = s2 = 0.0
    for ti in range(nt):
        for tj in range(ti, nt):
            sb = sp[ti * T:(ti + 1) * T, tj * T:(tj + 1) * T].reshape(2, 4, 2, 4, T)      # row = 32 si + 8 e_hi + 4 hh + e_lo
            wb = wp[ti * T:(ti + 1) * T, tj * T:(tj + 1) * T].reshape(2, 4, 2, 4, T)
            p1 = np.zeros((2, 2, T), F32)
            p2 = np.zeros((2, 2, T), F32)
            for eh_ in range(4):
                for el in range(4):
                    sv, wv = sb[:, eh_, :, el, :], wb[:, eh_, :, el, :]
                    p1 = fma32(wv, sv, p1)
                    p2 = fma32((wv * sv).astype(F32), sv, p2)
            s1 += p1.astype(F64).sum()
            s2 += p2.astype(F64).sum()
    npairs = W * (W - 1) / 2
    out["pairs"] = int(npairs)
    mean = s1 / npairs if npairs else 0.0
    out["pair_mean"] = F32(mean)
    out["pair_var"] = F32(max(0.0, s2 / npairs - mean * mean) if npairs else 0.0)
    return out


@pytest.fixture(scope="module", params=S.DIMS)
def case(request):
    c = S.build_case(request.param)
    return c, S.reference(c)


def test_fp32_in_the_kernels_order_is_inside_the_bounds(case):
    c, ref = case
    off = c["offsets"]
    for g, (name, r) in enumerate(zip(c["names"], ref)):
        a, b = int(off[g]), int(off[g + 1])
        got = group32(c["e"][a:b], c["weights"][a:b])
        for k in ("disagreement", "pair_mean", "pair_var", "row_mean"):
            assert S.worst(got[k], r[k], r[k + "_bound"]) <= 1.0, (name, k, got[k], r[k], r[k + "_bound"])
        assert got["pairs"] == r["pairs"]
        if S.medoid_compared(name, r):
            assert got["medoid"] == r["medoid"], name
        if name == "tie":
            assert got["medoid"] == 0 and got["row_mean"][0] == got["row_mean"][1]


def test_weighted_forms_equal_the_literally_expanded_group(case):
    c, ref = case
    off, w = c["offsets"], c["weights"]
    for g, (name, r) in enumerate(zip(c["names"], ref)):
        a, b = int(off[g]), int(off[g + 1])
        x = S.expanded_stats64(c["e"][a:b], w[a:b])
        for k in ("disagreement", "pair_mean", "pair_var"):
            assert abs(x[k] - r[k]) < 1e-12, (name, k)
        assert x["pairs"] == r["pairs"]
        assert np.abs(x["row_mean"] - r["row_mean"]).max(initial=0.0) < 1e-12, name
        if S.medoid_compared(name, r):
            assert x["medoid"] == r["medoid"], name


def test_the_case_list_is_what_the_gpu_file_relies_on(case):
    c, ref = case
    sizes = np.diff(c["offsets"]).tolist()
    T, B = S.SIM_TILE, S.SIM_SUB
    for n in (0, 1, 2, 3, 63, 64, 65, B - 1, B, B + 1, T - 1, T, T + 1):
        assert n in sizes
    assert max(sizes) > 2 * T                                           # a group that spans three tiles a side
    assert c["weights"].min() >= 1 and c["weights"].max() == 5 and (c["weights"] == np.round(c["weights"])).all()
    by = dict(zip(c["names"], range(len(sizes))))
    e, off = c["e"].astype(np.float64), c["offsets"]
    grp = lambda n: e[off[by[n]]:off[by[n] + 1]]  # noqa: E731
    s, _ = S.cosine64(grp("near_duplicates"), grp("near_duplicates"))
    assert (np.abs(1 - s) < 1e-6).all() and ref[by["near_duplicates"]]["pair_var"] < 1e-12
    assert abs(S.cosine64(grp("orthogonal"), grp("orthogonal"))[0][0, 1]) < 1e-7
    assert abs(S.cosine64(grp("antipodal"), grp("antipodal"))[0][0, 1] + 1) < 1e-7
    norms = np.linalg.norm(grp("norms"), axis=1)
    assert abs(norms[0] - 1e3) < 1 and norms[1] < 2e-20
    assert (np.linalg.norm(grp("zero_row"), axis=1) == 0).sum() == 1
    t = c["e"][off[by["tie"]]:off[by["tie"] + 1]]
    assert t[0].tobytes() == t[1].tobytes() and ref[by["tie"]]["medoid"] == 0
    # the medoid is compared on every group but the named exceptions and the tie: their two best row means are four bounds apart
    for name, r in zip(c["names"], ref):
        if name not in S.MEDOID_EXEMPT and name != "tie" and r["medoid"] >= 0:
            assert S.medoid_compared(name, r), (name, r["gap"], np.max(r["row_mean_bound"]))
    # a zero row has cosine 0 with everything, itself included
    z = np.flatnonzero(np.linalg.norm(grp("zero_row"), axis=1) == 0)[0]
    assert (S.cosine64(grp("zero_row"), grp("zero_row"))[0][z] == 0).all()


@pytest.mark.parametrize("D", S.DIMS)
def test_matrix_form_in_the_kernels_order_is_inside_its_bound(D):
    a, b, a2 = S.matrix_inputs(D)
    ref, bound = S.cosine64(a, b)
    got = gram32(normalise32(a), normalise32(b))
    assert S.worst(got, ref, bound) <= 1.0
    assert a2.shape == b.shape


def test_bounds_are_of_the_order_of_the_chain_lengths():
    # D = 384: a 384-link chain and two normalised factors - a few 1e-5, not a tolerance wide enough to hide a wrong pair
    assert 2e-5 < S.s_bound(1.0, 1.0, 384) < 3e-5 and S.s_bound(1.0, 1.0, 8) < 3e-6
    assert S.dot_roundings(384) == 14 and S.dot_roundings(1024) == 22


def test_caption_groups_distinct_captions_counts_offsets_and_empty_groups():
    from embodied_captioning_amd.distributed import captions_frequency
    from embodied_captioning_amd.similarity import caption_groups
    freq = captions_frequency({(0, 1): ["a red chair", "a chair", "a red chair", "a red chair"], (0, 2): [], (3, 4): ["a lamp"]})
    keys, sentences, offsets, weights = caption_groups(freq)
    assert keys == [(0, 1), (0, 2), (3, 4)]
    assert sentences == ["a red chair", "a chair", "a lamp"]
    assert offsets == [0, 2, 2, 3] and weights == [3, 1, 1]
    # a caption listed twice in one group is one row with the summed count; the same caption in two groups is two rows
    keys, sentences, offsets, weights = caption_groups({"a": [[2, "x"], [1, "y"], [4, "x"]], "b": [[1, "x"]]})
    assert sentences == ["x", "y", "x"] and weights == [6, 1, 1] and offsets == [0, 2, 3]
    assert caption_groups({}) == ([], [], [0], [])
    with pytest.raises(ValueError):
        caption_groups({"a": [[0, "x"]]})


def test_medoid_caption_takes_the_largest_row_mean_and_the_first_on_ties():
    from embodied_captioning_amd.distributed import consensus_caption, medoid_caption
    fl = [[1, "a"], [5, "b"], [1, "c"]]
    assert medoid_caption(fl, [0.2, 0.1, 0.9]) == "c"
    assert medoid_caption(fl, [0.5, 0.5, 0.5]) == "a"
    assert medoid_caption(fl, [0.1, 0.7, 0.7]) == "b"
    assert medoid_caption(fl[:1], [0.0]) == "a"
    assert consensus_caption(fl) == "b"                  # the frequency rule is untouched
    with pytest.raises(ValueError):
        medoid_caption(fl, [0.1, 0.2])
    with pytest.raises(ValueError):
        medoid_caption([], [])


def test_caption_consistency_csv_groups_rows_and_averages_the_groups_that_have_a_pair(tmp_path):
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("caption_consistency_csv", os.path.join(os.path.dirname(S._SRC), "..", "..", "tools",
                                                                                          "caption_consistency_csv.py"))
    T = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(T)
    src = tmp_path / "caps.csv"
    src.write_text('episode_id,object_id,caption\n0,1,"a red, chair"\n0,1,a chair\n0,2,a lamp\n3,1,a shelf\n3,1,a shelf\n')
    grouped = T.read_groups(str(src))
    assert grouped == {("0", "1"): ["a red, chair", "a chair"], ("0", "2"): ["a lamp"], ("3", "1"): ["a shelf", "a shelf"]}

    class Stub:
        def caption_statistics(self, freq):
            assert not freq or freq[("3", "1")] == [[2, "a shelf"]]
            means = {("0", "1"): 0.25, ("0", "2"): 0.0, ("3", "1"): 0.75}
            return {k: dict(pairs=sum(n for n, _ in v) * (sum(n for n, _ in v) - 1) // 2, mean=means[k], std=0.0, disagreement=0.1,
                            medoid_caption=v[0][1]) for k, v in freq.items()}

    rows, overall = T.consistency(grouped, Stub())
    assert [r[:4] for r in rows] == [("0", "1", 2, 1), ("0", "2", 1, 0), ("3", "1", 2, 1)] and overall == 0.5
    out = tmp_path / "out.csv"
    T.write_csv(str(out), rows, overall)
    lines = out.read_text().splitlines()
    assert lines[0].startswith("episode_id,object_id,captions,pairs,mean_cosine") and lines[-1] == "overall,,2,,0.5,,,"
    assert T.consistency({}, Stub()) == ([], None)
