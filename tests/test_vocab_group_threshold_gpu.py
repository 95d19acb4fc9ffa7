"""GPU: the group step of the probability fusion (csrc/elementwise.hip, vocab_group_threshold_kernel) through
cap_op_vocab_group_threshold: per CSR group of accumulator rows the fp32 mean in listed order, the tokens above th in ascending
order, their means and their full count - against float64 (tests/_fusion_ref.py).

Threshold condition: the kept set and its order equal float64's for every token whose float64 mean is more than 4 fp32 spacings of
th away from th.  The inputs are built so that NO mean falls inside that band (asserted on the CPU before the launch), so the kept
set must be float64's exactly.  A dyadic case with power-of-two group sizes, where fp32 is exact, holds one mean equal to th."""
import ctypes as C

import numpy as np
import pytest
import torch

from _fusion_ref import assert_no_mean_in_band, group_mean64, kept64, spacing32, threshold_band

pytestmark = pytest.mark.gpu

N = 17
VOCABS = (5, 255, 1027, 4099, 50272)
# sizes 1, 2, 3, 7, 4 over a permuted, non-contiguous row order, and one empty group (in the middle)
GROUPS = [[11], [3, 16], [8, 0, 13], [], [5, 14, 1, 10, 7, 15, 2], [12, 4, 9, 6]]
ID_SENTINEL, PROB_SENTINEL, COUNT_SENTINEL = -9, -1.0, -3


def _p(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def _run(acc_dev, V, groups, th, K, n_rows=N, rows=None, off=None, expect_ok=True):
    from embodied_captioning_amd import _native
    from embodied_captioning_amd.engine import vocab_group_csr
    lib = _native.load_library()
    if rows is None:
        rows, off = vocab_group_csr(groups, n_rows)
    G = off.numel() - 1
    rows_d, off_d = rows.cuda(), off.cuda()
    ids = torch.full((G, K if K > 0 else 1), ID_SENTINEL, dtype=torch.int32, device="cuda")
    probs = torch.full((G, K if K > 0 else 1), PROB_SENTINEL, dtype=torch.float32, device="cuda")
    counts = torch.full((G,), COUNT_SENTINEL, dtype=torch.int32, device="cuda")
    rc = lib.cap_op_vocab_group_threshold(_p(acc_dev), acc_dev.shape[1], V, n_rows, _p(rows_d), rows.numel(), _p(off_d), G,
                                          C.c_float(th), K, _p(ids), _p(probs), _p(counts),
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    if not expect_ok:
        assert rc != 0
        assert bool((ids == ID_SENTINEL).all()) and bool((counts == COUNT_SENTINEL).all())      # refused before any launch
        return _native.last_error()
    assert rc == 0, _native.last_error()
    return ids.cpu(), probs.cpu(), counts.cpu()


def _inputs(V, th):
    """fp32 [N, acc_ld] (BIG-like sentinel 9.0 in the padding columns: a mean that read them would exceed every th) and the float64
    means per group, with every mean farther than the band from th."""
    g = torch.Generator().manual_seed(8000 + V)
    acc_ld = (V + 3) // 4 * 4 + 4
    acc = torch.full((N, acc_ld), 9.0, dtype=torch.float32)
    acc[:, :V] = torch.rand((N, V), generator=g) * 0.2
    n_hot = min(10, max(1, V // 2))
    for members in GROUPS:
        if members:
            hot = torch.randperm(V, generator=g)[:n_hot]
            vals = 0.3 + 0.7 * torch.rand((len(members), n_hot), generator=g)
            for j, r in enumerate(members):
                acc[r, hot] = vals[j]
    fth = float(np.float32(th))
    a64 = acc[:, :V].double().numpy()
    for members in GROUPS:                                   # move a mean that fell into the band well out of it
        if members:
            m = group_mean64(a64, members)
            for i in np.nonzero(np.abs(m - fth) <= 2 * threshold_band(th))[0]:
                acc[members[0], i] = 0.0
                a64[members[0], i] = 0.0
    means = [group_mean64(a64, m) if m else None for m in GROUPS]
    margin = min(assert_no_mean_in_band(m, th) for m in means if m is not None)
    return acc, means, margin


@pytest.mark.parametrize("th", (0.25, 0.5))
@pytest.mark.parametrize("V", VOCABS)
def test_kept_set_order_means_and_counts_against_float64(V, th):
    acc, means, margin = _inputs(V, th)
    dev = acc.cuda()
    K = 16
    ids, probs, counts = _run(dev, V, GROUPS, th, K)
    worst, kept_total = 0.0, 0
    for g, members in enumerate(GROUPS):
        if not members:
            assert int(counts[g]) == 0 and bool((ids[g] == ID_SENTINEL).all()) and bool((probs[g] == PROB_SENTINEL).all())
            continue
        want = kept64(means[g], th)
        c = int(counts[g])
        assert c == len(want) and c <= K, (V, th, g, c, len(want))
        assert ids[g, :c].tolist() == want.tolist()                                  # the same set, ascending
        err = np.abs(probs[g, :c].double().numpy() - means[g][want])
        bar = 4.0 * spacing32(means[g][want])
        worst = max(worst, float((err / bar).max()))
        assert (err <= bar).all(), (V, th, g, err, bar)
        assert bool((ids[g, c:] == ID_SENTINEL).all()) and bool((probs[g, c:] == PROB_SENTINEL).all())
        kept_total += c
    assert kept_total > 0
    print(f"vocab_group_threshold V={V:6d} th={th} kept={kept_total:3d} margin_to_th={margin:.3e} (band {threshold_band(th):.3e}) "
          f"mean_err_over_4_spacings_max={worst:.3f}")
    # K = 4: the full count, the first four entries, nothing beyond them
    ids4, probs4, counts4 = _run(dev, V, GROUPS, th, 4)
    assert torch.equal(counts4, counts)
    for g in range(len(GROUPS)):
        n = min(int(counts[g]), 4)
        assert torch.equal(ids4[g, :n], ids[g, :n]) and torch.equal(probs4[g, :n], probs[g, :n])
        assert bool((ids4[g, n:] == ID_SENTINEL).all()) and bool((probs4[g, n:] == PROB_SENTINEL).all())
    if V > 5:
        assert int(counts.max()) > 4                                                 # (the cut was exercised)
    # the same bits whether a group is listed first or last of G
    order = list(reversed(range(len(GROUPS))))
    ids_r, probs_r, counts_r = _run(dev, V, [GROUPS[j] for j in order], th, K)
    for pos, j in enumerate(order):
        assert int(counts_r[pos]) == int(counts[j]) and torch.equal(ids_r[pos], ids[j]) and torch.equal(probs_r[pos], probs[j])
    ids_1, probs_1, counts_1 = _run(dev, V, [GROUPS[4]], th, K)                      # alone: G = 1
    assert int(counts_1[0]) == int(counts[4]) and torch.equal(ids_1[0], ids[4]) and torch.equal(probs_1[0], probs[4])


def test_dyadic_values_with_power_of_two_groups_are_exact_and_a_mean_equal_to_th_is_excluded():
    V, th = 1027, 0.25
    g = torch.Generator().manual_seed(9)
    acc = torch.full((N, 1032), 9.0, dtype=torch.float32)
    acc[:, :V] = torch.randint(0, 33, (N, V), generator=g).float() / 64.0            # multiples of 1/64 in [0, 1/2]
    groups = [[6], [9, 2], [15, 0, 11, 4], [1, 3, 5, 7, 8, 10, 12, 13]]
    acc[[15, 0, 11, 4], 1000] = torch.tensor([0.5, 0.25, 0.125, 0.125])              # mean exactly 1/4: excluded
    acc[[15, 0, 11, 4], 1001] = torch.tensor([0.5, 0.25, 0.125, 0.125 + 1 / 64])     # just above: kept
    acc[6, 17] = 0.25                                                                # a group of one AT th: excluded
    a64 = acc[:, :V].double().numpy()
    ids, probs, counts = _run(acc.cuda(), V, groups, th, 1027)
    for j, members in enumerate(groups):
        m = group_mean64(a64, members)                                               # exact in both precisions
        want = np.nonzero(m > th)[0]
        c = int(counts[j])
        assert c == len(want) and ids[j, :c].tolist() == want.tolist()
        assert probs[j, :c].double().numpy().tolist() == m[want].tolist()
    assert 1000 not in ids[2].tolist() and 1001 in ids[2].tolist() and 17 not in ids[0].tolist()
    assert group_mean64(a64, groups[2])[1000] == th


def test_bad_csr_arguments_are_refused_by_name():
    V = 255
    dev = torch.zeros((N, 256), device="cuda")
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)                               # noqa: E731
    assert "group_off" in _run(dev, V, None, 0.25, 4, rows=i32([0, 1, 2]), off=i32([0, 2, 1, 3]), expect_ok=False)     # not monotone
    assert "group_off" in _run(dev, V, None, 0.25, 4, rows=i32([0, 1, 2]), off=i32([0, 2, 4]), expect_ok=False)        # beyond M
    assert "group_off" in _run(dev, V, None, 0.25, 4, rows=i32([0, 1, 2]), off=i32([1, 2, 3]), expect_ok=False)        # not from 0
    assert "group_rows" in _run(dev, V, None, 0.25, 4, rows=i32([0, 17, 2]), off=i32([0, 3]), expect_ok=False)         # row >= N
    assert "group_rows" in _run(dev, V, None, 0.25, 4, rows=i32([0, -1, 2]), off=i32([0, 3]), expect_ok=False)
    assert "th must be finite" in _run(dev, V, None, float("nan"), 4, rows=i32([0]), off=i32([0, 1]), expect_ok=False)
    assert "th must be finite" in _run(dev, V, None, float("inf"), 4, rows=i32([0]), off=i32([0, 1]), expect_ok=False)
    assert "K (0)" in _run(dev, V, None, 0.25, 0, rows=i32([0]), off=i32([0, 1]), expect_ok=False)
    ids, probs, counts = _run(dev, V, None, 0.25, 4, rows=i32([0]), off=i32([0, 1]))                                   # the handle still works
    assert int(counts[0]) == 0
