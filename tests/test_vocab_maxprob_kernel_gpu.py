"""GPU: the vocab form of the greedy selection kernel (csrc/elementwise.hip, greedy_select_vocab_kernel) through
cap_op_select_vocab: per open row and vocabulary entry, acc = max(acc, softmax of the logits row as the selection sees it), over
three successive steps with fresh logits, against float64 `max_t softmax` on the same fp32 rows; everything else the step writes
bit-equal to the scoring form (cap_op_select_logprob).  Row families and helpers are those of tests/test_logprob_kernel_gpu.py.

Bar (per value): the larger of 8 x the maximal error of torch float32 softmax on the CPU against float64 over the same rows and
4 fp32 spacings at the value (tests/_fusion_ref.py).  Run with -s for the table (profiles/vocab_fusion_gpu_tolerances.txt)."""
import ctypes as C

import numpy as np
import pytest
import torch

from _fusion_ref import prob_bar, softmax64
from test_logprob_kernel_gpu import (BIG, FINISHED_ROW, MAX_LEN, N_FAMILY_ROWS, PAD, _chunks, _family_rows, _ld, _lib, _p, _padded,
                                     _select)

pytestmark = pytest.mark.gpu

VOCABS = (5, 255, 1027, 4099, 30524, 50272)
ROWS = (1, 3, 17)
SENTINEL = -5.0        # what untouched accumulator entries hold (a probability is never negative)
STEPS = (2, 3, 4)      # the `t` of three successive steps (MAX_LEN 8: none of them is the last)


def _select_vocab(logits_dev, V, t, eos, acc, min_len=0, force_eos=0, finished=None, live=None, scored0=3):
    """One launch on the caller's accumulator acc [n_caps, acc_ld] (device, updated in place).  -> tokens, finished, lengths,
    logprobs (column t), scored - on the host, as test_logprob_kernel_gpu._select returns them."""
    from embodied_captioning_amd import _native
    lib = _lib()
    R, n_caps = logits_dev.shape[0], acc.shape[0]
    fin = (torch.zeros(n_caps, dtype=torch.int32) if finished is None else finished.clone().int()).cuda()
    seq = torch.full((n_caps, MAX_LEN), -7, dtype=torch.int32, device="cuda")
    lens = torch.full((n_caps,), -1, dtype=torch.int32, device="cuda")
    lp = torch.zeros((n_caps, MAX_LEN - 1), dtype=torch.float32, device="cuda")
    sc = torch.full((n_caps,), scored0, dtype=torch.int32, device="cuda")
    live_d = n_live = None
    if live is not None:
        live_d = torch.tensor(live, dtype=torch.int32, device="cuda")
        n_live = torch.tensor([len(live)], dtype=torch.int32, device="cuda")
        assert len(live) <= R and max(live) < n_caps and min(live) >= 0
    assert acc.is_cuda and acc.dtype == torch.float32 and acc.is_contiguous() and acc.shape[1] >= V and acc.shape[1] % 4 == 0
    rc = lib.cap_op_select_vocab(_p(logits_dev), logits_dev.shape[1], V, R, t, MAX_LEN, eos, PAD, min_len, force_eos, _p(fin),
                                 _p(live_d), _p(n_live), _p(seq), _p(lens), _p(lp), MAX_LEN - 1, _p(sc), _p(acc), acc.shape[1],
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, _native.last_error()
    torch.cuda.synchronize()
    return seq[:, t + 1].cpu(), fin.cpu(), lens.cpu(), lp[:, t].cpu(), sc.cpu()


def _acc(n, V, fill=0.0):
    a = torch.full((n, _ld(V)), SENTINEL, dtype=torch.float32)
    a[:, :V] = fill
    return a.cuda()


def _step_rows(V, k):
    """The rows of step k: the families of the log-prob test, then fresh draws (gaussian, two of them peaked by 30)."""
    if k == 0:
        return _family_rows(V)
    g = torch.Generator().manual_seed(5000 + 10 * V + k)
    rows = torch.randn((N_FAMILY_ROWS, V), generator=g, dtype=torch.float32) * 2.0
    for base in (2, 11):
        rows[base, int(torch.randint(0, V, (1,), generator=g))] += 30.0
    rows[8, torch.rand(V, generator=g) < 0.3] = float("-inf")
    rows[8, V // 3] = 0.5
    return rows


@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("V", VOCABS)
def test_three_steps_of_every_row_family_against_float64(V, R):
    steps = [_step_rows(V, k) for k in range(3)]
    p64 = [softmax64(r) for r in steps]
    eos = V - 2
    # float64 expectation: a row contributes the steps at which it is open (it closes when its fp32 argmax is EOS)
    want = np.zeros((N_FAMILY_ROWS, V))
    open_ = np.array([i != FINISHED_ROW for i in range(N_FAMILY_ROWS)])
    open_at = []
    for k in range(3):
        open_at.append(open_.copy())
        want[open_] = np.maximum(want[open_], p64[k][open_])
        open_ = open_ & (steps[k].argmax(dim=1).numpy() != eos)
    all_rows = torch.cat(steps)
    bar, ref_err = prob_bar(all_rows, want)
    worst = 0.0
    for idx in _chunks(N_FAMILY_ROWS, R):
        acc = _acc(len(idx), V)
        for k, i in enumerate(idx):
            if i == FINISHED_ROW:
                acc[k] = SENTINEL                                                    # the finished row: sentinel everywhere
        fin = torch.tensor([int(i == FINISHED_ROW) for i in idx], dtype=torch.int32)
        for k, t in enumerate(STEPS):
            dev = _padded(steps[k][idx])                                             # BIG in the logits padding: never read
            assert torch.equal(fin.bool(), torch.tensor([not open_at[k][i] for i in idx]))
            tok, f, ln, lp, sc = _select_vocab(dev, V, t, eos, acc, finished=fin)
            tok0, f0, ln0, lp0, sc0 = _select(dev, V, t, eos, finished=fin)
            assert torch.equal(tok, tok0) and torch.equal(f, f0) and torch.equal(ln, ln0)
            assert torch.equal(lp, lp0) and torch.equal(sc, sc0)                     # bit-equal to the scoring form
            fin = f
        got = acc.cpu()
        assert bool((got[:, V:] == SENTINEL).all())                                  # padding columns are never written
        for k, i in enumerate(idx):
            if i == FINISHED_ROW:
                assert bool((got[k] == SENTINEL).all())
                continue
            err = np.abs(got[k, :V].double().numpy() - want[i])
            worst = max(worst, float((err / bar[i]).max()))
            assert (err <= bar[i]).all(), (V, R, i, float(err.max()), float(bar[i].min()))
            assert bool((got[k, :V] >= 0).all()) and bool((got[k, :V] <= 1).all())
    # -inf entries give exactly 0 when they are -inf at every step the row was open (row 8 at one step only: its maximum is taken)
    print(f"vocab_maxprob V={V:6d} R={R:2d} families x 3 steps  ref_err_fp32={ref_err:.3e} bar_min={bar.min():.3e} "
          f"bar_max={bar.max():.3e} kernel_err_over_bar_max={worst:.3f}")


@pytest.mark.parametrize("V", VOCABS)
def test_masked_eos_and_minus_inf_give_exactly_zero_and_the_selected_token_its_own_value(V):
    g = torch.Generator().manual_seed(6000 + V)
    x = torch.randn((3, V), generator=g, dtype=torch.float32) * 2.0
    eos = V // 2
    x[:, eos] = x.max(dim=1).values + 1.0                      # EOS is the unmasked maximum
    dead = [i for i in (0, V - 1, V // 3) if i != eos]
    x[1, dead] = float("-inf")
    masked = x.clone()
    masked[:, eos] = float("-inf")
    want = softmax64(masked)
    bar, ref_err = prob_bar(masked, want)
    acc = _acc(3, V)
    tok, f, ln, lp, sc = _select_vocab(_padded(x), V, 1, eos, acc, min_len=5, force_eos=1)
    tok0, f0, ln0, lp0, sc0 = _select(_padded(x), V, 1, eos, min_len=5, force_eos=1)
    assert torch.equal(tok, tok0) and torch.equal(f, f0) and torch.equal(ln, ln0) and torch.equal(lp, lp0) and torch.equal(sc, sc0)
    got = acc.cpu()
    assert bool((got[:, eos] == 0.0).all()) and bool((tok != eos).all())
    assert bool((got[1, dead] == 0.0).all())
    assert bool((got[:, V:] == SENTINEL).all())
    err = np.abs(got[:, :V].double().numpy() - want)
    assert (err <= bar).all(), (V, float((err / bar).max()))
    # the selected token's value is 1 / (1 + total) = exp(lp), and it is the row's maximum
    for r in range(3):
        assert int(got[r, :V].argmax()) == int(tok[r])
        assert abs(float(got[r, int(tok[r])]) - float(np.exp(np.float64(lp[r])))) <= float(bar[r].max())
    # without the mask EOS wins and carries the largest probability; a later step keeps the maximum of both
    acc2 = acc.clone()
    tok, _, _, _, _ = _select_vocab(_padded(x), V, 6 - 1, eos, acc2, min_len=5, force_eos=1)
    both = np.maximum(want, softmax64(x))
    bar2, _ = prob_bar(torch.cat([masked, x]), both)
    assert bool((tok == eos).all())
    assert (np.abs(acc2.cpu()[:, :V].double().numpy() - both) <= bar2).all()
    print(f"vocab_maxprob V={V:6d} eos-mask / -inf            ref_err_fp32={ref_err:.3e} kernel_err_over_bar_max={float((err / bar).max()):.3f}")


@pytest.mark.parametrize("V", (1027, 30524))
def test_a_rows_bits_do_not_depend_on_its_position_or_the_row_map(V):
    g = torch.Generator().manual_seed(7000 + V)
    row = torch.randn((1, V), generator=g, dtype=torch.float32) * 2.0
    others = torch.randn((17, V), generator=g, dtype=torch.float32) * 2.0
    eos = V - 2
    acc1 = _acc(1, V)
    tok1, _, _, lp1, _ = _select_vocab(_padded(row), V, 2, eos, acc1)
    for pos in (0, 7, 16):
        x = others.clone()
        x[pos] = row[0]
        acc = _acc(17, V)
        tok, _, _, lp, _ = _select_vocab(_padded(x), V, 2, eos, acc)
        assert int(tok[pos]) == int(tok1[0]) and torch.equal(lp[pos:pos + 1], lp1)
        assert torch.equal(acc[pos], acc1[0]), pos                                   # R = 1 and inside R = 17: the same bits
    # through a RowMap: compact row 0 of 3 is caption 5 of 17; captions outside the map and rows beyond *n_live are untouched
    x = others[:3].clone()
    x[0] = row[0]
    live = [5, 9, 12]
    acc = _acc(17, V, fill=SENTINEL)
    acc[live] = _acc(3, V)
    tok, f, ln, lp, sc = _select_vocab(_padded(x), V, 2, eos, acc, live=live)
    tok0, f0, ln0, lp0, sc0 = _select(_padded(x), V, 2, eos, live=live, n_caps=17)
    assert torch.equal(tok, tok0) and torch.equal(f, f0) and torch.equal(ln, ln0) and torch.equal(lp, lp0) and torch.equal(sc, sc0)
    assert torch.equal(acc[5], acc1[0])
    untouched = [i for i in range(17) if i not in live]
    assert bool((acc[untouched] == SENTINEL).all()) and bool((acc[live][:, :V] >= 0).all())
    acc = _acc(17, V, fill=SENTINEL)
    acc[live[:2]] = _acc(2, V)
    _select_vocab(_padded(x), V, 2, eos, acc, live=live[:2])
    assert bool((acc[12] == SENTINEL).all()) and torch.equal(acc[5], acc1[0])


def test_bad_accumulator_arguments_are_refused():
    from embodied_captioning_amd import _native
    lib = _lib()
    V = 255
    dev = _padded(torch.zeros((1, V)))
    i32 = lambda v: torch.full((1,), v, dtype=torch.int32, device="cuda")            # noqa: E731
    fin, lens, sc = i32(0), i32(0), i32(0)
    seq = torch.zeros((1, MAX_LEN), dtype=torch.int32, device="cuda")
    lp = torch.zeros((1, MAX_LEN - 1), device="cuda")
    acc = torch.zeros((1, 264), device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(acc_ptr, acc_ld, lp_t=lp):
        return lib.cap_op_select_vocab(_p(dev), dev.shape[1], V, 1, 2, MAX_LEN, V - 2, PAD, 0, 0, _p(fin), None, None, _p(seq), _p(lens),
                                       _p(lp_t), MAX_LEN - 1, _p(sc), acc_ptr, acc_ld, s)
    assert call(_p(acc), 252) != 0 and "acc_ld" in _native.last_error()              # below V
    assert call(_p(acc), 262) != 0 and "acc_ld" in _native.last_error()              # not a multiple of 4
    assert call(C.c_void_p(acc.data_ptr() + 4), 256) != 0 and "aligned" in _native.last_error()
    assert call(_p(acc), 256, lp_t=None) != 0
    assert call(_p(acc), 256) == 0
    torch.cuda.synchronize()
