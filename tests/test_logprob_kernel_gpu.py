"""GPU: the scoring form of the greedy selection kernel (csrc/elementwise.hip, greedy_select_logprob_kernel) through
cap_op_select_logprob: per open row, log max softmax of the logits row as the selection sees it, against float64 numpy on the
same fp32 logits; tokens / finished / lengths bit-equal to the plain kernel (the same entry with null log-prob buffers).

Bar (per value): the larger of
  8 x the maximal error of torch float32 on the CPU (`log_softmax(-1).max(-1)`) against float64 over the same rows - the
      project's convention for an fp32 kernel against another fp32 implementation's own rounding, and
  4 spacings of fp32 at the value's magnitude (a correctly rounded result is already half a spacing off, and on a tiny
      vocabulary the measured reference error can be 0).
Run with -s for the table of reference error, bar and kernel error per shape (the output meant for
profiles/token_logprob_gpu_tolerances.txt)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

VOCABS = (5, 255, 1024, 1027, 4099, 30524, 50272)
ROWS = (1, 3, 17)
N_FAMILY_ROWS = 17
FINISHED_ROW = 9
BIG = 3.0e38          # what the padding columns between V and ld hold: a kernel that reads them picks them
PAD, MAX_LEN = 0, 8


def _p(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def _lib():
    from embodied_captioning_amd import _native
    return _native.load_library()


def _ld(V):
    return (V + 3) // 4 * 4 + 4


def _padded(rows):
    """fp32 [n, V] host rows -> device [n, ld] with BIG in the padding columns."""
    n, V = rows.shape
    buf = torch.full((n, _ld(V)), BIG, dtype=torch.float32)
    buf[:, :V] = rows
    return buf.cuda()


def _select(logits_dev, V, t, eos, min_len=0, force_eos=0, finished=None, live=None, n_caps=None, score=True, scored0=3):
    """One launch.  -> tokens [n_caps] (column t + 1), finished, lengths, logprobs [n_caps] (column t), scored - on the host."""
    from embodied_captioning_amd import _native
    lib = _lib()
    R = logits_dev.shape[0]
    n_caps = n_caps or R
    fin = torch.zeros(n_caps, dtype=torch.int32) if finished is None else finished.clone().int()
    fin = fin.cuda()
    seq = torch.full((n_caps, MAX_LEN), -7, dtype=torch.int32, device="cuda")
    lens = torch.full((n_caps,), -1, dtype=torch.int32, device="cuda")
    lp = torch.zeros((n_caps, MAX_LEN - 1), dtype=torch.float32, device="cuda") if score else None
    sc = torch.full((n_caps,), scored0, dtype=torch.int32, device="cuda") if score else None
    live_d = n_live = None
    if live is not None:
        live_d = torch.tensor(live, dtype=torch.int32, device="cuda")
        n_live = torch.tensor([len(live)], dtype=torch.int32, device="cuda")
        assert len(live) <= R and max(live) < n_caps and min(live) >= 0
    rc = lib.cap_op_select_logprob(_p(logits_dev), logits_dev.shape[1], V, R, t, MAX_LEN, eos, PAD, min_len, force_eos, _p(fin),
                                   _p(live_d), _p(n_live), _p(seq), _p(lens), _p(lp), MAX_LEN - 1, _p(sc),
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, _native.last_error()
    torch.cuda.synchronize()
    if score:
        other = torch.ones(MAX_LEN - 1, dtype=torch.bool)
        other[t] = False
        assert float(lp[:, other].abs().max()) == 0.0                     # only column t is written
    return (seq[:, t + 1].cpu(), fin.cpu(), lens.cpu(), lp[:, t].cpu() if score else None, sc.cpu() if score else None)


@functools.lru_cache(maxsize=None)
def _family_rows(V):
    """17 fp32 rows: gaussian x 4, peaked, flat, maximum at 0, maximum at V - 1, -inf entries, (the finished row), then the same
    families again with other draws."""
    g = torch.Generator().manual_seed(1000 + V)
    rows = torch.randn((N_FAMILY_ROWS, V), generator=g, dtype=torch.float32) * 2.0
    for base in (4, 13):
        rows[base, int(torch.randint(0, V, (1,), generator=g))] += 30.0          # peaked: one logit 30 above the rest
    rows[5] = 1.75                                                                # flat: -log V
    rows[14] = -3.5
    rows[6, 0] = rows[6].max() + 1.0                                              # maximum at index 0
    rows[7, V - 1] = rows[7].max() + 1.0                                          # maximum at index V - 1
    rows[15, 0] = rows[15].max() + 0.5
    rows[16, V - 1] = rows[16].max() + 0.5
    rows[8, torch.rand(V, generator=g) < 0.4] = float("-inf")                     # -inf entries (never the whole row)
    rows[8, V // 2] = 0.25
    return rows


def _want(rows):
    """float64 log max softmax, and what torch float32 on the CPU gives for it."""
    x = rows.double().numpy()
    m = x.max(axis=1, keepdims=True)
    want = -np.log(np.exp(x - m).sum(axis=1))
    ref32 = torch.log_softmax(rows, dim=-1).max(dim=-1).values.double().numpy()
    return want, ref32


def _bar(want, ref_err):
    return np.maximum(8.0 * ref_err, 4.0 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64))


def _chunks(n, R):
    return [list(range(s, s + R)) if s + R <= n else list(range(n - R, n)) for s in range(0, n, R)]


@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("V", VOCABS)
def test_logprob_of_every_row_family_against_float64(V, R):
    rows = _family_rows(V)
    want, ref32 = _want(rows)
    ref_err = float(np.abs(ref32 - want).max())
    bar = _bar(want, ref_err)
    eos = V - 2
    exp_tok = rows.argmax(dim=1).int()
    worst = 0.0
    for idx in _chunks(N_FAMILY_ROWS, R):
        fin = torch.tensor([int(i == FINISHED_ROW) for i in idx], dtype=torch.int32)
        dev = _padded(rows[idx])
        tok, f, ln, lp, sc = _select(dev, V, 2, eos, finished=fin)
        tok0, f0, ln0, _, _ = _select(dev, V, 2, eos, finished=fin, score=False)
        assert torch.equal(tok, tok0) and torch.equal(f, f0) and torch.equal(ln, ln0)
        for k, i in enumerate(idx):
            if i == FINISHED_ROW:                  # pad emitted, nothing scored
                assert int(tok[k]) == PAD and float(lp[k]) == 0.0 and int(sc[k]) == 3 and int(f[k]) == 1
                continue
            assert int(tok[k]) == int(exp_tok[i]) and int(sc[k]) == 4
            assert int(f[k]) == int(int(exp_tok[i]) == eos)
            err = abs(float(lp[k]) - want[i])
            worst = max(worst, err / bar[i])
            assert err <= bar[i], (V, R, i, float(lp[k]), want[i], bar[i])
    live = [i for i in range(N_FAMILY_ROWS) if i != FINISHED_ROW]
    print(f"token_logprob V={V:6d} R={R:2d} families   ref_err_fp32={ref_err:.3e} bar_min={bar[live].min():.3e} "
          f"bar_max={bar[live].max():.3e} kernel_err_over_bar_max={worst:.3f}")
    if V > 1:
        flat = -np.log(float(V))
        assert abs(want[5] - flat) < 1e-12 and abs(want[14] - flat) < 1e-12


@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("V", VOCABS)
def test_eos_mask_and_forced_eos(V, R):
    """MinLength: EOS is the row's maximum but masked - the token is the runner-up and lp is that of the masked row.  Forced EOS
    on the last step: the token is EOS, lp is that of the row's maximum (which is not EOS)."""
    g = torch.Generator().manual_seed(2000 + V + R)
    rows = torch.randn((R, V), generator=g, dtype=torch.float32) * 2.0
    worst = 0.0
    for eos, t, min_len in ((V // 2, 1, 5), (V - 1, 0, 3), (V - 1, MAX_LEN - 2, 3)):
        x = rows.clone()
        last = t + 2 >= MAX_LEN
        if not last:
            x[:, eos] = x.max(dim=1).values + 1.0            # EOS is the unmasked maximum
        else:
            x[:, eos] = x.min(dim=1).values - 1.0            # EOS would never be chosen
        masked = x.clone()
        if t + 1 < min_len:
            masked[:, eos] = float("-inf")
        assert (t + 1 < min_len) == (not last)
        want, ref32 = _want(masked)
        bar = _bar(want, float(np.abs(ref32 - want).max()))
        dev = _padded(x)
        tok, f, ln, lp, sc = _select(dev, V, t, eos, min_len=min_len, force_eos=1)
        tok0, f0, ln0, _, _ = _select(dev, V, t, eos, min_len=min_len, force_eos=1, score=False)
        assert torch.equal(tok, tok0) and torch.equal(f, f0) and torch.equal(ln, ln0)
        top = masked.argmax(dim=1).int()
        if last:
            assert bool((tok == eos).all()) and bool((top != eos).all()) and bool((f == 1).all()) and bool((ln == t + 2).all())
        else:
            assert torch.equal(tok, top) and bool((tok != eos).all())
            assert bool((tok != x.argmax(dim=1).int()).all())              # the mask changed the token
        assert bool((sc == 4).all())
        err = np.abs(lp.double().numpy() - want)
        worst = max(worst, float((err / bar).max()))
        assert (err <= bar).all(), (V, R, eos, t, lp, want, bar)
    print(f"token_logprob V={V:6d} R={R:2d} eos-mask   kernel_err_over_bar_max={worst:.3f}")


@pytest.mark.parametrize("V", (1027, 30524))
def test_value_does_not_depend_on_the_rows_position(V):
    g = torch.Generator().manual_seed(3000 + V)
    row = torch.randn((1, V), generator=g, dtype=torch.float32) * 2.0
    others = torch.randn((17, V), generator=g, dtype=torch.float32) * 2.0
    eos = V - 2
    tok1, _, _, lp1, _ = _select(_padded(row), V, 2, eos)
    for pos in (0, 7, 16):
        x = others.clone()
        x[pos] = row[0]
        tok, _, _, lp, sc = _select(_padded(x), V, 2, eos)
        assert int(tok[pos]) == int(tok1[0]) and torch.equal(lp[pos:pos + 1], lp1), (pos, float(lp[pos]), float(lp1[0]))
    # through a RowMap: compact row 0 of 3 is caption 5 of 17
    x = others[:3].clone()
    x[0] = row[0]
    live = [5, 9, 12]
    tok, f, ln, lp, sc = _select(_padded(x), V, 2, eos, live=live, n_caps=17)
    tok0, f0, ln0, _, _ = _select(_padded(x), V, 2, eos, live=live, n_caps=17, score=False)
    assert torch.equal(tok, tok0) and torch.equal(f, f0) and torch.equal(ln, ln0)
    assert torch.equal(lp[5:6], lp1) and int(tok[5]) == int(tok1[0])
    untouched = [i for i in range(17) if i not in live]
    assert float(lp[untouched].abs().max()) == 0.0 and bool((sc[untouched] == 3).all()) and bool((sc[live] == 4).all())
    assert bool((tok[untouched] == -7).all())
    # rows of the launch beyond *n_live are skipped
    tok, _, _, lp, sc = _select(_padded(x), V, 2, eos, live=live[:2], n_caps=17)
    assert int(tok[12]) == -7 and float(lp[12]) == 0.0 and int(sc[12]) == 3 and torch.equal(lp[5:6], lp1)
