"""GPU: the processed forms of the two token selections alone (cap_set_repeat_controls' kernels): greedy_select_processed_kernel
through cap_op_select_processed and the processed beam candidate kernels through cap_op_beam_step_processed, against
tests/_repeat_ref.py (and tests/_bad_words_ref.py for the ban that may come with them).

Greedy: equality is exact - kernel and restatement read the same fp32 values, penalise them with the same two fp32 operations (a
multiplication, a correctly rounded division) and only compare them.
Beam step: as tests/test_bad_words_kernels_gpu.py - the next running beams of a step are the K best of all K x V continuations by
(value desc, flat index asc), value = fp64 log-softmax of the RAW row, the penalty on the log-probs, the bans at -inf, + the running
score.  Tokens must be identical; scores within 8 x the error of the same restatement in fp32 against fp64 over the case + one fp32
spacing of the score.  The test asserts on the REFERENCE that the decisions it compares are further apart than twice that bar."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from _bad_words_ref import bitmap_and_table
from _repeat_ref import beam_log_probs, greedy_choice, ngram_banned_mask

pytestmark = pytest.mark.gpu

BIG = 3.0e38          # the columns between V and ld: a kernel that reads them picks them
PAD, EOS, MAX_LEN = 0, 2, 12
VOCABS = ((37, 40), (515, 517), (30524, 30528), (50272, 50276))      # (V, ld): 515 / 517 = rows that are not 16-byte aligned
N_ROWS = 5
N_CAPS = 7
COMBOS = {            # name -> (penalty, n-gram size, with a ban set)
    "penalty_only": (1.5, 0, False),
    "ngram1_only": (1.0, 1, False),
    "ngram2_only": (1.0, 2, False),
    "ngram3_only": (1.0, 3, False),
    "ban_only": (1.0, 0, True),
    "all_three": (1.5, 2, True),
    "reward_and_ngram3": (0.5, 3, True),
}


@pytest.fixture(scope="module")
def lib():
    from embodied_captioning_amd import _native
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _native.load_library()


def _p(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _words(V):
    return ((V + 31) // 32 + 3) // 4 * 4


def _ban_arrays(seqs, V, eos):
    """The set as the kernels read it; no sequences = no static bitmap at all (a null pointer)."""
    if not seqs:
        return None, None, 0
    bits, table = bitmap_and_table(seqs, V, _words(V), eos=eos)
    bits_d = torch.from_numpy(bits.view(np.int32)).cuda()
    table_d = torch.from_numpy(table).cuda() if len(table) else None
    return bits_d, table_d, len(table)


@functools.lru_cache(maxsize=None)
def _rows(V):
    """5 fp32 rows, computed once per vocabulary and never modified: gaussian rows of both signs, the maximum 1.2 x the runner-up
    at an index of its own (0, 31, 32, V // 3, V - 1): a penalty of 1.5 takes it to 0.8 x the runner-up, a reward keeps it first."""
    g = torch.Generator().manual_seed(177 + V)
    rows = (torch.randn((N_ROWS, V), generator=g, dtype=torch.float32) * 2.0).numpy()
    rows = np.abs(rows)                                                    # positive maxima: the penalty divides
    rows[:, 1::2] *= -1.0                                                  # and negative entries, which it multiplies
    for r, i in enumerate((0, 31, 32, V // 3, V - 1)):
        rows[r, i] = -1.0
        rows[r, i] = 1.2 * rows[r].max()
    rows.setflags(write=False)
    return rows


def _top(row, k=3):
    return [int(i) for i in np.argsort(-row, kind="stable")[:k]]


def _histories(V, rows, t, hist0, cap_of_row, seed):
    """Caption histories [N_CAPS, MAX_LEN] whose columns hist0 .. t are the stored context: ordinary tokens, and for the caption of
    logits row c a tail around top = the row's arg-max: `top`, `top x`, `x top x`, `x top u x`, and from five tokens on `u x top u x` -
    top is always in the context (the penalty and n = 1 reach it), from three tokens on behind an earlier `x` (n = 2), from five on
    behind an earlier `u x` (n = 3).  Columns in front of hist0 hold other tokens, which nothing may read."""
    g = torch.Generator().manual_seed(seed)
    lo = 4 if V > 64 else 3
    hist = torch.randint(lo, V, (N_CAPS, MAX_LEN), generator=g).numpy().astype(np.int32)
    for c, cap in enumerate(cap_of_row):
        top = _top(rows[c])[0]
        u, x = (top + 5) % V, (top + 11) % V
        tail = {1: [top], 2: [top, x], 3: [x, top, x], 4: [x, top, u, x]}.get(t + 1 - hist0, [u, x, top, u, x])
        hist[cap, t + 1 - len(tail):t + 1] = tail
    return hist


def _context(hist_row, t, hist0, prefix):
    vn, vtok, vbos = prefix
    real = [int(x) for x in hist_row[hist0:t + 1]]
    if vbos >= 0 and real:
        real[0] = vbos
    return [vtok] * vn + real


def _select(lib, V, ld, rows, hist, t, p, n, seqs, live=None, finished=(), hist0=0, prefix=(0, 0, -1), eos=EOS):
    """One launch over the logits rows; -> seq column t + 1, finished, lengths of every caption."""
    R = rows.shape[0]
    buf = torch.full((R, ld), BIG, dtype=torch.float32)
    buf[:, :V] = torch.from_numpy(np.array(rows))
    logits = buf.cuda()
    seq = torch.full((N_CAPS, MAX_LEN), -7, dtype=torch.int32)
    seq[:, :t + 1] = torch.from_numpy(np.array(hist[:, :t + 1]))
    seq = seq.cuda()
    fin = torch.zeros(N_CAPS, dtype=torch.int32)
    for c in finished:
        fin[c] = 1
    fin = fin.cuda()
    lens = torch.full((N_CAPS,), -1, dtype=torch.int32, device="cuda")
    live_d = n_live = None
    if live is not None:
        live_d = torch.tensor(list(live) + [0] * (R - len(live)), dtype=torch.int32, device="cuda")
        n_live = torch.tensor([len(live)], dtype=torch.int32, device="cuda")
    bits_d, table_d, n_multi = _ban_arrays(seqs, V, eos)
    rc = lib.cap_op_select_processed(_p(logits), ld, V, R, t, MAX_LEN, eos, PAD, _p(fin), _p(live_d), _p(n_live), _p(seq), _p(lens),
                                     _p(bits_d), _p(table_d), n_multi, hist0, C.c_float(p), n, prefix[0], prefix[1], prefix[2], _stream())
    assert rc == 0, lib.cap_last_error().decode()
    torch.cuda.synchronize()
    assert torch.equal(seq[:, :t + 1].cpu(), torch.from_numpy(np.array(hist[:, :t + 1])))      # the history is read only
    return seq[:, t + 1].cpu().numpy(), fin.cpu().numpy(), lens.cpu().numpy()


def _want(V, rows, hist, t, p, n, seqs, live=None, finished=(), hist0=0, prefix=(0, 0, -1), eos=EOS):
    caps = list(range(rows.shape[0])) if live is None else list(live)
    tok = np.full(N_CAPS, -7, dtype=np.int64)
    for c, cap in enumerate(caps):
        ctx = _context(hist[cap], t, hist0, prefix)
        tok[cap] = PAD if cap in finished else greedy_choice(rows[c], ctx, p, n, seqs, eos=eos, ban_context=hist[cap, hist0:t + 1])
    return tok


def _ban_for(rows, V):
    """A ban set of single tokens: every row's runner-up (unless it is another row's arg-max) and two edge tokens."""
    tops = {_top(r)[0] for r in rows}
    return [[_top(r)[1]] for r in rows if _top(r)[1] not in tops] + [[V - 2], [33 % V]]


@pytest.mark.parametrize("V,ld", VOCABS)
@pytest.mark.parametrize("combo", sorted(COMBOS))
def test_greedy_combinations_against_the_restatement(lib, V, ld, combo):
    p, n, with_ban = COMBOS[combo]
    rows = _rows(V)
    seqs = _ban_for(rows, V) if with_ban else []
    raw = np.array([_top(r)[0] for r in rows])
    for R in (1, 5):
        for t in (0, 1, 4, 9):
            hist = _histories(V, rows[:R], t, 0, range(R), seed=V + t)
            got, fin, lens = _select(lib, V, ld, rows[:R], hist, t, p, n, seqs)
            want = _want(V, rows[:R], hist, t, p, n, seqs)
            assert np.array_equal(got, want), (combo, R, t, got, want)
            assert (got[R:] == -7).all() and (fin[R:] == 0).all()
            # what _rows and _histories arrange, asserted on the reference: the arg-max is taken away by a penalty, by n = 1, by n = 2
            # from 3 context tokens on and by n = 3 from 5 on; the ban alone holds runner-ups only and a reward keeps the arg-max
            # (with the runner-up banned as well, whether a penalised arg-max still wins depends on the third entry: not asserted)
            banned = n == 1 or (n == 2 and t + 1 >= 3) or (n == 3 and t + 1 >= 5)
            if banned or (p > 1.0 and not with_ban):
                assert (want[:R] != raw[:R]).all(), (combo, t, want, raw)
            elif p <= 1.0:
                assert (want[:R] == raw[:R]).all(), (combo, t, want, raw)
            assert (fin[:R] == ((got[:R] == EOS) | (t + 2 >= MAX_LEN))).all()


@pytest.mark.parametrize("V,ld", VOCABS)
def test_row_map_finished_rows_and_a_virtual_prefix(lib, V, ld):
    """Logits row c belongs to caption live[c]; a finished caption emits pad whatever is processed.  BLIP-2's shape: the stored
    context starts at column hist0 = 3, its first token reads as BOS whatever the column holds, and 8 image placeholders stand in
    front of it - at the first step both ids are already penalised, and a model that emits the placeholder meets the prefix's
    n-grams."""
    rows = _rows(V)
    tops = [_top(r) for r in rows]
    live, finished = [5, 2, 6, 0], (2,)
    seqs = _ban_for(rows, V)
    t = 6
    hist = _histories(V, rows[:4], t, 0, live, seed=V)
    got, fin, lens = _select(lib, V, ld, rows[:4], hist, t, 1.5, 2, seqs, live=live, finished=finished)
    want = _want(V, rows[:4], hist, t, 1.5, 2, seqs, live=live, finished=finished)
    assert np.array_equal(got, want), (got, want)
    assert got[2] == PAD and fin[2] == 1 and lens[2] == -1
    assert (got[[1, 3, 4]] == -7).all() and (fin[[1, 3, 4]] == 0).all() and (lens[[1, 3, 4]] == -1).all()
    assert got[5] != tops[0][0] and got[6] != tops[2][0] and got[0] != tops[3][0]
    # the virtual prefix: placeholder = row 0's arg-max, BOS = row 1's
    hist0, prefix = 3, (8, tops[0][0], tops[1][0])
    for t in (3, 4, 8):
        for p, n in ((1.5, 0), (1.0, 1), (1.0, 2), (1.5, 3)):
            hist = _histories(V, rows, t, hist0, range(N_ROWS), seed=V + 50 + t)
            if t == 4:
                hist[0, 4] = prefix[1]                  # caption 0 has just emitted the placeholder id
                hist[1, 4] = prefix[2]                  # caption 1 BOS
            got, _, _ = _select(lib, V, ld, rows, hist, t, p, n, [], hist0=hist0, prefix=prefix)
            want = _want(V, rows, hist, t, p, n, [], hist0=hist0, prefix=prefix)
            assert np.array_equal(got, want), (t, p, n, got, want)
            if t == 3 and (p > 1.0 or n == 1):          # the first step: context = placeholders + BOS
                assert want[0] != tops[0][0] and want[1] != tops[1][0]
            if t == 4 and n == 2:                       # "placeholder placeholder" and "placeholder BOS" have occurred
                m = ngram_banned_mask(_context(hist[0], t, hist0, prefix), V, 2)
                assert m[prefix[1]] and m[prefix[2]] and want[0] != tops[0][0]


def test_bos_equal_to_eos_is_penalised_from_the_first_step(lib):
    """OPT's BOS and EOS are one id: under a penalty the EOS score is penalised at every step, the first included."""
    V, ld = 515, 520
    rows = np.array(_rows(V)[:2])
    eos = 9
    rows[0, eos] = rows[0].max() + 0.5           # EOS would win and end the caption ...
    rows[1, eos] = rows[1].max() * 3.0           # ... and here it still wins after the penalty
    prefix = (8, V - 4, eos)                     # BOS = EOS
    hist = _histories(V, rows, 3, 3, range(2), seed=3)
    hist[:, 3] = PAD                             # the column that stands for BOS holds pad
    got, fin, lens = _select(lib, V, ld, rows, hist, 3, 1.5, 0, [], hist0=3, prefix=prefix, eos=eos)
    want = _want(V, rows, hist, 3, 1.5, 0, [], hist0=3, prefix=prefix, eos=eos)
    assert np.array_equal(got, want)
    assert got[0] != eos and fin[0] == 0 and got[1] == eos and fin[1] == 1 and lens[1] == 5
    free, fin0, _ = _select(lib, V, ld, rows, hist, 3, 1.0, 1, [[V - 9]], hist0=3, prefix=(0, 0, -1), eos=eos)      # no penalty: EOS wins
    assert free[0] == eos and fin0[0] == 1


@pytest.mark.parametrize("V,ld", ((37, 40), (50272, 50276)))
def test_ties_created_by_the_penalty_and_a_row_with_nothing_left(lib, V, ld):
    # 3.0 / 1.5 == 2.0 exactly: the first maximal index wins, whichever side the unseen 2.0 lies on
    a, b = 5, V - 2
    for seen_tok, unseen_tok in ((a, b), (b, a)):
        row = np.full((1, V), -1.0, dtype=np.float32)
        row[0, seen_tok], row[0, unseen_tok] = 3.0, 2.0
        hist = np.full((N_CAPS, MAX_LEN), 7, dtype=np.int32)
        hist[0, 2] = seen_tok
        got, _, _ = _select(lib, V, ld, row, hist, 4, 1.5, 0, [])
        assert got[0] == min(a, b) == _want(V, row, hist, 4, 1.5, 0, [])[0]
        got, _, _ = _select(lib, V, ld, row, hist, 4, 1.4, 0, [])
        assert got[0] == seen_tok
    # scores exactly 0 and -inf stay what they are; a negative maximum is multiplied
    row = np.full((1, V), -np.inf, dtype=np.float32)
    row[0, 3], row[0, 4], row[0, 6] = 0.0, -0.5, -0.7
    hist = np.full((N_CAPS, MAX_LEN), 3, dtype=np.int32)
    hist[0, 1], hist[0, 2] = 4, 8
    got, _, _ = _select(lib, V, ld, row, hist, 4, 1.5, 0, [])
    assert got[0] == 3 == _want(V, row, hist, 4, 1.5, 0, [])[0]
    row[0, 3] = -np.inf
    got, _, _ = _select(lib, V, ld, row, hist, 4, 1.5, 0, [])          # -0.5 * 1.5 = -0.75 < -0.7
    assert got[0] == 6 == _want(V, row, hist, 4, 1.5, 0, [])[0]
    # everything banned: n = 1 takes the context's tokens, the ban set every other one -> index 0, like torch.argmax
    rows = _rows(V)[:2]
    hist = _histories(V, rows, 6, 0, range(2), seed=1)
    for r in range(2):
        ctx = set(int(x) for x in hist[r, :7])
        seqs = [[i] for i in range(V) if i not in ctx]
        got, _, _ = _select(lib, V, ld, rows[r:r + 1], hist[r:r + 1].repeat(N_CAPS, 0), 6, 1.5, 1, seqs, eos=-5)
        assert got[0] == 0
    # context ids outside [0, V) are ignored by both controls
    hist = np.full((N_CAPS, MAX_LEN), V + 100, dtype=np.int32)
    hist[:, 1] = -3
    got, _, _ = _select(lib, V, ld, rows, hist, 5, 1.5, 1, [])
    assert (got[:2] == [_top(r)[0] for r in rows]).all()


def test_refusals(lib):
    V = 515
    logits = torch.zeros((1, 520), device="cuda")
    seq = torch.zeros((1, MAX_LEN), dtype=torch.int32, device="cuda")
    fin = torch.zeros(1, dtype=torch.int32, device="cuda")
    lens = torch.zeros(1, dtype=torch.int32, device="cuda")

    def call(p=1.5, n=2, n_multi=0, hist0=0, vn=0):
        return lib.cap_op_select_processed(_p(logits), 520, V, 1, 3, MAX_LEN, EOS, PAD, _p(fin), None, None, _p(seq), _p(lens), None, None,
                                           n_multi, hist0, C.c_float(p), n, vn, 0, -1, _stream())
    assert call() == 0
    for kw, word in ((dict(p=0.0), "penalty"), (dict(p=float("inf")), "penalty"), (dict(p=float("nan")), "penalty"), (dict(n=-1), "n-gram size"),
                     (dict(n_multi=1), "ban_multi"), (dict(hist0=5), "hist0"), (dict(vn=-1), "virtual")):
        assert call(**kw) != 0 and word in lib.cap_last_error().decode(), (word, lib.cap_last_error().decode())
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ beam step
BOS = 1
BEAM_CASES = [      # the shapes of tests/test_bad_words_kernels_gpu.py's BEAM_CASES: name, B, K, V, ld, steps; then penalty, n, ban, prefix
    ("1x3_v515", 1, 3, 515, 520, 5, 0.7, 2, False, 0),
    ("2x5_v515", 2, 5, 515, 520, 5, 1.5, 1, True, 0),
    ("2x5_v515_plain_kernel", 2, 5, 515, 517, 4, 0.7, 3, True, 8),            # ld % 4 != 0: the plain rows kernel
    ("1x3_v30524_row_in_lds", 1, 3, 30524, 30528, 4, 0.7, 2, True, 8),        # row + lists + two bitmaps: 142 KB, still staged
    ("1x3_v50272_lists_only", 1, 3, 50272, 50276, 4, 0.7, 2, False, 0),
    ("2x5_v515_no_penalty", 2, 5, 515, 520, 5, 1.0, 1, False, 0),
]


def _beam_context(tok_row, cur_len, vn, vtok):
    return [vtok] * vn + [int(x) for x in tok_row[:cur_len]]


def _host_step(run_tok, run_sc, rows, cur_len, ctl, seqs, B, K, V, dtype):
    """One step of HF's `_beam_search` when nothing finishes (see the module docstring).  -> tokens [R, L], scores [R], the source
    beam of every new beam, and the gap between the K-th and the (K + 1)-th value per item."""
    p, n, vn, vtok = ctl
    new_tok, new_sc, src, gaps = run_tok.copy(), np.zeros(B * K, dtype=dtype), np.zeros(B * K, dtype=np.int64), []
    for b in range(B):
        vals = np.stack([beam_log_probs(rows[b * K + k], _beam_context(run_tok[b * K + k], cur_len, vn, vtok), p, n, seqs, dtype, eos=EOS,
                                        ban_context=run_tok[b * K + k, :cur_len]) + dtype(run_sc[b * K + k])
                         for k in range(K)]).reshape(-1)
        order = np.lexsort((np.arange(vals.size), -vals))[:K + 1]
        gaps += [float(vals[order[i]] - vals[order[i + 1]]) for i in range(K)]
        for k in range(K):
            f = int(order[k])
            sk, tok = f // V, f % V
            new_tok[b * K + k] = run_tok[b * K + sk]
            new_tok[b * K + k, cur_len] = tok
            new_sc[b * K + k] = vals[f]
            src[b * K + k] = sk
    return new_tok, new_sc, src, min(gaps)


def _step_inputs(g, tok64, cur_len, case):
    """The logits rows and the ban set of one step, from the reference's own beams.  Every row gets its context's most recent
    distinct tokens among its best: above the maximum under a penalty or n = 1 (which then take them away), just below it under a
    reward (which then lifts them over it - so beams repeat themselves and the n-gram rule has work)."""
    name, B, K, V, ld, steps, p, n, with_ban, vn = case
    R = B * K
    vtok = V - 3
    rows = (torch.randn((R, V), generator=g, dtype=torch.float32) * 2.0).numpy()
    rows[:, EOS] = -60.0                                                                       # never a candidate worth keeping
    for r in range(R):
        ctx = _beam_context(tok64[r], cur_len, vn, vtok)
        recent = list(dict.fromkeys(reversed(ctx)))[:4]
        top = float(rows[r].max())
        if p < 1.0:
            for j, tok in enumerate(recent):
                rows[r, tok] = top - 0.5 - 0.05 * j
        else:
            rows[r, recent[0]] = top + 0.3
    seqs = []
    if with_ban:
        seqs = [[7], [31], [32], [V - 1]]
        for r in range(R):                      # the token each beam would take first, behind its logical history's last token
            seqs.append([int(tok64[r, cur_len - 1]), int(np.argsort(-rows[r])[1])])
    return rows, seqs


def reference_trajectory(case):
    """The fp64 beams of every step of a case with what the kernel is given at it, and the fp32 restatement's error against them."""
    name, B, K, V, ld, steps, p, n, with_ban, vn = case
    R, L = B * K, MAX_LEN
    ctl = (p, n, vn, V - 3)
    g = torch.Generator().manual_seed(11 + V + K + n)
    tok64 = np.zeros((R, L), dtype=np.int64)
    tok64[:, 0] = BOS
    sc64 = np.full(R, -1e9)
    sc64[::K] = 0.0
    sc32 = sc64.astype(np.float32)
    out, err, reordered, bitten, ngram_bites = [], 0.0, False, 0, 0
    for cur_len in range(1, steps + 1):
        rows, seqs = _step_inputs(g, tok64, cur_len, case)
        free = _host_step(tok64, sc64, rows, cur_len, (1.0, 0, 0, 0), [], B, K, V, np.float64)
        no_ngram = _host_step(tok64, sc64, rows, cur_len, (p, 0, vn, V - 3), seqs, B, K, V, np.float64)
        want_tok, want_sc, src, gap = _host_step(tok64, sc64, rows, cur_len, ctl, seqs, B, K, V, np.float64)
        _, sc32_next, _, _ = _host_step(tok64, sc32, rows, cur_len, ctl, seqs, B, K, V, np.float32)
        bitten += int(not np.array_equal(free[0], want_tok))
        ngram_bites += int(not np.array_equal(no_ngram[0], want_tok))
        reordered = reordered or any(int(src[r]) != r % K for r in range(R))
        live = want_sc > -1e8
        err = max(err, float(np.abs(sc32_next.astype(np.float64) - want_sc)[live].max()))
        out.append((cur_len, rows, seqs, want_tok, want_sc, gap))
        tok64, sc64, sc32 = want_tok, want_sc, sc32_next.astype(np.float32)
    return out, err, reordered, bitten, ngram_bites


@pytest.mark.parametrize("case", BEAM_CASES, ids=[c[0] for c in BEAM_CASES])
def test_processed_beam_step_against_fp64(lib, case):
    name, B, K, V, ld, steps, p, n, with_ban, vn = case
    R, L = B * K, MAX_LEN
    traj, err, reordered, bitten, ngram_bites = reference_trajectory(case)
    assert reordered, "no step re-ordered the beams: the logical history was never different from the physical row's"
    assert bitten == steps, "the controls changed nothing at some step"
    assert ngram_bites >= 1, "the n-gram rule changed nothing at any step"
    nbytes = lib.cap_op_beam_state_bytes(B, K, L)
    state = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device="cuda")
    anc = torch.zeros((2, R, L), dtype=torch.int32, device="cuda")
    run_tokens = torch.zeros((R, L), dtype=torch.int32, device="cuda")
    run_scores = torch.zeros((R,), dtype=torch.float32, device="cuda")
    active = torch.zeros((1,), dtype=torch.int32, device="cuda")
    assert lib.cap_op_beam_init(_p(state), B, K, L, BOS, PAD, EOS, 0, _stream()) == 0
    worst = 0.0
    for cur_len, rows, seqs, want_tok, want_sc, gap in traj:
        buf = torch.full((R, ld), BIG, dtype=torch.float32)
        buf[:, :V] = torch.from_numpy(rows)
        logits = buf.cuda()
        bits_d, table_d, n_multi = _ban_arrays(seqs, V, EOS)
        rc = lib.cap_op_beam_step_processed(_p(state), _p(logits), ld, V, B, K, L, cur_len, EOS, 1.0, _p(anc), L, _p(bits_d), _p(table_d),
                                            n_multi, C.c_float(p), n, vn, V - 3, BOS if vn else -1, _stream())
        assert rc == 0, lib.cap_last_error().decode()
        assert lib.cap_op_beam_peek(_p(state), B, K, L, (cur_len + 1) & 1, _p(run_tokens), _p(run_scores), _p(active), _stream()) == 0
        torch.cuda.synchronize()
        tok, sc = run_tokens.cpu().numpy().astype(np.int64), run_scores.cpu().numpy()
        assert int(active.item()) == 1
        bar = max(8.0 * err + float(np.spacing(np.float32(abs(s)))) for s in want_sc)
        assert gap > 2.0 * bar, (name, cur_len, "the reference's own decision is closer than the bar", gap, bar)
        assert np.array_equal(tok[:, :cur_len + 1], want_tok[:, :cur_len + 1]), (name, cur_len, tok, want_tok)
        for r in range(R):
            e = abs(float(sc[r]) - float(want_sc[r]))
            assert e <= 8.0 * err + float(np.spacing(np.float32(abs(want_sc[r])))), (name, cur_len, r, float(sc[r]), float(want_sc[r]), e, err)
            worst = max(worst, e)
    print(f"\n{name:28s} ref32-vs-ref64 {err:.3e}  bar {8 * err:.3e} + spacing  kernel {worst:.3e}")
