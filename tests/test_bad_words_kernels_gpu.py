"""GPU: the banned forms of the two token selections alone (cap_set_bad_words' kernels): greedy_select_banned_kernel through
cap_op_select_banned and the banned beam candidate kernels through cap_op_beam_step_banned, against tests/_bad_words_ref.py.

Greedy: equality is exact - kernel and restatement read the same fp32 values and only compare them.
Beam step: the next running beams of a step are the K best of all K x V continuations by (value desc, flat index asc) - EOS is kept
out of reach and max_len far, so nothing finishes - where value = fp64 log-softmax of the RAW row, banned entries -inf, + the running
score.  Tokens must be identical; scores within the bar of tests/test_beam_search_gpu.py: 8 x the error of the same restatement in
fp32 against fp64 over the case + one fp32 spacing of the score.  The test asserts on the REFERENCE that the decisions it compares
are further apart than twice that bar, so an fp32 rounding cannot flip them."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from _bad_words_ref import banned_mask, beam_log_probs, bitmap_and_table, greedy_choice

pytestmark = pytest.mark.gpu

BIG = 3.0e38          # the columns between V and ld: a kernel that reads them picks them
PAD, EOS, MAX_LEN = 0, 2, 12
VOCABS = (515, 30524, 50272)      # V % 4 = 3 and V % 32 = 3; V % 32 = 28; V % 32 = 0
N_ROWS = 5
TIE_ROW = 3


@pytest.fixture(scope="module")
def lib():
    from embodied_captioning_amd import _native
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _native.load_library()


def _p(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ld(V):
    return (V + 3) // 4 * 4 + 4


def _ban_arrays(lib, seqs, V):
    words = lib.cap_op_ban_words(V)
    assert words * 32 >= V and words % 4 == 0
    bits, table = bitmap_and_table(seqs, V, words, eos=EOS)
    bits_d = torch.from_numpy(bits.view(np.int32)).cuda()
    table_d = torch.from_numpy(table).cuda() if len(table) else None
    return bits_d, table_d, len(table)


@functools.lru_cache(maxsize=None)
def _rows(V):
    """5 fp32 rows and 7 caption histories, computed once per vocabulary and never modified: gaussian rows whose maxima sit at
    0, 31, 32, (a tie of two indices), V - 1."""
    g = torch.Generator().manual_seed(77 + V)
    rows = (torch.randn((N_ROWS, V), generator=g, dtype=torch.float32) * 2.0).numpy()
    for r, i in ((0, 0), (1, 31), (2, 32), (4, V - 1)):
        rows[r, i] = rows[r].max() + 1.0
    a, b = V // 3, V // 3 + 37
    rows[TIE_ROW, a] = rows[TIE_ROW, b] = rows[TIE_ROW].max() + 1.0
    hist = torch.randint(4, V, (7, MAX_LEN), generator=g).numpy().astype(np.int32)
    rows.setflags(write=False)
    hist.setflags(write=False)
    return rows, hist, (a, b)


def _select(lib, V, rows, hist, t, seqs, live=None, finished=(), hist0=0):
    """One launch over the logits rows `rows`; caption c's history is hist[c, :t + 1].  -> seq column t + 1, finished, lengths."""
    n_caps = hist.shape[0]
    R = rows.shape[0]
    buf = torch.full((R, _ld(V)), BIG, dtype=torch.float32)
    buf[:, :V] = torch.from_numpy(np.array(rows))
    logits = buf.cuda()
    seq = torch.full((n_caps, MAX_LEN), -7, dtype=torch.int32)
    seq[:, :t + 1] = torch.from_numpy(np.array(hist[:, :t + 1]))
    seq = seq.cuda()
    fin = torch.zeros(n_caps, dtype=torch.int32)
    for c in finished:
        fin[c] = 1
    fin = fin.cuda()
    lens = torch.full((n_caps,), -1, dtype=torch.int32, device="cuda")
    live_d = n_live = None
    if live is not None:
        live_d = torch.tensor(list(live) + [0] * (R - len(live)), dtype=torch.int32, device="cuda")
        n_live = torch.tensor([len(live)], dtype=torch.int32, device="cuda")
    bits_d, table_d, n_multi = _ban_arrays(lib, seqs, V)
    rc = lib.cap_op_select_banned(_p(logits), logits.shape[1], V, R, t, MAX_LEN, EOS, PAD, _p(fin), _p(live_d), _p(n_live), _p(seq),
                                  _p(lens), _p(bits_d), _p(table_d), n_multi, hist0, _stream())
    assert rc == 0, lib.cap_last_error().decode()
    torch.cuda.synchronize()
    assert torch.equal(seq[:, :t + 1].cpu(), torch.from_numpy(np.array(hist[:, :t + 1])))      # the history is read only
    return seq[:, t + 1].cpu().numpy(), fin.cpu().numpy(), lens.cpu().numpy()


def _want(V, rows, hist, t, seqs, live=None, finished=(), hist0=0):
    n_caps = hist.shape[0]
    caps = list(range(rows.shape[0])) if live is None else list(live)
    tok = np.full(n_caps, -7, dtype=np.int64)
    for c, cap in enumerate(caps):
        tok[cap] = PAD if cap in finished else greedy_choice(rows[c], hist[cap, hist0:t + 1], seqs, eos=EOS)
    return tok


def _top2(row):
    o = np.argsort(-row, kind="stable")
    return int(o[0]), int(o[1])


def _other(tok, V):
    """Another ordinary token than `tok` (the histories hold ids from 4 on)."""
    return (int(tok) - 4 + 1) % (V - 4) + 4


def _single_sets(V):
    rows, hist, (a, b) = _rows(V)
    top = [_top2(r) for r in rows]
    return {
        "edges": [[0], [31], [32], [V - 1]],
        "argmax": [[t[0]] for t in top],
        "argmax_and_runner_up": [[i] for t in top for i in t],
        "tie_lower_banned": [[a]],
        "eos_alone_dropped": [[EOS], [top[0][0]]],
        "everything_but_eos": [[i] for i in range(V) if i != EOS],
    }


@pytest.mark.parametrize("V", VOCABS)
@pytest.mark.parametrize("R", (1, 5))
def test_single_tokens_wherever_they_sit(lib, V, R):
    rows, hist, (a, b) = _rows(V)
    rows, t = rows[:R], 6
    for name, seqs in _single_sets(V).items():
        got, fin, lens = _select(lib, V, rows, hist, t, seqs)
        want = _want(V, rows, hist, t, seqs)
        assert np.array_equal(got, want), (name, got, want)
        raw = [int(np.argmax(r)) for r in rows]
        if name in ("argmax", "argmax_and_runner_up"):
            assert all(g != w for g, w in zip(got[:R], raw)), name                 # the ban bites in every row
        if name == "tie_lower_banned" and R == 5:
            assert raw[TIE_ROW] == a and got[TIE_ROW] == b
        if name == "everything_but_eos":
            # only EOS is left open: it wins everywhere; and with EOS banned as well (below) nothing is left
            assert (got[:R] == EOS).all() and (fin[:R] == 1).all() and (lens[:R] == t + 2).all()
    # every entry banned (EOS through a 2-token sequence that matches every row's history tail): index 0, like torch.argmax
    hist2 = np.array(hist)
    hist2[:, t] = 9
    seqs = [[i] for i in range(V) if i != EOS] + [[9, EOS]]
    got, fin, lens = _select(lib, V, rows, hist2, t, seqs)
    assert np.array_equal(got, _want(V, rows, hist2, t, seqs))
    assert (got[:R] == 0).all() and (got[R:] == -7).all()


@pytest.mark.parametrize("V", VOCABS)
def test_multi_token_sequences_follow_the_history(lib, V):
    rows, hist, _ = _rows(V)
    top = [_top2(r) for r in rows]
    for t in (1, 6, 8):
        h = hist[:N_ROWS]
        match2 = [[int(h[r, t]), top[r][0]] for r in range(N_ROWS)]                         # last token matches
        miss2 = [[_other(h[r, t], V), top[r][0]] for r in range(N_ROWS)]
        sets = {"match2": match2, "miss2": miss2,
                "two_sequences_one_last_token": match2 + [[_other(h[0, t], V), top[0][0]], [int(h[1, t - 1]), int(h[1, t]), top[0][0]]]}
        if t >= 2:
            sets["match3"] = [[int(h[r, t - 1]), int(h[r, t]), top[r][0]] for r in range(N_ROWS)]
            sets["miss3_by_one"] = [[_other(h[r, t - 1], V), int(h[r, t]), top[r][0]] for r in range(N_ROWS)]
            sets["match7"] = [[int(x) for x in h[r, t - 5:t + 1]] + [top[r][0]] for r in range(N_ROWS)]
        if t == 6:      # 8 tokens against a context of 7: skipped, though its first 7 ARE the context
            sets["miss8_one_longer_than_the_context"] = [[int(x) for x in h[r, 0:7]] + [top[r][0]] for r in range(N_ROWS)]
        if t == 8:
            sets["match8"] = [[int(x) for x in h[r, t - 6:t + 1]] + [top[r][0]] for r in range(N_ROWS)]
        else:
            # the context has t + 1 = 2 tokens: a sequence of 4 needs 3 and never matches, though its tail is the context
            sets["longer_than_context"] = [[5, int(h[r, 0]), int(h[r, 1]), top[r][0]] for r in range(N_ROWS)]
        for name, seqs in sets.items():
            got, _, _ = _select(lib, V, rows, hist, t, seqs)
            want = _want(V, rows, hist, t, seqs)
            assert np.array_equal(got, want), (name, t, got, want)
            raw = np.array([tp[0] for tp in top])
            if name.startswith("match"):
                assert (got[:N_ROWS] != raw).all(), (name, t)
            if name.startswith("miss") or name == "longer_than_context":
                assert (got[:N_ROWS] == raw).all(), (name, t)
    # a context that starts at column 3 (BLIP-2: its row holds more than the context): a sequence that would match through column 2
    # does not; from column 2 it is one longer than the context; from column 1 it matches
    t, h0 = 4, 3
    seqs = [[int(hist[r, 2]), int(hist[r, 3]), int(hist[r, 4]), top[r][0]] for r in range(N_ROWS)]
    got, _, _ = _select(lib, V, rows, hist, t, seqs, hist0=h0)
    assert np.array_equal(got, _want(V, rows, hist, t, seqs, hist0=h0)) and (got[:N_ROWS] == [tp[0] for tp in top]).all()
    got, _, _ = _select(lib, V, rows, hist, t, seqs, hist0=2)
    assert np.array_equal(got, _want(V, rows, hist, t, seqs, hist0=2)) and (got[:N_ROWS] == [tp[0] for tp in top]).all()
    got, _, _ = _select(lib, V, rows, hist, t, seqs, hist0=1)
    assert np.array_equal(got, _want(V, rows, hist, t, seqs, hist0=1)) and (got[:N_ROWS] != [tp[0] for tp in top]).all()


@pytest.mark.parametrize("V", VOCABS)
def test_row_map_and_finished_rows(lib, V):
    """Logits row c belongs to caption live[c]: the history, the token and the flags are that caption's; rows from n_live on and
    captions outside the map are untouched; a finished caption emits pad whatever is banned."""
    rows, hist, _ = _rows(V)
    t, live, finished = 6, [5, 2, 6, 0], (2,)
    top = [_top2(r) for r in rows]
    seqs = [[int(hist[cap, t]), top[c][0]] for c, cap in enumerate(live)] + [[top[3][1]]]
    got, fin, lens = _select(lib, V, rows, hist, t, seqs, live=live, finished=finished)
    want = _want(V, rows, hist, t, seqs, live=live, finished=finished)
    assert np.array_equal(got, want), (got, want)
    assert got[2] == PAD and fin[2] == 1 and lens[2] == -1
    assert (got[[1, 3, 4]] == -7).all() and (fin[[1, 3, 4]] == 0).all() and (lens[[1, 3, 4]] == -1).all()
    assert got[5] != top[0][0] and got[6] != top[2][0] and got[0] != top[3][0]


def test_refusals(lib):
    V = 515
    rows, hist, _ = _rows(V)
    logits = torch.zeros((1, _ld(V)), device="cuda")
    seq = torch.zeros((1, MAX_LEN), dtype=torch.int32, device="cuda")
    fin = torch.zeros(1, dtype=torch.int32, device="cuda")
    lens = torch.zeros(1, dtype=torch.int32, device="cuda")
    bits, _, _ = _ban_arrays(lib, [[5]], V)

    def call(bits_=bits, n_multi=0, hist0=0):
        return lib.cap_op_select_banned(_p(logits), logits.shape[1], V, 1, 3, MAX_LEN, EOS, PAD, _p(fin), None, None, _p(seq), _p(lens),
                                        _p(bits_), None, n_multi, hist0, _stream())
    for rc, word in ((call(bits_=None), "ban_bits"), (call(n_multi=1025), "1024"), (call(n_multi=1), "ban_multi"), (call(hist0=5), "hist0")):
        assert rc != 0 and word in lib.cap_last_error().decode(), (word, lib.cap_last_error().decode())


# ------------------------------------------------------------------------------------------------------------------ beam step
BEAM_CASES = [      # name, B, K, V, ld, steps
    ("1x3_v515", 1, 3, 515, 520, 5),
    ("2x5_v515", 2, 5, 515, 520, 5),
    ("2x5_v515_plain_kernel", 2, 5, 515, 517, 4),            # ld % 4 != 0: the plain rows kernel
    ("1x3_v30524_row_in_lds", 1, 3, 30524, 30528, 4),
    ("1x3_v50272_lists_only", 1, 3, 50272, 50276, 4),
]
BOS = 1


def _host_step(run_tok, run_sc, rows, cur_len, seqs, B, K, V, dtype):
    """One step of HF's `_beam_search` when nothing finishes: per item the K best of the K x V continuations by (value desc, flat
    index asc), value = log-softmax(raw row) with the banned entries at -inf + the running score.  -> tokens [R, L], scores [R],
    the source beam of every new beam, and the gap between the K-th and the (K + 1)-th value per item."""
    L = run_tok.shape[1]
    new_tok, new_sc, src, gaps = run_tok.copy(), np.zeros(B * K, dtype=dtype), np.zeros(B * K, dtype=np.int64), []
    for b in range(B):
        vals = np.stack([beam_log_probs(rows[b * K + k], run_tok[b * K + k, :cur_len], seqs, dtype, eos=EOS) + dtype(run_sc[b * K + k])
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


@pytest.mark.parametrize("name,B,K,V,ld,steps", BEAM_CASES, ids=[c[0] for c in BEAM_CASES])
def test_banned_beam_step_against_fp64(lib, name, B, K, V, ld, steps):
    R, L = B * K, MAX_LEN
    g = torch.Generator().manual_seed(5 + V + K)
    nbytes = lib.cap_op_beam_state_bytes(B, K, L)
    state = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device="cuda")
    anc = torch.zeros((2, R, L), dtype=torch.int32, device="cuda")
    run_tokens = torch.zeros((R, L), dtype=torch.int32, device="cuda")
    run_scores = torch.zeros((R,), dtype=torch.float32, device="cuda")
    active = torch.zeros((1,), dtype=torch.int32, device="cuda")
    assert lib.cap_op_beam_init(_p(state), B, K, L, BOS, PAD, EOS, 0, _stream()) == 0

    def peek(par):
        assert lib.cap_op_beam_peek(_p(state), B, K, L, par, _p(run_tokens), _p(run_scores), _p(active), _stream()) == 0
        torch.cuda.synchronize()
        return run_tokens.cpu().numpy().astype(np.int64), run_scores.cpu().numpy(), int(active.item())

    tok, sc, act = peek(1)
    tok64, sc64, sc32 = tok.copy(), sc.astype(np.float64), sc.astype(np.float32)
    err, checks, reordered, bitten = 0.0, [], False, 0
    static = [[int(i)] for i in torch.randint(4, V, (6,), generator=g)] + [[0 + 3], [31], [32], [V - 1]]
    for cur_len in range(1, steps + 1):
        rows = (torch.randn((R, V), generator=g, dtype=torch.float32) * 2.0).numpy()
        rows[:, EOS] = -60.0                                                                   # never a candidate worth keeping
        # the set of this step: the static tokens, and for every beam a sequence made of its LOGICAL history's tail and the token
        # the unbanned step would give it first - 2 tokens, and 3 once the history has them
        seqs = list(static)
        for r in range(R):
            best = int(np.argmax(rows[r]))
            n = 2 if cur_len < 3 or r % 2 == 0 else 3
            seqs.append([int(x) for x in tok64[r, cur_len - (n - 1):cur_len]] + [best])
        seqs.append([int(tok64[0, 0]), 5, 6, 7, 8, 9, 10, int(np.argsort(-rows[0])[1])])        # 8 tokens, matching nowhere
        if cur_len == 1:      # the context is BOS alone: no sequence of two is looked at yet, so step 1 is bitten by single tokens
            seqs += [[int(np.argmax(rows[b * K]))] for b in range(B)]
        free = _host_step(tok64, sc64, rows, cur_len, [], B, K, V, np.float64)
        want_tok, want_sc, src, gap = _host_step(tok64, sc64, rows, cur_len, seqs, B, K, V, np.float64)
        _, sc32_next, _, _ = _host_step(tok64, sc32, rows, cur_len, seqs, B, K, V, np.float32)
        bitten += int(not np.array_equal(free[0], want_tok))
        reordered = reordered or any(int(src[r]) != r % K for r in range(R))
        buf = torch.full((R, ld), BIG, dtype=torch.float32)
        buf[:, :V] = torch.from_numpy(rows)
        logits = buf.cuda()
        bits_d, table_d, n_multi = _ban_arrays(lib, seqs, V)
        rc = lib.cap_op_beam_step_banned(_p(state), _p(logits), ld, V, B, K, L, cur_len, EOS, 1.0, _p(anc), L, 0, 0, _p(bits_d),
                                         _p(table_d), n_multi, _stream())
        assert rc == 0, lib.cap_last_error().decode()
        tok, sc, act = peek((cur_len + 1) & 1)
        assert act == 1
        live = want_sc > -1e8                                   # (step 1: every continuation comes from beam 0, all live)
        e32 = float(np.abs(sc32_next.astype(np.float64) - want_sc)[live].max())
        err = max(err, e32)
        checks.append((cur_len, tok.copy(), sc.copy(), want_tok, want_sc, gap))
        tok64, sc64, sc32 = want_tok, want_sc, sc32_next.astype(np.float32)
    assert reordered, "no step re-ordered the beams: the logical history was never different from the physical row's"
    assert bitten == steps, "the ban changed nothing at some step"
    worst = 0.0
    for cur_len, tok, sc, want_tok, want_sc, gap in checks:
        bar = max(8.0 * err + float(np.spacing(np.float32(abs(s)))) for s in want_sc)
        assert gap > 2.0 * bar, (name, cur_len, "the reference's own decision is closer than the bar", gap, bar)
        assert np.array_equal(tok[:, :cur_len + 1], want_tok[:, :cur_len + 1]), (name, cur_len, tok, want_tok)
        for r in range(R):
            e = abs(float(sc[r]) - float(want_sc[r]))
            assert e <= 8.0 * err + float(np.spacing(np.float32(abs(want_sc[r])))), (name, cur_len, r, float(sc[r]), float(want_sc[r]), e, err)
            worst = max(worst, e)
    print(f"\n{name:28s} ref32-vs-ref64 {err:.3e}  bar {8 * err:.3e} + spacing  kernel {worst:.3e}")
