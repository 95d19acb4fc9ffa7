"""GPU: the sampled form of the greedy token selection alone (cap_set_sampling's kernel, greedy_select_sampled_kernel) through
cap_op_select_sampled, against tests/_sampling_ref.py.

Every row of every case is checked: the token has weight in the fp64 restatement, out_kept equals the restatement's count, and the
draw satisfies the interval rule  cdf64[i - 1] - delta <= (U / 2^64) * total <= cdf64[i] + delta  with
delta = total * ((max|z| + 28) * 2^-24 + 2^-22) + V * 2^-40 (unit: maximal weight = 1) computed from the case's own inputs
(_sampling_ref.delta: division and subtraction rounding on exponents within 40 ln 2 of the maximum, two ulp of expf, the truncation).
The fixtures are chosen, and asserted on the CPU side, so that no top-k boundary holds a tie, every top-p cut lies further than delta
from a flip and no weight sits at the 2^-40 truncation edge: the kept SET must then be the restatement's, exactly.

The distribution test draws 65 536 tokens from one V = 64 row (T = 0.7, top_k = 12, top_p = 0.9: 8 tokens stay, the rarest at
p = 0.035) and requires Pearson's chi-square against the fp64 probabilities to stay below the 1 - 1e-6 quantile (Wilson-Hilferty:
41.87 for 7 degrees of freedom); the draws are a function of the seed, so the statistic is one fixed number."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _sampling_ref as S
from _bad_words_ref import bitmap_and_table
from _repeat_ref import processed_row

pytestmark = pytest.mark.gpu

BIG = 3.0e38          # the columns between V and ld: a kernel that reads them draws them
PAD, EOS, MAX_LEN = 0, 2, 12
VOCABS = ((64, 64), (509, 512), (30524, 30528))
N_ROWS = 8
T_STEP = 4            # the step of the cases: contexts of five tokens
SEED, DRAW = 0x1234_5678_9ABC_DEF1, 3
SETTINGS = {          # name -> (temperature, top_k, top_p)
    "t_only": (0.7, 0, 1.0),
    "k5": (1.0, 5, 1.0),
    "k50_p09": (0.7, 50, 0.9),
    "k0_p08": (1.3, 0, 0.8),
    "k1": (1.0, 1, 1.0),
}
PROCESSED = (1.5, 2)  # the penalty and the n-gram size of the "processed" variant, with a ban set


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


def _history(V, row, seed):
    """A caption's stored context (columns 0 .. T_STEP): `u x top u x` with top = the row's arg-max - the penalty reaches it, and
    n = 2 bans it (it followed an earlier x)."""
    g = np.random.default_rng(seed)
    h = g.integers(3, V, MAX_LEN).astype(np.int32)
    top = int(np.argmax(row))
    u, x = (top + 5) % V, (top + 11) % V
    h[T_STEP - 4:T_STEP + 1] = [u, x, top, u, x]
    return h


def _ban_for(row, V):
    order = np.argsort(-row, kind="stable")
    return [[int(order[1])], [V - 2], [33 % V]]


def _refs(V, row, hist, processed):
    """The restatement of one row under every setting -> {name: ref}; None when a precondition fails for some setting."""
    out = {}
    for name, (T, k, p) in SETTINGS.items():
        if processed:
            ctx = [int(x) for x in hist[:T_STEP + 1]]
            ref = S.reference(row, T, k, p, context=ctx, penalty=PROCESSED[0], ngram=PROCESSED[1], seqs=_ban_for(row, V), eos=EOS)
        else:
            ref = S.reference(row, T, k, p)
        if ref["topk_tie"] or ref["edge"] or not ref["topp_margin"] > 4.0 * S.delta(ref) or ref["kept"] < 1:
            return None
        out[name] = ref
    return out


@functools.lru_cache(maxsize=None)
def _case(V):
    """8 fp32 rows of a vocabulary with their histories and restatements, computed once and never modified.  Candidate rows come from
    consecutive seeds; a row is taken when every setting, plain and processed, meets the preconditions (asserted again by the tests)."""
    rows, hists, plain, proc = [], [], [], []
    seed = 1000 * V
    while len(rows) < N_ROWS:
        seed += 1
        assert seed < 1000 * V + 200, "no fixture rows found"
        g = np.random.default_rng(seed)
        row = (g.standard_normal(V) * 2.0).astype(np.float32)
        hist = _history(V, row, seed)
        a, b = _refs(V, row, hist, False), _refs(V, row, hist, True)
        if a is None or b is None:
            continue
        row.setflags(write=False)
        hist.setflags(write=False)
        rows.append(row); hists.append(hist); plain.append(a); proc.append(b)
    return np.stack(rows), np.stack(hists), plain, proc


def _select(lib, V, ld, rows, hist, setting, processed=False, keys=None, draw=DRAW, live=None, finished=(), seed=SEED, n_caps=None,
            ban_rows=None):
    """One launch over the logits rows -> (seq column T_STEP + 1, out_kept, finished) of every caption."""
    T, k, p = SETTINGS[setting] if isinstance(setting, str) else setting
    R = rows.shape[0]
    n_caps = n_caps or hist.shape[0]
    buf = torch.full((R, ld), BIG, dtype=torch.float32)
    buf[:, :V] = torch.from_numpy(np.array(rows))
    logits = buf.cuda()
    seq = torch.full((n_caps, MAX_LEN), -7, dtype=torch.int32)
    seq[:, :T_STEP + 1] = torch.from_numpy(np.array(hist[:, :T_STEP + 1]))
    seq = seq.cuda()
    fin = torch.zeros(n_caps, dtype=torch.int32)
    for c in finished:
        fin[c] = 1
    fin = fin.cuda()
    lens = torch.full((n_caps,), -1, dtype=torch.int32, device="cuda")
    kept = torch.full((n_caps,), -1, dtype=torch.int32, device="cuda")
    live_d = n_live = None
    if live is not None:
        live_d = torch.tensor(list(live) + [0] * (R - len(live)), dtype=torch.int32, device="cuda")
        n_live = torch.tensor([len(live)], dtype=torch.int32, device="cuda")
    keys_d = None if keys is None else torch.from_numpy(np.asarray(keys, dtype=np.uint64).view(np.int64).copy()).cuda()
    bits_d = table_d = None
    pen, ngram = 1.0, 0
    if processed:
        pen, ngram = PROCESSED
        assert ban_rows is not None
        bits, table = bitmap_and_table(ban_rows, V, _words(V), eos=EOS)
        assert len(table) == 0
        bits_d = torch.from_numpy(bits.view(np.int32)).cuda()
    rc = lib.cap_op_select_sampled(_p(logits), ld, V, R, T_STEP, MAX_LEN, EOS, PAD, _p(fin), _p(live_d), _p(n_live), _p(seq), _p(lens),
                                   _p(bits_d), _p(table_d), 0, 0, C.c_float(pen), ngram, 0, 0, -1, C.c_float(T), k, C.c_float(p),
                                   C.c_uint64(seed), _p(keys_d), draw, _p(kept), _stream())
    assert rc == 0, lib.cap_last_error().decode()
    torch.cuda.synchronize()
    assert torch.equal(seq[:, :T_STEP + 1].cpu(), torch.from_numpy(np.array(hist[:, :T_STEP + 1])))      # the history is read only
    return seq[:, T_STEP + 1].cpu().numpy(), kept.cpu().numpy(), fin.cpu().numpy()


@pytest.mark.parametrize("V,ld", VOCABS)
@pytest.mark.parametrize("processed", (False, True), ids=("plain", "processed"))
@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_every_row_against_the_restatement(lib, V, ld, setting, processed):
    rows, hists, plain, proc = _case(V)
    refs = [r[setting] for r in (proc if processed else plain)]
    T, k, p = SETTINGS[setting]
    for ref in refs:                                     # the preconditions, on the reference side
        assert not ref["topk_tie"] and not ref["edge"] and ref["topp_margin"] > S.delta(ref) and ref["kept"] >= 1
    # one ban set per launch: the processed variant's rows go one launch each, with their own set (the set is the launch's)
    keys = np.arange(N_ROWS, dtype=np.uint64) * np.uint64(0x1_0000_0001) + np.uint64(77)
    if processed:
        got = np.zeros(N_ROWS, dtype=np.int64)
        kept = np.zeros(N_ROWS, dtype=np.int64)
        for r in range(N_ROWS):
            g, kk, _ = _select(lib, V, ld, rows[r:r + 1], hists[r:r + 1], setting, True, keys=keys[r:r + 1], ban_rows=_ban_for(rows[r], V))
            got[r], kept[r] = g[0], kk[0]
    else:
        got, kept, _ = _select(lib, V, ld, rows, hists, setting, keys=keys)
    for r, ref in enumerate(refs):
        U = S.uniform64(SEED, int(keys[r]), DRAW)
        print(f"V={V} {setting} row {r}: token {got[r]} kept {kept[r]} (ref {ref['kept']}) delta {S.delta(ref):.3e} "
              f"topp_margin {ref['topp_margin']:.3e} ref draw {S.draw(ref, U)}")
        assert kept[r] == ref["kept"], (r, kept[r], ref["kept"])
        assert S.check_draw(ref, got[r], U) is None, (r, S.check_draw(ref, got[r], U))
    if k == 1:                                           # the plain kernel's arg-max on these tie-free rows
        for r in range(N_ROWS):
            x = rows[r] if not processed else processed_row(rows[r], [int(t) for t in hists[r][:T_STEP + 1]], PROCESSED[0], PROCESSED[1],
                                                             _ban_for(rows[r], V), EOS)
            assert got[r] == int(np.argmax(x)) and kept[r] == 1


@pytest.mark.parametrize("V,ld", VOCABS)
def test_a_token_depends_on_its_row_key_and_draw_alone(lib, V, ld):
    """The same call twice; a RowMap permutation; finished neighbours; another grid size: the same bits for the same (row, key)."""
    rows, hists, plain, _ = _case(V)
    setting = "k50_p09"
    keys = np.arange(N_ROWS, dtype=np.uint64) + np.uint64(1 << 40)
    base, kept, _ = _select(lib, V, ld, rows, hists, setting, keys=keys)
    again, kept2, _ = _select(lib, V, ld, rows, hists, setting, keys=keys)
    assert np.array_equal(base, again) and np.array_equal(kept, kept2)
    # RowMap: logits row c belongs to caption live[c]; the key is the caption's
    live = [5, 2, 7, 0, 3]
    got, kp, fin = _select(lib, V, ld, rows[live], hists, setting, keys=keys, live=live)
    for c in live:
        assert got[c] == base[c] and kp[c] == kept[c], (c, got, base)
    assert all(got[c] == -7 for c in range(N_ROWS) if c not in live)
    # finished neighbours emit pad and change nothing
    got, _, fin = _select(lib, V, ld, rows, hists, setting, keys=keys, finished=(1, 4, 6))
    for c in range(N_ROWS):
        assert got[c] == (PAD if c in (1, 4, 6) else base[c])
    # another grid: each row alone, with its caption's key
    for c in (0, 3, 7):
        got, kp, _ = _select(lib, V, ld, rows[c:c + 1], hists[c:c + 1], setting, keys=keys[c:c + 1])
        assert got[0] == base[c] and kp[0] == kept[c]
    # keys = NULL is the caption's index; another draw index or seed is another uniform
    got, _, _ = _select(lib, V, ld, rows, hists, setting, keys=None)
    want, _, _ = _select(lib, V, ld, rows, hists, setting, keys=np.arange(N_ROWS, dtype=np.uint64))
    assert np.array_equal(got, want)
    for r in range(N_ROWS):
        assert S.check_draw(plain[r][setting], got[r], S.uniform64(SEED, r, DRAW)) is None


def test_a_row_with_nothing_left_selects_zero_and_nan_stands_as_minus_inf(lib):
    V, ld = 509, 512
    rows = np.full((2, V), -np.inf, dtype=np.float32)
    rows[1, 7] = np.nan
    rows[1, 100] = 0.5
    rows[1, 200] = 0.25
    hist = np.full((2, MAX_LEN), 3, dtype=np.int32)
    got, kept, _ = _select(lib, V, ld, rows, hist, (1.0, 0, 1.0))
    assert got[0] == 0 and kept[0] == 0
    assert got[1] in (100, 200) and kept[1] == 2
    ref = S.reference(rows[1], 1.0, 0, 1.0)
    assert S.check_draw(ref, got[1], S.uniform64(SEED, 1, DRAW)) is None


def test_distribution_chi_square(lib):
    row, T, k, p = S.distribution_fixture()
    ref = S.reference(row, T, k, p)
    assert ref["kept"] == 8 and not ref["topk_tie"] and ref["topp_margin"] > S.delta(ref)
    probs = ref["w"] / ref["total"]
    n_caps = 4096
    rows = np.broadcast_to(row, (n_caps, 64))
    hist = np.full((n_caps, MAX_LEN), 3, dtype=np.int32)
    keys = np.arange(n_caps, dtype=np.uint64)
    counts = np.zeros(64, dtype=np.int64)
    want = np.zeros(64, dtype=np.int64)
    for d in range(16):
        got, _, _ = _select(lib, 64, 64, rows, hist, (T, k, p), keys=keys, draw=d, seed=1234)
        counts += np.bincount(got, minlength=64)
        want += np.bincount(S.draw_many(ref, S.uniform64(1234, keys, d)), minlength=64)
    assert counts.sum() == 65536
    assert counts[probs == 0].sum() == 0, "a token outside the kept set was drawn"
    stat, df = S.chi_square(counts, probs)
    print(f"chi-square {stat:.3f} on {df} degrees of freedom; critical {S.chi_square_quantile(df):.2f}; "
          f"tokens that differ from the restatement's own draws: {np.abs(counts - want).sum() // 2}")
    assert df == 7 and stat < S.chi_square_quantile(df)


def test_refusals_by_message(lib):
    V = 64
    logits = torch.zeros((1, V), dtype=torch.float32, device="cuda")
    seq = torch.zeros((1, MAX_LEN), dtype=torch.int32, device="cuda")
    fin = torch.zeros(1, dtype=torch.int32, device="cuda")
    lens = torch.zeros(1, dtype=torch.int32, device="cuda")

    def call(T=1.0, k=0, p=1.0, logits_=logits, seq_=seq, draw=0):
        rc = lib.cap_op_select_sampled(_p(logits_), V, V, 1, 0, MAX_LEN, EOS, PAD, _p(fin), _p(None), _p(None), _p(seq_), _p(lens), _p(None),
                                       _p(None), 0, 0, C.c_float(1.0), 0, 0, 0, -1, C.c_float(T), k, C.c_float(p), C.c_uint64(0), _p(None),
                                       draw, _p(None), _stream())
        return rc, lib.cap_last_error().decode()

    assert call()[0] == 0
    for T in (0.0, -1.0, float("inf"), float("nan")):
        rc, msg = call(T=T)
        assert rc != 0 and "temperature" in msg, msg
    rc, msg = call(k=-1)
    assert rc != 0 and "top_k" in msg, msg
    for p in (0.0, -0.1, 1.5, float("nan")):
        rc, msg = call(p=p)
        assert rc != 0 and "top_p" in msg, msg
    rc, msg = call(logits_=None)
    assert rc != 0 and "null" in msg, msg
    rc, msg = call(seq_=None)
    assert rc != 0 and "null" in msg, msg
    rc, msg = call(draw=-1)
    assert rc != 0 and "draw" in msg, msg
    torch.cuda.synchronize()
