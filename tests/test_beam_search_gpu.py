"""GPU: the device beam search (csrc/beam.hip: candidate rows from step 2 on, merge, finished pool, both early-stop rules, ancestry
table, loop-still-running flag, finalize) alone, through cap_op_beam_init / _step / _peek / _finalize, on the scripted logits of
tests/_beam_script.py.  After every step the test peeks the running tokens, builds the next rows on the host and uploads them - the
kernels see exactly the fp32 rows the references saw.

References (tests/_beam_ref.py, held to HF's own generate by tests/test_beam_ref_cpu.py):
  tokens, lengths, running tokens, the step at which the flag drops     exactly the fp32 host reference's, which equals the fp64
                                                                        one's on every decision (checked per case on the CPU)
  final and running scores                                              the fp64 host reference, within
        8 x max |fp32 host reference - fp64 host reference| over the case + one fp32 spacing of the score
    (the rule of tests/test_attention_kernels_gpu.py).  Scores that carry a -1e9 mask have fp32 spacing 64: they take no part in
    the case's error and are held to the same formula, whose spacing term is then 64.
The running beams of the max_len step all carry the mask (every candidate stops); which of them come first is decided by the fp32
rounding of -1e9 + score and read by nobody: there the tokens are compared with the fp32 reference alone.

Run with -s for the table of errors and bars (profiles/beam_search_gpu_tolerances.txt is that output)."""
import ctypes as C

import numpy as np
import pytest
import torch

from _beam_ref import MARGIN, bar, beam_search, live, refs
from _beam_script import BY_NAME, CASES, PAD, logits_row

pytestmark = pytest.mark.gpu

GUARD, CANARY = 64, -77
BIG = 3.0e38            # the columns between V and ld: a kernel that reads them picks them


@pytest.fixture(scope="module")
def lib():
    from embodied_captioning_amd import _native
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _native.load_library()


def _p(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _check(lib, rc):
    assert rc == 0, lib.cap_last_error().decode()


def _refused(lib, rc, *words):
    msg = lib.cap_last_error().decode()
    assert rc != 0 and all(w in msg for w in words), (rc, msg)


class Search:
    """One search over a state block of its own.  items: the case's items this search holds (default all)."""

    def __init__(self, lib, case, items=None, anc_ld=None, state=None):
        self.lib, self.case = lib, case
        self.items = list(range(case.B)) if items is None else list(items)
        self.n, self.K, self.L, self.V, self.ld = len(self.items), case.K, case.max_len, case.V, case.row_ld
        self.R = self.n * self.K
        self.anc_ld = self.L if anc_ld is None else anc_ld
        nbytes = lib.cap_op_beam_state_bytes(self.n, self.K, self.L)
        assert nbytes > 0, lib.cap_last_error().decode()
        # the block is the caller's: poison it, so that nothing is read before init wrote it
        self.state = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device="cuda") if state is None else state
        assert self.state.numel() == nbytes
        self.anc_full = torch.full((GUARD + 2 * self.R * self.anc_ld + GUARD,), CANARY, dtype=torch.int32, device="cuda")
        self.anc = self.anc_full[GUARD:GUARD + 2 * self.R * self.anc_ld].view(2, self.R, self.anc_ld)
        self.anc[:, :, 0] = torch.arange(self.R, dtype=torch.int32, device="cuda")        # position 0: every row wrote its own BOS
        self.run_tokens = torch.zeros((self.R, self.L), dtype=torch.int32, device="cuda")
        self.run_scores = torch.zeros((self.R,), dtype=torch.float32, device="cuda")
        self.active = torch.zeros((1,), dtype=torch.int32, device="cuda")
        self.logits = torch.empty((self.R, self.ld), dtype=torch.float32, device="cuda")
        _check(lib, lib.cap_op_beam_init(_p(self.state), self.n, self.K, self.L, case.bos, PAD, case.eos, case.mode, _stream()))
        self.wrote = np.full((self.R, self.L), -1, dtype=np.int64)       # wrote[row][pos]: the token physical row `row` fed at `pos`

    def peek(self, parity):
        _check(self.lib, self.lib.cap_op_beam_peek(_p(self.state), self.n, self.K, self.L, parity, _p(self.run_tokens),
                                                   _p(self.run_scores), _p(self.active), _stream()))
        torch.cuda.synchronize()
        return self.run_tokens.cpu().numpy().copy(), self.run_scores.cpu().numpy().copy(), int(self.active.item())

    def step(self, cur_len, tokens):
        """Feed the rows of `tokens` [R, L] (their first cur_len positions) and run the step that writes position cur_len."""
        c = self.case
        host = np.full((self.R, self.ld), BIG, dtype=np.float32)
        for r in range(self.R):
            host[r, :self.V] = logits_row(c, self.items[r // self.K], tokens[r, :cur_len])
            self.wrote[r, cur_len - 1] = tokens[r, cur_len - 1]
        self.logits.copy_(torch.from_numpy(host))
        _check(self.lib, self.lib.cap_op_beam_step(_p(self.state), _p(self.logits), self.ld, self.V, self.n, self.K, self.L, cur_len,
                                                   c.eos, c.lp, _p(self.anc), self.anc_ld, c.mode, c.min_len, _stream()))
        return self.peek((cur_len + 1) & 1)

    def finalize(self):
        ids = torch.full((self.n, self.L), -5, dtype=torch.int32, device="cuda")
        lens = torch.full((self.n,), -5, dtype=torch.int32, device="cuda")
        sc = torch.full((self.n,), float("nan"), dtype=torch.float32, device="cuda")
        _check(self.lib, self.lib.cap_op_beam_finalize(_p(self.state), self.n, self.K, self.L, _p(ids), _p(lens), _p(sc), _stream()))
        torch.cuda.synchronize()
        return ids.cpu().numpy(), lens.cpu().numpy(), sc.cpu().numpy()

    def check_ancestry(self, cur_len, tokens):
        """After the step at cur_len: the table's new plane names, for every row and position, the physical row that fed the
        token the row's history has there; untouched columns and the bands either side keep the canary."""
        anc = self.anc_full.cpu().numpy()
        assert (anc[:GUARD] == CANARY).all() and (anc[-GUARD:] == CANARY).all()
        new = anc[GUARD:-GUARD].reshape(2, self.R, self.anc_ld)[(cur_len + 1) & 1]
        for r in range(self.R):
            for j in range(min(cur_len, self.anc_ld)):
                a = new[r, j]
                assert r // self.K * self.K <= a < (r // self.K + 1) * self.K, (r, j, a)       # a row of the same item
                assert self.wrote[a, j] == tokens[r, j], (cur_len, r, j, a)
            if cur_len < self.anc_ld:
                assert new[r, cur_len] == r                                                   # the row writes the new position itself
            assert (new[r, cur_len + 1:] == CANARY).all(), (cur_len, r)

    def run(self, on_step=None):
        """The loop as cap_generate runs it: step while the flag is up.  -> list of (cur_len, tokens, scores, active)."""
        tokens, scores, active = self.peek(1)
        assert active == 1 and (tokens[:, 0] == self.case.bos).all()
        assert np.array_equal(scores, np.where(np.arange(self.R) % self.K == 0, np.float32(0), np.float32(-1e9)).astype(np.float32))
        out = []
        for cur_len in range(1, self.L):
            tokens, scores, active = self.step(cur_len, tokens)
            self.check_ancestry(cur_len, tokens)
            out.append((cur_len, tokens, scores, active))
            if on_step:
                on_step(cur_len)
            if not active:
                break
        return out


def _compare(case, trace, final, r32, r64, err, items=None):
    idx = list(range(case.B)) if items is None else list(items)
    K, L = case.K, case.max_len
    ids, lens, sc = final
    worst_final = worst_run = 0.0
    assert len(trace) <= len(r32["steps"])
    for (cur_len, tokens, scores, active), s32, s64 in zip(trace, r32["steps"], r64["steps"]):
        assert cur_len == s32["cur_len"]
        want = s32["run_tokens"][idx].reshape(-1, L)
        assert np.array_equal(tokens, want), (case.name, cur_len, tokens, want)
        if cur_len + 1 < L:
            assert np.array_equal(tokens, s64["run_tokens"][idx].reshape(-1, L))
        ref = s64["run_scores"][idx].reshape(-1)
        for r in range(len(ref)):
            e = abs(float(scores[r]) - float(ref[r]))
            assert e <= bar(err, ref[r]), (case.name, "running score", cur_len, r, float(scores[r]), float(ref[r]), e, bar(err, ref[r]))
            if live(ref[r]):
                worst_run = max(worst_run, e)
        if items is None:
            assert bool(active) == s32["active"] == s64["active"], (case.name, cur_len, active)
    if items is None:
        # the flag drops at the step on which the reference's loop stops, neither earlier nor later
        assert len(trace) == len(r32["steps"]) and trace[-1][0] == r32["stop_cur_len"]
        assert [t[3] for t in trace[:-1]] == [1] * (len(trace) - 1)
    assert np.array_equal(ids, r32["ids"][idx]) and np.array_equal(ids, r64["ids"][idx]), (case.name, ids, r64["ids"][idx])
    assert np.array_equal(lens, r64["lens"][idx])
    for b, i in enumerate(idx):
        e = abs(float(sc[b]) - float(r64["scores"][i]))
        assert e <= bar(err, r64["scores"][i]), (case.name, "final score", i, float(sc[b]), float(r64["scores"][i]), e)
        worst_final = max(worst_final, e)
    return worst_run, worst_final


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_search_matches_the_host_references(lib, case):
    r32, r64, err = refs(case)
    s = Search(lib, case)
    trace = s.run()
    final = s.finalize()
    run_e, fin_e = _compare(case, trace, final, r32, r64, err)
    print(f"\n{case.name:34s} ref32-vs-ref64 {err:.3e}  bar {MARGIN * err:.3e} + spacing  kernel: running {run_e:.3e}  final {fin_e:.3e}  "
          f"steps {len(trace)}  lens {final[1].tolist()}")


@pytest.mark.parametrize("name", ["v5_k3_v64_lp1", "v5_items_differ", "legacy_k2_v1000_min3_lp2", "legacy_all_eos_step2",
                                  "v5_never_ends"])
def test_step_after_the_flag_dropped_changes_nothing_and_init_resets(lib, name):
    case = BY_NAME[name]
    s = Search(lib, case)
    trace = s.run()
    last_len, tokens, scores, active = trace[-1]
    assert active == 0
    final = s.finalize()
    anc_before = s.anc_full.clone()
    state_before = s.state.clone()
    # a further step (the position after the last one, where there is one; else the last one again), with rows that would
    # change everything: EOS towers over the rest
    cur_len = min(last_len + 1, case.max_len - 1)
    s.logits.fill_(0.0)
    s.logits[:, case.eos] = 50.0
    _check(lib, lib.cap_op_beam_step(_p(s.state), _p(s.logits), s.ld, s.V, s.n, s.K, s.L, cur_len, case.eos, case.lp, _p(s.anc),
                                     s.anc_ld, case.mode, case.min_len, _stream()))
    torch.cuda.synchronize()
    assert torch.equal(s.state, state_before), "a step after the flag dropped wrote to the state block"
    assert torch.equal(s.anc_full, anc_before)
    for par in (0, 1):
        t2, s2, a2 = s.peek(par)
        assert a2 == 0
    t2, s2, a2 = s.peek((last_len + 1) & 1)
    assert np.array_equal(t2, tokens) and np.array_equal(s2.view(np.int32), scores.view(np.int32))
    again = s.finalize()
    for x, y in zip(final, again):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))
    # init again on the same block: the same search gives the same result, bit for bit (no stale flag accumulators)
    s3 = Search(lib, case, state=s.state)
    trace3 = s3.run()
    assert len(trace3) == len(trace)
    for (c1, t1, sc1, a1), (c3, t3, sc3, a3) in zip(trace, trace3):
        assert c1 == c3 and a1 == a3 and np.array_equal(t1, t3) and np.array_equal(sc1.view(np.int32), sc3.view(np.int32))
    for x, y in zip(final, s3.finalize()):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))


@pytest.mark.parametrize("name", ["v5_items_differ", "legacy_items_differ", "v5_k5_v64_lp06", "legacy_tie_sums_k4_v64"])
def test_item_alone_has_the_bits_it_has_in_the_batch(lib, name):
    case = BY_NAME[name]
    assert case.B == 3
    r32, r64, err = refs(case)
    K = case.K
    whole = Search(lib, case)
    trace = whole.run()
    ids, lens, sc = whole.finalize()
    for b in range(case.B):
        alone = Search(lib, case, items=[b])
        t1 = alone.run()
        i1, l1, s1 = alone.finalize()
        assert np.array_equal(i1[0], ids[b]) and l1[0] == lens[b] and s1.view(np.int32)[0] == sc.view(np.int32)[b]
        # alone, the loop ends when this item's does; up to there every step's running state is the batch's
        assert len(t1) <= len(trace)
        solo = beam_search(case, np.float32, items=[b])
        assert len(t1) == len(solo["steps"])
        for (c1, tok1, sc1, a1), (c, tok, scs, a) in zip(t1, trace):
            assert np.array_equal(tok1, tok[b * K:(b + 1) * K])
            assert np.array_equal(sc1.view(np.int32), scs[b * K:(b + 1) * K].view(np.int32))
        _compare(case, t1, (i1, l1, s1), r32, r64, err, items=[b])


@pytest.mark.parametrize("name", ["v5_k3_v64_lp1", "legacy_k3_v64_min0_lp06"])
def test_ancestry_table_narrower_than_the_sequences(lib, name):
    """anc_ld < max_len: columns from anc_ld on do not exist - the copy stops there and the band behind the table survives."""
    case = BY_NAME[name]
    r32, r64, err = refs(case)
    s = Search(lib, case, anc_ld=4)
    trace = s.run()
    _compare(case, trace, s.finalize(), r32, r64, err)


def test_without_an_ancestry_table(lib):
    case = BY_NAME["v5_k2_v1000_lp06"]
    r32, r64, err = refs(case)
    s = Search(lib, case)
    tokens, _, _ = s.peek(1)
    trace = []
    for cur_len in range(1, case.max_len):
        host = np.full((s.R, s.ld), BIG, dtype=np.float32)
        for r in range(s.R):
            host[r, :s.V] = logits_row(case, r // s.K, tokens[r, :cur_len])
        s.logits.copy_(torch.from_numpy(host))
        _check(lib, lib.cap_op_beam_step(_p(s.state), _p(s.logits), s.ld, s.V, s.n, s.K, s.L, cur_len, case.eos, case.lp, None, 0,
                                         case.mode, case.min_len, _stream()))
        tokens, scores, active = s.peek((cur_len + 1) & 1)
        trace.append((cur_len, tokens, scores, active))
        if not active:
            break
    _compare(case, trace, s.finalize(), r32, r64, err)
    full = s.anc_full.cpu().numpy()[GUARD:-GUARD].reshape(2, s.R, s.anc_ld)
    assert (full[:, :, 1:] == CANARY).all()                         # the table was never passed


def test_argument_checks_fail_by_name(lib):
    """Only arguments that are refused before any launch."""
    B, K, L, V, ld = 2, 3, 8, 64, 64
    n = lib.cap_op_beam_state_bytes(B, K, L)
    assert n > 0
    for bad in ((B, 0, L), (B, 9, L), (0, K, L), (B, K, 1)):
        assert lib.cap_op_beam_state_bytes(*bad) == 0
        assert "cap_op_beam_state_bytes" in lib.cap_last_error().decode()
    st = torch.zeros(n, dtype=torch.uint8, device="cuda")
    x = torch.zeros((B * K, ld), dtype=torch.float32, device="cuda")
    anc = torch.zeros((2, B * K, L), dtype=torch.int32, device="cuda")
    ids = torch.zeros((B, L), dtype=torch.int32, device="cuda")
    rt = torch.zeros((B * K, L), dtype=torch.int32, device="cuda")
    rs = torch.zeros((B * K,), dtype=torch.float32, device="cuda")
    ac = torch.zeros((1,), dtype=torch.int32, device="cuda")
    S = _stream()
    _refused(lib, lib.cap_op_beam_init(None, B, K, L, 2, 0, 1, 0, S), "cap_op_beam_init", "state")
    _refused(lib, lib.cap_op_beam_init(_p(st), B, 0, L, 2, 0, 1, 0, S), "cap_op_beam_init", "K = 0")
    _refused(lib, lib.cap_op_beam_init(_p(st), B, 9, L, 2, 0, 1, 0, S), "cap_op_beam_init", "K = 9")
    _refused(lib, lib.cap_op_beam_init(_p(st), B, K, L, 2, 0, 1, 2, S), "cap_op_beam_init", "mode")

    def step(state=st, logits=x, ld_=ld, V_=V, K_=K, cur=1, anc_=anc, anc_ld=L, mode=0):
        return lib.cap_op_beam_step(_p(state), _p(logits), ld_, V_, B, K_, L, cur, 1, 1.0, _p(anc_), anc_ld, mode, 0, S)

    _refused(lib, step(state=None), "cap_op_beam_step", "state")
    _refused(lib, step(logits=None), "cap_op_beam_step", "logits")
    _refused(lib, step(K_=0), "cap_op_beam_step", "K = 0")
    _refused(lib, step(K_=9), "cap_op_beam_step", "K = 9")
    _refused(lib, step(ld_=V - 1), "cap_op_beam_step", "ld")
    _refused(lib, step(cur=0), "cap_op_beam_step", "cur_len = 0")
    _refused(lib, step(cur=-1), "cap_op_beam_step", "cur_len")
    _refused(lib, step(cur=L), "cap_op_beam_step", "cur_len = %d" % L)
    _refused(lib, step(anc_ld=0), "cap_op_beam_step", "anc_ld")
    _refused(lib, step(mode=7), "cap_op_beam_step", "mode")
    _refused(lib, lib.cap_op_beam_finalize(None, B, K, L, _p(ids), None, None, S), "cap_op_beam_finalize", "state")
    _refused(lib, lib.cap_op_beam_finalize(_p(st), B, K, L, None, None, None, S), "cap_op_beam_finalize", "out_ids")
    _refused(lib, lib.cap_op_beam_finalize(_p(st), B, 9, L, _p(ids), None, None, S), "cap_op_beam_finalize", "K = 9")
    _refused(lib, lib.cap_op_beam_peek(None, B, K, L, 0, _p(rt), _p(rs), _p(ac), S), "cap_op_beam_peek", "state")
    _refused(lib, lib.cap_op_beam_peek(_p(st), B, K, L, 0, None, _p(rs), _p(ac), S), "cap_op_beam_peek", "null")
    _refused(lib, lib.cap_op_beam_peek(_p(st), B, K, L, 0, _p(rt), None, _p(ac), S), "cap_op_beam_peek", "null")
    _refused(lib, lib.cap_op_beam_peek(_p(st), B, K, L, 0, _p(rt), _p(rs), None, S), "cap_op_beam_peek", "null")
    _refused(lib, lib.cap_op_beam_peek(_p(st), B, K, L, 2, _p(rt), _p(rs), _p(ac), S), "cap_op_beam_peek", "parity")
    _refused(lib, lib.cap_op_beam_peek(_p(st), B, 0, L, 0, _p(rt), _p(rs), _p(ac), S), "cap_op_beam_peek", "K = 0")
    torch.cuda.synchronize()
    assert int(st.sum()) == 0 and int(anc.sum()) == 0, "a refused call wrote"
