"""GPU: the helper kernels of csrc/elementwise.hip one launch at a time, through their cap_op_* hooks: the decoder / sentence
embeddings, the prompt rows, row compaction, the split-K consumer without LayerNorm, sentence pooling, the patch gather, the class
rows, the 2-D weight conversions, absmax, and the greedy selection on rows without a winner.

Every output lives in a buffer of sentinels (NaN bit patterns for fp32 / bf16 values, the odd word 0x5A5A5A5B for int32 outputs and
G8 containers) with GUARD sentinel elements before and after it; every case compares the WHOLE buffer with the expected bit image,
so what the kernel does not own (rows from *n_live on, pad columns, tokens other than the class token, the guards) must still be
the sentinel.  A refused call must name its launcher and leave every output untouched.

Where the kernel only moves, adds once or encodes (y_out, prompt rows, compaction, the split-K sums, the fmt 0 patch gather, class
rows, conversions, absmax, token selection) the expectation is the exact bit pattern, built on the host by tests/_elementwise_ref.py
and the encodings of tests/_util.py.  The LayerNorm of the embedding kernels is compared bit for bit with cap_op_layernorm on the
host's fp32 sum (both run ln_row of csrc/ln.h without contraction), and against float64 with the bounds this LayerNorm already
has: test_kernels_gpu.py::test_layernorm (2e-5 fp32, 5e-2 bf16) and test_split_gpu.py::test_layernorm_writes_g8 (2e-5, G8 image
within 2^-21 max|f| of the fp32 output).  The two rounding kernels that have no earlier test get derived bounds, written next to
their references in _elementwise_ref.py: mean_pool_normalize64 (the fp32 sequential-sum bound carried through the norm) and
normalise_u8_64 (three fp32 roundings scaled by 1 / std, plus the division's), with store_error for the output type.  No tolerance
in this module is tuned to the kernels; each rounding test prints its worst error / bound ratio (MEASURE) before it asserts.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _elementwise_ref as E
from _util import G8_WSCALE, g8_decode

pytestmark = pytest.mark.gpu

TAG = {"f32": 0, "bf16": 1, "f32s": 2}
DTYPES = ["f32", "bf16", "f32s"]
GUARD = 64                      # sentinel elements on each side of an output (256 bytes, 128 for bf16: alignment is kept)
EPS = 1e-5
INT_MAX = 2 ** 31 - 1
TOL_LN_F32, TOL_LN_BF16, TOL_G8_REL = 2e-5, 5e-2, 2.0 ** -21      # test_layernorm / test_layernorm_writes_g8


@pytest.fixture(scope="module")
def lib():
    from embodied_captioning_amd import _native
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _native.load_library()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ok(lib, rc):
    assert rc == 0, lib.cap_last_error().decode()


def _refused(lib, rc, *needles):
    msg = lib.cap_last_error().decode()
    assert rc != 0, "the call was accepted"
    for n in needles:
        assert n in msg, msg


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _p(t):
    return t.data_ptr() if t is not None else None


class Buf:
    """an output of `shape` elements of `kind` (f32 / bf16 / g8 / i32) filled with its sentinel, guards on both sides"""

    def __init__(self, kind, *shape):
        self.kind, self.shape = kind, shape
        self.n = int(np.prod(shape))
        self.tdt = torch.int16 if kind == "bf16" else torch.int32
        self.raw = torch.full((self.n + 2 * GUARD,), E.sentinel(kind), dtype=self.tdt, device="cuda")
        self.ptr = self.raw.data_ptr() + GUARD * self.raw.element_size()

    def bits(self):
        torch.cuda.synchronize()
        h = self.raw.cpu().numpy()
        s = h.dtype.type(E.sentinel(self.kind))
        assert (h[:GUARD] == s).all() and (h[GUARD + self.n:] == s).all(), "a guard region was written"
        return h[GUARD:GUARD + self.n].reshape(self.shape)

    def untouched(self):
        return bool((self.bits() == E.sentinel(self.kind)).all())

    def values(self):
        """the stored numbers as float64 (a sentinel decodes to NaN or to garbage: compare owned elements only)"""
        b = np.ascontiguousarray(self.bits())
        if self.kind == "f32":
            return b.view(np.float32).astype(np.float64)
        if self.kind == "bf16":
            return torch.from_numpy(b).view(torch.bfloat16).double().numpy()
        return g8_decode(b.view(np.float32)).astype(np.float64)


def _ptr(b):
    return b.ptr if b is not None else None


def _rows_then_sentinel(kind, bits, total_rows):
    """bit image of a buffer of total_rows rows whose first rows hold `bits`, the rest the sentinel"""
    return np.concatenate([bits, np.full((total_rows - bits.shape[0], bits.shape[1]), E.sentinel(kind), dtype=bits.dtype)])


def _same(buf, want, what=""):
    got = buf.bits().reshape(want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} of {want.size} words differ, first at {bad[0].tolist()}: "
                             f"got {int(got[tuple(bad[0])]):#x}, want {int(want[tuple(bad[0])]):#x}")


def _layernorm(lib, dt, y32, gamma_d, beta_d, eps=EPS):
    """cap_op_layernorm on host fp32 rows -> (operand bits, fp32 bits)"""
    M, D = y32.shape
    yd = _dev(y32)
    ot, of = Buf(E.KIND[dt], M, D), Buf("f32", M, D)
    _ok(lib, lib.cap_op_layernorm(TAG[dt], _p(yd), _p(gamma_d), _p(beta_d), eps, ot.ptr, of.ptr, M, D, _stream()))
    return ot.bits().copy(), of.bits().copy()


def _check_ln64(dt, y32, gamma, beta, ot_vals, of_vals, what):
    """the float64 bounds test_layernorm / test_layernorm_writes_g8 hold this LayerNorm to; a None output was not requested"""
    ref = E.layernorm64(y32, gamma, beta, EPS)
    if of_vals is not None:
        err = np.abs(of_vals - ref).max()
        print(f"MEASURE {what} out_f {err:.3e} / {TOL_LN_F32:.0e}")
        assert err < TOL_LN_F32
    if ot_vals is not None:
        if dt == "f32s":
            f = of_vals if of_vals is not None else ref
            slack = 0.0 if of_vals is not None else TOL_LN_F32
            assert np.abs(ot_vals - f).max() <= np.abs(f).max() * TOL_G8_REL + slack
        else:
            err = np.abs(ot_vals - ref).max()
            print(f"MEASURE {what} out_t {err:.3e}")
            assert err < (TOL_LN_F32 if dt == "f32" else TOL_LN_BF16)


def _ln_params(rng, D):
    gamma, beta = rng.standard_normal(D).astype(np.float32), rng.standard_normal(D).astype(np.float32)
    return gamma, beta, _dev(gamma), _dev(beta)


# ---- embed ---------------------------------------------------------------------------------------------------------------
# 128: lanes 32.. idle inside the first vector; 260: one lane of a second vector; 768 / 1024: exactly full vectors; 1032: two lanes
# of a fifth vector; 2560: OPT-2.7b; 3072: the LN_MAXV limit
EMBED_D = [128, 260, 768, 1024, 1032, 2560, 3072]


@pytest.mark.parametrize("D", EMBED_D)
@pytest.mark.parametrize("dt", DTYPES)
def test_embed(lib, dt, D):
    kind = E.KIND[dt]
    V, T, RT = 11, 6, 8
    rng = np.random.default_rng(1000 + D)
    word = (rng.standard_normal((V, D)) * 3 + 1).astype(np.float32)
    pos = rng.standard_normal((T, D)).astype(np.float32)
    gamma, beta, gd, bd = _ln_params(rng, D)
    seq = rng.integers(0, V, (RT, T)).astype(np.int32)            # every token inside [0, V): embed does not clamp
    wd, pd, sd = _dev(word), _dev(pos), _dev(seq)

    def call(R, t, ot, of, y, live=None, n=None):
        return lib.cap_op_embed(TAG[dt], _p(sd), T, t, _p(wd), _p(pd), _p(gd), _p(bd), EPS, _ptr(ot), _ptr(of), _ptr(y), R, D,
                                _p(live), _p(n), _stream())

    if kind == "g8" and D % 8:
        ot, of, y = Buf(kind, 5, D), Buf("f32", 5, D), Buf("f32", 5, D)
        _refused(lib, call(5, 0, ot, of, y), "embed: G8 rows need D % 8 == 0", f"D={D}")
        assert ot.untouched() and of.untouched() and y.untouched()
        return

    for R in (1, 5, 8):                                           # 5: a partial block of four waves; 8: two blocks
        for t in (0, T - 1):
            y32 = E.embed_sum32(word, pos, seq[:R, t], t)
            ref_t, ref_f = _layernorm(lib, dt, y32, gd, bd)
            for has_t, has_f, has_y in ((1, 1, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1)):
                ot, of, y = Buf(kind, R, D) if has_t else None, Buf("f32", R, D) if has_f else None, Buf("f32", R, D) if has_y else None
                _ok(lib, call(R, t, ot, of, y))
                what = f"embed {dt} D={D} R={R} t={t} outputs {has_t}{has_f}{has_y}"
                if y:
                    _same(y, E.encode("f32", y32), what + " y_out vs the host fp32 sum")
                if of:
                    _same(of, ref_f, what + " out_f vs cap_op_layernorm")
                if ot:
                    _same(ot, ref_t, what + " out_t vs cap_op_layernorm")
                _check_ln64(dt, y32, gamma, beta, ot.values() if ot else None, of.values() if of else None, what)

    # RowMap: a permuted live[] and *n < R - compact row c carries the token of row live[c], rows from *n on are not written
    live = np.array([6, 2, 7, 0, 3, 5, 1, 4], dtype=np.int32)
    for n in (5, 1):
        ld_, nd = _dev(live), _dev(np.array([n], dtype=np.int32))
        for t in (0, T - 1):
            y32 = E.embed_sum32(word, pos, seq[live[:n], t], t)
            ref_t, ref_f = _layernorm(lib, dt, y32, gd, bd)
            ot, of, y = Buf(kind, RT, D), Buf("f32", RT, D), Buf("f32", RT, D)
            _ok(lib, call(RT, t, ot, of, y, ld_, nd))
            what = f"embed {dt} D={D} RowMap n={n} t={t}"
            _same(y, _rows_then_sentinel("f32", E.encode("f32", y32), RT), what + " y_out")
            _same(of, _rows_then_sentinel("f32", ref_f, RT), what + " out_f")
            _same(ot, _rows_then_sentinel(kind, ref_t, RT), what + " out_t")


# ---- embed_prompt --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [128, 768])
@pytest.mark.parametrize("dt", DTYPES)
def test_embed_prompt_equals_separate_embed_calls(lib, dt, D):
    kind = E.KIND[dt]
    V, T, RT = 11, 34, 5                                          # seq rows 0..4: row0 <= 2, n_caps <= 3
    rng = np.random.default_rng(2000 + D)
    word = (rng.standard_normal((V, D)) * 3 + 1).astype(np.float32)
    pos = rng.standard_normal((T, D)).astype(np.float32)
    gamma, beta, gd, bd = _ln_params(rng, D)
    seq = rng.integers(0, V, (RT, T)).astype(np.int32)
    wd, pd, sd = _dev(word), _dev(pos), _dev(seq)
    single = []                                                   # per position: (out_t, out_f, y_out) bits of cap_op_embed, rows 0..4
    for t in range(31):
        ot, of, y = Buf(kind, RT, D), Buf("f32", RT, D), Buf("f32", RT, D)
        _ok(lib, lib.cap_op_embed(TAG[dt], _p(sd), T, t, _p(wd), _p(pd), _p(gd), _p(bd), EPS, ot.ptr, of.ptr, y.ptr, RT, D, None, None, _stream()))
        single.append((ot.bits().copy(), of.bits().copy(), y.bits().copy()))
        assert np.array_equal(single[-1][2], E.encode("f32", E.embed_sum32(word, pos, seq[:, t], t)))

    def call(npos, row0, n_caps, ot, of, y, seq_ld=T):
        return lib.cap_op_embed_prompt(TAG[dt], _p(sd), seq_ld, npos, row0, _p(wd), _p(pd), _p(gd), _p(bd), EPS, _ptr(ot), _ptr(of), _ptr(y),
                                       n_caps, D, _stream())

    for n_caps in (1, 3):
        for npos in (1, 5, 31):
            for row0 in (0, 2):
                R = n_caps * npos
                ot, of, y = Buf(kind, R, D), Buf("f32", R, D), Buf("f32", R, D)
                _ok(lib, call(npos, row0, n_caps, ot, of, y))
                for i, b in enumerate((ot, of, y)):
                    want = np.stack([single[p][i][row0 + c] for c in range(n_caps) for p in range(npos)])
                    _same(b, want, f"embed_prompt {dt} D={D} n_caps={n_caps} npos={npos} row0={row0} output {i}")
    # y_out and out_f optional here too
    ot = Buf(kind, 5, D)
    _ok(lib, call(5, 2, 1, ot, None, None))
    _same(ot, np.stack([single[p][0][2] for p in range(5)]), "embed_prompt out_t alone")

    ot, of, y = Buf(kind, 3 * 31, D), Buf("f32", 3 * 31, D), Buf("f32", 3 * 31, D)
    _refused(lib, call(8, 0, 1, ot, of, y, seq_ld=7), "embed_prompt: 8 positions", "do not fit rows of 7 tokens")
    _refused(lib, call(5, -1, 1, ot, of, y), "embed_prompt: 5 positions", "from row -1", "do not fit")
    _refused(lib, call(5, 0, 0, ot, of, y), "embed_prompt: 5 positions of 0 captions", "do not fit")
    assert ot.untouched() and of.untouched() and y.untouched()


def test_embed_prompt_refuses_g8_rows_that_are_no_whole_groups(lib):
    D = 260
    z = torch.zeros(8, D, device="cuda")
    ids = torch.zeros(8, dtype=torch.int32, device="cuda")
    ot, of = Buf("g8", 4, D), Buf("f32", 4, D)
    rc = lib.cap_op_embed_prompt(2, _p(ids), 4, 2, 0, _p(z), _p(z), _p(z), _p(z), EPS, ot.ptr, of.ptr, None, 2, D, _stream())
    _refused(lib, rc, "embed_prompt: G8 rows need D % 8 == 0", "D=260")
    assert ot.untouched() and of.untouched()


# ---- embed_tokens --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,R", [(1, 5), (7, 21)])               # R is no multiple of 4 L: the last block is partial
@pytest.mark.parametrize("D", [128, 260, 768])
@pytest.mark.parametrize("dt", DTYPES)
def test_embed_tokens(lib, dt, D, L, R):
    kind = E.KIND[dt]
    V = 9
    rng = np.random.default_rng(3000 + D + L)
    word = (rng.standard_normal((V, D)) * 3 + 1).astype(np.float32)
    pos = rng.standard_normal((L, D)).astype(np.float32)
    type0 = rng.standard_normal(D).astype(np.float32)
    gamma, beta, gd, bd = _ln_params(rng, D)
    ids = rng.integers(0, V, R).astype(np.int32)
    ids[:5] = [-1, V, INT_MAX, V - 1, 0]                          # clamped to the table ends
    y32 = E.embed_tokens_sum32(word, pos, type0, ids, L)
    assert np.array_equal(y32[:3], np.stack([(word[0] + type0) + pos[0], (word[V - 1] + type0) + pos[1 % L], (word[V - 1] + type0) + pos[2 % L]]))
    ot, of = Buf(kind, R, D), Buf("f32", R, D)
    idd, wd, pd, td = _dev(ids), _dev(word), _dev(pos), _dev(type0)      # (named: a temporary would be freed before the launch)
    rc = lib.cap_op_embed_tokens(TAG[dt], _p(idd), L, _p(wd), _p(pd), _p(td), _p(gd), _p(bd), EPS,
                                 ot.ptr, of.ptr, R, D, V, _stream())
    if kind == "g8" and D % 8:                                    # rows of 260 start in the middle of a group of 8
        _refused(lib, rc, "embed_tokens: G8 rows need D % 8 == 0", f"D={D}")
        assert ot.untouched() and of.untouched()
        return
    _ok(lib, rc)
    ref_t, ref_f = _layernorm(lib, dt, y32, gd, bd)
    what = f"embed_tokens {dt} D={D} L={L}"
    _same(of, ref_f, what + " out_f vs cap_op_layernorm of (word + type0) + pos")
    _same(ot, ref_t, what + " out_t vs cap_op_layernorm")
    _check_ln64(dt, y32, gamma, beta, ot.values(), of.values(), what)


# ---- init_prompt_seq -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,L", [(3, 5), (70, 256)])              # 70 x 256 = 17 920 elements: past one sweep of the 64 x 256 grid
def test_init_prompt_seq(lib, R, L):
    V, pad = 50, 7
    rng = np.random.default_rng(R)
    for rows in (1, R):
        for P in (1, L):
            prompt = rng.integers(-3, V + 3, (rows, P)).astype(np.int32)
            prompt.reshape(-1)[:1] = INT_MAX
            prompt.reshape(-1)[-1:] = -INT_MAX - 1
            if P > 2:
                prompt[:, 1] = [V] * rows
            seq, fin, ln = Buf("i32", R, L), Buf("i32", R), Buf("i32", R)
            prd = _dev(prompt)
            _ok(lib, lib.cap_op_init_prompt_seq(seq.ptr, fin.ptr, ln.ptr, R, L, _p(prd), rows, P, V, pad, _stream()))
            ws, wf, wl = E.init_prompt_seq(R, L, prompt, V, pad)
            what = f"init_prompt_seq R={R} L={L} rows={rows} P={P}"
            _same(seq, ws, what + " seq")
            _same(fin, wf, what + " finished")
            _same(ln, wl, what + " lengths")
            assert ws.min() >= 0 and ws.max() < V


def test_init_prompt_seq_refusals(lib):
    R, L, V = 3, 5, 50
    prompt = _dev(np.ones((R, L), np.int32))
    seq, fin, ln = Buf("i32", R, L), Buf("i32", R), Buf("i32", R)
    for pp, rows, P, v in ((None, 1, 2, V), (_p(prompt), 1, 0, V), (_p(prompt), 1, L + 1, V), (_p(prompt), 2, 2, V), (_p(prompt), 1, 2, 0)):
        rc = lib.cap_op_init_prompt_seq(seq.ptr, fin.ptr, ln.ptr, R, L, pp, rows, P, v, 0, _stream())
        _refused(lib, rc, f"init_prompt_seq: a prompt of {rows} rows x {P} tokens does not fit {R} rows of {L} tokens (vocabulary {v})")
    assert seq.untouched() and fin.untouched() and ln.untouched()


# ---- compact_rows --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 63, 64, 65, 1023, 1024, 1025, 2500])      # wave and 1024-row sweep boundaries, three sweeps
def test_compact_rows(lib, R):
    rng = np.random.default_rng(R)
    odd = rng.integers(0, 2, R)
    odd[rng.integers(0, R, max(R // 5, 1))] = 2                   # any non-zero value is "finished"
    odd[rng.integers(0, R, max(R // 5, 1))] = -1
    patterns = {"open": np.zeros(R), "finished": np.ones(R), "alternating": np.arange(R) % 2, "alternating1": (np.arange(R) + 1) % 2,
                "random": rng.integers(0, 2, R), "sparse": (rng.random(R) < 0.97), "values": odd}
    for name, fin in patterns.items():
        fin = fin.astype(np.int32)
        live, n = Buf("i32", R), Buf("i32", 1)
        find = _dev(fin)
        _ok(lib, lib.cap_op_compact_rows(_p(find), R, live.ptr, n.ptr, _stream()))
        want = np.flatnonzero(fin == 0)
        assert np.array_equal(E.compact_rows(fin), want)
        assert int(n.bits()[0]) == len(want), f"compact_rows R={R} {name}: count"
        _same(live, np.concatenate([want.astype(np.int32), np.full(R - len(want), E.ODD, np.int32)]), f"compact_rows R={R} {name}")


# ---- reduce_bias_act -----------------------------------------------------------------------------------------------------
_RBA = {}


def _rba_inputs(M, N):
    if (M, N) not in _RBA:
        _RBA.clear()                                              # the largest is 34 MB: keep one
        g = torch.Generator().manual_seed(M * 131 + N)
        part = torch.randn(4, M, N, generator=g).numpy()
        bias = torch.randn(N, generator=g).numpy()
        sums = {1: part[0]}
        sums[2] = sums[1] + part[1]
        sums[4] = (sums[2] + part[2]) + part[3]
        _RBA[(M, N)] = (part, bias, _dev(part), _dev(bias), sums)
    return _RBA[(M, N)]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M,N", [(1, 8), (5, 96), (33, 7680), (70, 30720)])      # the last: 537 600 float4s, past the 2048-block grid
def test_reduce_bias_act(lib, dt, M, N):
    kind = E.KIND[dt]
    part, bias, pd, bd, sums = _rba_inputs(M, N)
    assert np.array_equal(sums[4][:1], E.reduce_bias_act32(part[:, :1], None, 0))
    for S in (1, 2, 4):
        for has_bias in (1, 0):
            s = sums[S] + bias[None, :] if has_bias else sums[S]
            for act in (0, 2):
                want = np.maximum(s, np.float32(0)) if act == 2 else s
                if M * N <= 480:
                    assert np.array_equal(want, E.reduce_bias_act32(part[:S], bias if has_bias else None, act))
                out = Buf(kind, M, N)
                _ok(lib, lib.cap_op_reduce_bias_act(TAG[dt], _p(pd), S, _p(bd) if has_bias else None, out.ptr, M, N, act, _stream()))
                _same(out, E.encode(kind, want), f"reduce_bias_act {dt} {M}x{N} S={S} bias={has_bias} act={act}")


@pytest.mark.parametrize("dt", DTYPES)
def test_reduce_bias_act_refusals(lib, dt):
    kind = E.KIND[dt]
    part = torch.randn(2, 3, 12, device="cuda")
    out = Buf(kind, 3, 12)
    _refused(lib, lib.cap_op_reduce_bias_act(TAG[dt], _p(part), 2, None, out.ptr, 3, 6, 0, _stream()), "reduce_bias_act: N must be a multiple of 4")
    assert out.untouched()
    rc = lib.cap_op_reduce_bias_act(TAG[dt], _p(part), 2, None, out.ptr, 3, 12, 0, _stream())
    if kind == "g8":                                              # rows of 12 start in the middle of a group of 8
        _refused(lib, rc, "reduce_bias_act: G8 rows need N % 8 == 0", "N=12")
        assert out.untouched()
    else:
        _ok(lib, rc)
        h = part.cpu().numpy()
        _same(out, E.encode(kind, h[0] + h[1]), f"reduce_bias_act {dt} 3x12")


# ---- mean_pool_normalize -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 7, 128])
@pytest.mark.parametrize("D", [4, 384, 772, 1024])                # one thread; 1.5 waves; 193 threads: one lane of the last wave; every thread
def test_mean_pool_normalize(lib, D, L):
    B = 5
    rng = np.random.default_rng(D * 1000 + L)
    x = (rng.standard_normal((B, L, D)) + 0.5).astype(np.float32)
    x[4] = 0.0                                                    # an all-zero sentence: zeros, not NaN
    lens = np.array([0, 1, L, L + 5, L], dtype=np.int32)          # clamped to [1, L]
    xd, ld_ = _dev(x), _dev(lens)
    out = Buf("f32", B, D)
    _ok(lib, lib.cap_op_mean_pool_normalize(_p(xd), _p(ld_), B, L, D, out.ptr, _stream()))
    got = out.values()
    ref, bound = E.mean_pool_normalize64(x, lens)
    assert np.isfinite(got).all()
    assert not got[4].any(), "the all-zero sentence"
    err = np.abs(got[:4] - ref[:4])
    print(f"MEASURE mean_pool D={D} L={L} max error {err.max():.3e}, worst error / bound {(err / bound[:4]).max():.3f}")
    assert (err <= bound[:4]).all()
    for b in range(B):                                            # a sentence alone has the bits it has in the batch
        one = Buf("f32", 1, D)
        _ok(lib, lib.cap_op_mean_pool_normalize(_p(xd) + b * L * D * 4, _p(ld_) + b * 4, 1, L, D, one.ptr, _stream()))
        _same(one, out.bits()[b:b + 1], f"mean_pool D={D} L={L} sentence {b} alone")


@pytest.mark.parametrize("D", [1028, 6])
def test_mean_pool_normalize_refuses_width(lib, D):
    x, lens, out = torch.zeros(2 * 2 * 1028, device="cuda"), torch.ones(2, dtype=torch.int32, device="cuda"), Buf("f32", 2, D)
    _refused(lib, lib.cap_op_mean_pool_normalize(_p(x), _p(lens), 2, 2, D, out.ptr, _stream()), f"mean_pool: unsupported width {D}")
    assert out.untouched()


# ---- patchify ------------------------------------------------------------------------------------------------------------
PIX_MEAN = np.array([0.48145466, 0.4578275, 0.40821073], dtype=np.float32)
PIX_STD = np.array([0.26862954, 0.26130258, 0.27577711], dtype=np.float32)


def _f3(a):
    return (C.c_float * 3)(*[float(v) for v in a])


def _patchify(lib, dt, pix_ptr, fmt, B, img, ps, Kpad, out):
    mean, std = _f3(PIX_MEAN), _f3(PIX_STD)                       # host pointers: the launcher reads them before it returns
    return lib.cap_op_patchify(TAG[dt], pix_ptr, fmt, B, img, ps, Kpad, out.ptr, C.cast(mean, C.c_void_p), C.cast(std, C.c_void_p), _stream())


def _pads_intact(kind, bits, cols):
    rows, ld = bits.shape
    if kind != "g8":
        return bool((bits[:, cols:] == E.sentinel(kind)).all())
    halves = np.ascontiguousarray(bits).view(np.int16).reshape(rows, ld // 8, 2, 8)
    sent = np.full((rows, ld), E.ODD, np.int32).view(np.int16).reshape(rows, ld // 8, 2, 8)
    pad = np.broadcast_to((np.arange(ld) >= cols).reshape(1, ld // 8, 1, 8), halves.shape)
    return bool((halves[pad] == sent[pad]).all())


@pytest.mark.parametrize("ps", [14, 16, 32])                      # 14: the per-element kernel, 3 ps^2 = 588 is no multiple of 8
@pytest.mark.parametrize("dt", DTYPES)
def test_patchify(lib, dt, ps):
    kind = E.KIND[dt]
    K = 3 * ps * ps
    rng = np.random.default_rng(ps)
    worst = 0.0
    for img in (2 * ps, 3 * ps):
        for B in (1, 3):
            px = (rng.standard_normal((B, 3, img, img)) * 2).astype(np.float32)
            u8 = rng.integers(0, 256, (B, img, img, 3), dtype=np.uint8)
            u8[0, 0, :2] = [[0, 255, 0], [255, 0, 255]]
            pxd, u8d = _dev(px), _dev(u8)
            assert pxd.data_ptr() % 16 == 0 and u8d.data_ptr() % 16 == 0
            gathered = E.patch_gather(px, ps)
            v64, b64 = E.normalise_u8_64(u8, PIX_MEAN, PIX_STD)
            ref, bound = E.patch_gather(v64, ps), E.patch_gather(b64, ps)
            rows = B * (img // ps) ** 2
            for Kpad in ((K + 7) // 8 * 8, (K + 7) // 8 * 8 + 8):
                what = f"patchify {dt} ps={ps} img={img} B={B} Kpad={Kpad}"
                out = Buf(kind, rows, Kpad)
                _ok(lib, _patchify(lib, dt, _p(pxd), 0, B, img, ps, Kpad, out))
                _same(out, E.encode(kind, gathered, Kpad), what + " fmt 0 (a pure gather)")
                out = Buf(kind, rows, Kpad)
                _ok(lib, _patchify(lib, dt, _p(u8d), 1, B, img, ps, Kpad, out))
                assert _pads_intact(kind, out.bits(), K), what + " fmt 1 pad columns"
                err = np.abs(out.values()[:, :K] - ref)
                lim = bound + E.store_error(kind, np.abs(ref) + bound)
                worst = max(worst, float((err / lim).max()))
                assert (err <= lim).all(), what + f" fmt 1: error {err.max():.3e}, worst error / bound {(err / lim).max():.3f}"
    print(f"MEASURE patchify {dt} ps={ps} fmt 1 worst error / bound {worst:.3f}")


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("ps", [16, 32])
@pytest.mark.parametrize("dt", DTYPES)
def test_patchify_kernels_agree_bit_for_bit(lib, dt, ps, fmt):
    """the same pixels at a 16-byte aligned pointer (patchify8_kernel: 8 pixels per thread) and at a pointer 4 bytes (fp32) or
    1 byte (uint8) further (patchify_kernel: one element per thread)"""
    kind = E.KIND[dt]
    B, img = 3, 3 * ps
    K = 3 * ps * ps
    rng = np.random.default_rng(ps + fmt)
    if fmt == 0:
        flat = (rng.standard_normal(B * 3 * img * img) * 2).astype(np.float32)
    else:
        flat = rng.integers(0, 256, B * img * img * 3, dtype=np.uint8)
    a = _dev(flat)
    b = torch.zeros(flat.size + 1, dtype=a.dtype, device="cuda")
    b[1:] = a
    assert a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0
    rows = B * 9
    oa, ob = Buf(kind, rows, K + 8), Buf(kind, rows, K + 8)
    _ok(lib, _patchify(lib, dt, a.data_ptr(), fmt, B, img, ps, K + 8, oa))
    _ok(lib, _patchify(lib, dt, b.data_ptr() + b.element_size(), fmt, B, img, ps, K + 8, ob))
    assert _pads_intact(kind, oa.bits(), K) and not (oa.bits()[:, :K] == E.sentinel(kind)).all()
    _same(ob, oa.bits(), f"patchify {dt} ps={ps} fmt={fmt}: per-element kernel vs patchify8")


@pytest.mark.parametrize("dt", DTYPES)
def test_patchify_refusals(lib, dt):
    kind = E.KIND[dt]
    px = torch.zeros(3 * 32 * 32, device="cuda")
    out = Buf(kind, 4, 776)
    _refused(lib, _patchify(lib, dt, _p(px), 0, 1, 30, 16, 768, out), "patchify: image 30 not divisible by patch 16")
    _refused(lib, _patchify(lib, dt, _p(px), 0, 1, 32, 16, 760, out), "patchify: image 32", "Kpad 760 too small")
    if kind == "g8":                                              # rows of 588 start in the middle of a group of 8
        _refused(lib, _patchify(lib, dt, _p(px), 0, 1, 28, 14, 588, out), "patchify: G8 rows need Kpad % 8 == 0", "Kpad=588")
    assert out.untouched()


# ---- cls_rows ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,D", [(1, 128), (3, 260)])             # B D = 128, 780: neither a multiple of the 256-thread block
def test_cls_rows(lib, B, D):
    tokens = 3
    rng = np.random.default_rng(D)
    cls, pos = rng.standard_normal(D).astype(np.float32), rng.standard_normal((tokens, D)).astype(np.float32)
    X = Buf("f32", B, tokens, D)
    cd, pd = _dev(cls), _dev(pos)
    _ok(lib, lib.cap_op_cls_rows(_p(cd), _p(pd), X.ptr, B, tokens, D, _stream()))
    want = np.full((B, tokens, D), E.NAN32, np.int32)
    want[:, 0] = (cls + pos[0]).view(np.int32)
    _same(X, want, f"cls_rows B={B} D={D}")


# ---- convert2d / convert2d_t ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_convert2d(lib, dt):
    kind = E.KIND[dt]
    rng = np.random.default_rng(5)
    src = (rng.standard_normal((5, 12)) * 4).astype(np.float32)
    dst = Buf(kind, 5, 16)
    sd = _dev(src)
    _ok(lib, lib.cap_op_convert2d(TAG[dt], _p(sd), dst.ptr, 5, 12, 16, 1.0, 0, _stream()))
    _same(dst, E.encode(kind, src, 16), f"convert2d {dt} 5x12 into rows of 16")
    src = (rng.standard_normal((8, 20)) * 4).astype(np.float32)
    dst = Buf(kind, 20, 8)
    sd = _dev(src)
    _ok(lib, lib.cap_op_convert2d(TAG[dt], _p(sd), dst.ptr, 8, 20, 8, 1.0, 1, _stream()))
    _same(dst, E.encode(kind, src.T), f"convert2d_t {dt} 8x20")
    if kind == "g8":
        src = (rng.standard_normal((16, 24)) * 0.02).astype(np.float32)      # weights: 4096 w stays inside fp16's range
        sd = _dev(src)
        for tr in (0, 1):
            dst = Buf(kind, *((24, 16) if tr else (16, 24)))
            _ok(lib, lib.cap_op_convert2d(2, _p(sd), dst.ptr, 16, 24, 16 if tr else 24, G8_WSCALE, tr, _stream()))
            want = (src.T if tr else src) * np.float32(G8_WSCALE)
            _same(dst, E.encode(kind, want), f"convert2d G8 16x24 scale 4096 transposed={tr}")
        dst = Buf(kind, 5, 16)
        _refused(lib, lib.cap_op_convert2d(2, _p(sd), dst.ptr, 5, 12, 12, 1.0, 0, _stream()), "convert2d: G8 rows need ld % 8 == 0", "ld=12")
        _refused(lib, lib.cap_op_convert2d(2, _p(sd), dst.ptr, 5, 12, 5, 1.0, 1, _stream()), "convert2d_t: G8 rows need ld % 8 == 0", "ld=5")
        assert dst.untouched()


# ---- absmax --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 257, 100003])              # one thread; under / over one block; 391 blocks, the last partial
def test_absmax(lib, n):
    rng = np.random.default_rng(n)
    base = rng.standard_normal(n).astype(np.float32)
    at = int(rng.integers(0, n))
    neg, inf, nan, zeros = base.copy(), base.copy(), base.copy(), np.full(n, -0.0, np.float32)
    neg[at] = -77.25                                              # the largest magnitude is negative
    inf[at] = -np.inf
    nan[at] = np.nan
    if n > 1:
        nan[(at + 1) % n] = np.inf
    mz = base.copy()
    mz[::3] = -0.0
    for name, x in (("random", base), ("negative", neg), ("inf", inf), ("nan", nan), ("minus-zero", mz), ("all-minus-zero", zeros)):
        out = Buf("i32", 1)
        out.raw[GUARD] = 0                                        # the caller zeroes the accumulator
        xd = _dev(x)
        _ok(lib, lib.cap_op_absmax(_p(xd), n, out.ptr, _stream()))
        got = int(out.bits().view(np.uint32)[0])
        want = E.absmax_bits(x)
        if want is None:
            assert got > 0x7F800000, f"absmax n={n} {name}: a NaN must stick ({got:#x})"
        else:
            assert got == want, f"absmax n={n} {name}: {got:#x} != {want:#x}"
    out = Buf("i32", 1)                                           # an accumulator that already holds more is kept
    out.raw[GUARD] = 0x7F000000
    xd = _dev(base)
    _ok(lib, lib.cap_op_absmax(_p(xd), n, out.ptr, _stream()))
    assert int(out.bits()[0]) == 0x7F000000


# ---- greedy selection on rows without a winner ----------------------------------------------------------------------------
@pytest.mark.parametrize("mask", [1, 0])
@pytest.mark.parametrize("V", [1, 3, 7, 4103])                    # V < 4: the tail loop alone; 4103: four float4 rounds + a tail of 3
def test_greedy_select_on_degenerate_rows(lib, V, mask):
    """plain, log-prob and vocab forms on rows that have no entry above -inf, ties, or NaN: the token is torch.argmax of the row as
    masked (0 when nothing is above -inf; a NaN stands as -inf: csrc/ops.h), inside [0, V), the same in all three forms.  The
    columns V .. ld of the logits hold 1e30: never read into the selection.  The tokens are not fed to embed."""
    inf, nan = np.float32("inf"), np.float32("nan")
    ld = (V + 3) // 4 * 4 + 4
    eos, pad, max_len, t = V // 2, 0, 4, 0
    rng = np.random.default_rng(V)
    rows = []
    rows.append(np.full(V, -inf))                                 # 0: all -inf
    rows.append(np.full(V, 0.5))                                  # 1: all equal
    r = np.full(V, -inf); r[eos] = 1.0; rows.append(r)            # 2: finite only at EOS
    r = np.full(V, -inf); r[V - 1] = -3.0; rows.append(r)         # 3: finite only at the last index
    rows.append(np.full(V, nan))                                  # 4: all NaN
    r = rng.standard_normal(V); r[0] = nan; rows.append(r)        # 5: NaN first, ordinary after it
    r = np.full(V, -inf); r[V - 1] = nan; rows.append(r)          # 6: NaN last, nothing else above -inf
    r = rng.standard_normal(V); r[rng.integers(0, V)] = inf; rows.append(r)      # 7: +inf wins
    r = rng.standard_normal(V); rows.append(r)                    # 8: an ordinary row
    R = len(rows)
    logits = np.full((R, ld), 1e30, dtype=np.float32)
    logits[:, :V] = np.stack(rows).astype(np.float32)
    want = E.greedy_expected(logits, V, eos, bool(mask))
    assert want[0] == 0 and want[1] == 0 and want[4] == 0 and want[6] == 0
    assert want[2] == (0 if mask else eos)
    ld_ = _dev(logits)
    tokens = {}
    for form in ("plain", "logprob", "vocab"):
        seq, fin, ln = Buf("i32", R, max_len), Buf("i32", R), Buf("i32", R)
        fin.raw[GUARD:GUARD + R] = 0
        lp = torch.zeros(R, max_len, device="cuda")
        scored = torch.zeros(R, dtype=torch.int32, device="cuda")
        acc = torch.zeros(R, ld, device="cuda")
        head = (_p(ld_), ld, V, R, t, max_len, eos, pad, 3 if mask else 0, 0, fin.ptr, None, None, seq.ptr, ln.ptr)
        if form == "plain":
            rc = lib.cap_op_select_logprob(*head, None, max_len, None, _stream())
        elif form == "logprob":
            rc = lib.cap_op_select_logprob(*head, _p(lp), max_len, _p(scored), _stream())
        else:
            rc = lib.cap_op_select_vocab(*head, _p(lp), max_len, _p(scored), _p(acc), ld, _stream())
        _ok(lib, rc)
        s = seq.bits()
        assert (s[:, 0] == E.ODD).all() and (s[:, 2:] == E.ODD).all(), f"{form}: only column t + 1 is written"
        tok = s[:, t + 1].copy()
        assert ((tok >= 0) & (tok < V)).all(), f"{form} V={V}: a token outside the vocabulary: {tok.tolist()}"
        assert np.array_equal(tok, want), f"{form} V={V} mask={mask}: {tok.tolist()} != {want.tolist()}"
        f = fin.bits()
        assert np.array_equal(f != 0, tok == eos), f"{form}: a row finishes exactly when it emits EOS"
        if form == "vocab":
            assert not acc.cpu().numpy()[:, V:].any(), "vocab_acc columns from V on are never touched"
        tokens[form] = tok
    assert np.array_equal(tokens["plain"], tokens["logprob"]) and np.array_equal(tokens["plain"], tokens["vocab"])
