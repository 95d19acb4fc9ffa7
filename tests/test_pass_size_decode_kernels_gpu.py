"""GPU: the pass-size form of the decoder's self-attention step and the head of the compacted greedy loop, bit for bit against
the launches they stand in for (same build, same inputs) - the operations and their order are the same, so the tolerance is 0.

  self-attention  the fused k/v-append step with each partial-sum column finished once per unit (form 2) against the form in which
                  every key sub-lane finishes its own (form 1)
  head            the transform GEMM, its LayerNorm, the vocabulary GEMM and the token selection with the live-row count against
                  the launches over every row

Rows from the live count on must keep what was there before the launch (a sentinel), in every output.
(A pass-size split-K consumer was built and tested here too; it measured behind both existing kernels and was taken out again with
its cases - docs/experiments.md.)
"""
import ctypes as C
import math

import pytest
import torch

from _util import g8_encode

pytestmark = pytest.mark.gpu

TAG = {"f32": 0, "bf16": 1, "f32s": 2}
NAN = float("nan")


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


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _op_dtype(dt):
    return torch.bfloat16 if dt == "bf16" else torch.float32      # (the G8 container is 4 bytes per element)


def _count(n):
    return torch.tensor([n], dtype=torch.int32, device="cuda")


# ---- self-attention: the fused k/v-append step ------------------------------------------------------------------------------
H, KV_LD = 12, 32
SA_KEYS = [1, 8, 9, 16, 17, 20, 32]           # both sides of every key-group boundary (8 keys per group; 1 / 2 / 4 groups per kernel)


@pytest.mark.parametrize("R", [1, 5, 130])
@pytest.mark.parametrize("dt", ["f32s", "bf16"])
def test_self_attention_shared_partial_sums_same_bits(lib, dt, R):
    ta = _op_dtype(dt)                           # cache type: fp32 in split mode, bf16
    g = torch.Generator().manual_seed(R)
    W = H * 64
    bias = (torch.randn(3 * W, generator=g) * 0.5).cuda()
    kc0 = torch.randn(R, H, KV_LD, 64, generator=g).to(ta).cuda()
    vc0 = torch.randn(R, H, KV_LD, 64, generator=g).to(ta).cuda()
    for i, nk in enumerate(SA_KEYS):
        S = (4, 2, 1, 3, 4, 5, 4)[i]                      # the decode GEMMs give up to 4 slices; 5: the loop beyond the unrolled four
        part = torch.randn(S, R, 3 * W, generator=g).cuda()
        for n_live in sorted({0, 1, R - 1, R}):
            live = torch.randperm(R, generator=g).to(torch.int32).cuda()        # compact row c -> the caption's row: shuffled
            count = _count(n_live)
            res = []
            for form in (1, 2):
                kc, vc = kc0.clone(), vc0.clone()
                ctx = torch.full((R, W), 3.0 if dt == "bf16" else 1.0e-30, dtype=ta, device="cuda")     # (split mode: a G8 container)
                _check(lib, lib.cap_op_decode_attention_live(TAG[dt], _p(part), S, _p(bias), 3 * W, 0, 1, _p(kc), _p(vc), KV_LD, nk, _p(ctx), R, H,
                                                             _p(live), _p(count), form, _stream()))
                res.append((ctx, kc, vc))
            where = f"{dt} R={R} keys={nk} S={S} live={n_live}"
            (c1, k1, v1), (c2, k2, v2) = res
            assert _same_bits(c1, c2) and _same_bits(k1, k2) and _same_bits(v1, v2), where
            # context rows from the count on keep the sentinel; the caches change at position nk - 1 of the live captions only
            fresh = torch.full_like(c2, 3.0 if dt == "bf16" else 1.0e-30)
            assert _same_bits(c2[n_live:], fresh[n_live:]), where
            rows = live[:n_live].long()
            touched = torch.zeros(R, H, KV_LD, dtype=torch.bool, device="cuda")
            touched[rows, :, nk - 1] = True
            for new, old in ((k2, kc0), (v2, vc0)):
                same = (_bits(new) == _bits(old)).all(-1)
                assert same[~touched].all(), "cache bytes outside the appended position changed: " + where
                assert not same[touched].any(), where
            if n_live:
                # the appended k / v are the sums asked for: slices in order, bias, through the cache type
                fin = part[0].clone()
                for z in range(1, S):
                    fin = fin + part[z]
                fin = (fin + bias).to(ta)
                assert torch.equal(k2[rows, :, nk - 1], fin[:n_live, W:2 * W].view(n_live, H, 64)), where
                assert torch.equal(v2[rows, :, nk - 1], fin[:n_live, 2 * W:].view(n_live, H, 64)), where
                assert not _same_bits(c2[:n_live], fresh[:n_live]), where


def test_self_attention_form_by_row_count_and_refusals(lib):
    """form 0 picks by row count and gives the same bits; form 2 without the fused k/v append is refused by name"""
    R, nk, S, W = 600, 10, 4, H * 64
    g = torch.Generator().manual_seed(7)
    part, bias = torch.randn(S, R, 3 * W, generator=g).cuda(), torch.randn(3 * W, generator=g).cuda()
    kc0, vc0 = torch.randn(R, H, KV_LD, 64, generator=g).cuda(), torch.randn(R, H, KV_LD, 64, generator=g).cuda()
    res = []
    for form in (0, 1, 2):
        kc, vc, ctx = kc0.clone(), vc0.clone(), torch.zeros(R, W, device="cuda")
        _check(lib, lib.cap_op_decode_attention_live(TAG["f32s"], _p(part), S, _p(bias), 3 * W, 0, 1, _p(kc), _p(vc), KV_LD, nk, _p(ctx), R, H,
                                                     _p(None), _p(None), form, _stream()))
        res.append((ctx, kc, vc))
    for a, b in zip(res[0] + res[1], res[1] + res[2]):
        assert _same_bits(a, b)
    assert lib.cap_op_decode_attention_live(TAG["f32s"], _p(part), S, _p(bias), 3 * W, 0, 0, _p(kc0), _p(vc0), KV_LD, nk, _p(res[0][0]), R, H,
                                            _p(None), _p(None), 2, _stream()) != 0
    assert b"form 2" in lib.cap_last_error()


# ---- the head over the open rows --------------------------------------------------------------------------------------------
def _operand(lib, dt, x):
    """fp32 host rows -> GEMM A operand on the device"""
    if dt == "f32s":
        return torch.from_numpy(g8_encode(x.contiguous().numpy())).cuda()
    return x.to(_op_dtype(dt)).cuda()


def _weight(lib, dt, w):
    if dt != "f32s":
        return w.to(_op_dtype(dt)).cuda()
    src, d = w.cuda(), torch.empty(w.shape, dtype=torch.float32, device="cuda")
    _check(lib, lib.cap_op_convert_weight(TAG[dt], _p(src), _p(d), w.shape[0], w.shape[1], _stream()))
    torch.cuda.synchronize()
    return d


class Head:
    """the decoder head of R rows of width Wd over a vocabulary slice of V columns, as run_step launches it"""
    EOS, PAD, T, MAXLEN = 2, 0, 3, 12

    def __init__(self, lib, dt, R, Wd, V, vocab_tile):
        self.lib, self.dt, self.R, self.Wd, self.V, self.vocab_tile = lib, dt, R, Wd, V, vocab_tile
        g = torch.Generator().manual_seed(R + V)
        self.x = _operand(lib, dt, torch.randn(R, Wd, generator=g))
        self.w_tr = _weight(lib, dt, torch.randn(Wd, Wd, generator=g) / math.sqrt(Wd))
        self.w_vocab = _weight(lib, dt, torch.randn(V, Wd, generator=g) / math.sqrt(Wd))
        self.b_tr, self.b_vocab = torch.randn(Wd, generator=g).cuda(), torch.randn(V, generator=g).cuda()
        self.gamma, self.beta = (torch.rand(Wd, generator=g) + 0.5).cuda(), torch.randn(Wd, generator=g).cuda()

    def run(self, n_live):
        """-> the six buffers the head writes; n_live None: the launches over every row"""
        lib, dt, R, Wd, V = self.lib, self.dt, self.R, self.Wd, self.V
        count = _count(n_live) if n_live is not None else None     # (named: it must outlive the launches)
        n = _p(count)
        dy = torch.full((R, Wd), NAN, device="cuda")
        _check(lib, lib.cap_op_gemm_live(TAG[dt], _p(self.x), _p(self.w_tr), _p(self.b_tr), _p(dy), R, Wd, Wd, 1, 1, 0, n, _stream()))
        x_t = torch.full((R, Wd), 5.0 if dt == "bf16" else 1.0e-30, dtype=_op_dtype(dt), device="cuda")
        x_f = torch.full((R, Wd), NAN, device="cuda")
        _check(lib, lib.cap_op_layernorm_live(TAG[dt], _p(dy), _p(self.gamma), _p(self.beta), C.c_float(1e-12), _p(x_t), _p(x_f), R, Wd, n, _stream()))
        logits = torch.full((R, V), NAN, device="cuda")
        _check(lib, lib.cap_op_gemm_live(TAG[dt], _p(x_t), _p(self.w_vocab), _p(self.b_vocab), _p(logits), R, V, Wd, 0, 1, self.vocab_tile, n, _stream()))
        seq = torch.full((R, self.MAXLEN), -7, dtype=torch.int32, device="cuda")
        fin, lens = torch.zeros(R, dtype=torch.int32, device="cuda"), torch.full((R,), self.MAXLEN, dtype=torch.int32, device="cuda")
        live = torch.arange(R, dtype=torch.int32, device="cuda") if n_live is not None else None
        _check(lib, lib.cap_op_select_logprob(_p(logits), V, V, R, self.T, self.MAXLEN, self.EOS, self.PAD, 0, 0, _p(fin), _p(live), n, _p(seq),
                                              _p(lens), _p(None), 0, _p(None), _stream()))
        torch.cuda.synchronize()
        return dict(dy=dy, x_t=x_t, x_f=x_f, logits=logits, seq=seq, finished=fin, lengths=lens)


def _check_head(h, lives):
    full, none = h.run(None), h.run(0)
    assert torch.isfinite(full["logits"]).all() and (full["seq"][:, Head.T + 1] >= 0).all()
    for n_live in lives:
        got = h.run(n_live)
        for k in got:
            where = f"{k} {h.dt} R={h.R} V={h.V} tile={h.vocab_tile} live={n_live}"
            assert _same_bits(got[k][:n_live], full[k][:n_live]), where
            assert _same_bits(got[k][n_live:], none[k][n_live:]), "rows from the count on were written: " + where
    for k in ("dy", "x_t", "x_f", "logits", "seq"):          # and a launch with nothing live writes nothing: `none` is the sentinel
        assert not _same_bits(none[k], full[k]), k


HEAD_LIVE = [0, 1, 63, 64, 65, 130]


# vocabulary slice: 512 columns and a ragged 500; vocab_tile 0 = the launcher's choice at this size (the register-staged tile), 20 =
# the 256 x 256 kernel the full vocabulary runs on
@pytest.mark.parametrize("V,vocab_tile", [(512, 0), (512, 20), (500, 20), (500, 0)])
@pytest.mark.parametrize("dt", ["f32s", "bf16"])
def test_head_over_the_open_rows(lib, dt, V, vocab_tile):
    _check_head(Head(lib, dt, 130, 256, V, vocab_tile), HEAD_LIVE)


@pytest.mark.parametrize("vocab_tile", [0, 3])
def test_head_over_the_open_rows_fp32(lib, vocab_tile):
    """fp32 mode: the register-staged tiles (0: the launcher's choice at this size) and the 256 x 256 kernel its full-size
    vocabulary GEMM runs on (3) take the count"""
    _check_head(Head(lib, "f32", 130, 256, 512, vocab_tile), HEAD_LIVE)


@pytest.mark.parametrize("dt", ["f32s", "bf16"])
def test_vocabulary_gemm_drops_whole_row_tiles(lib, dt):
    """three 256-row tiles: counts on both sides of a tile boundary change how many tiles the 256 x 256 kernel numbers"""
    _check_head(Head(lib, dt, 520, 256, 512, 20), [255, 256, 257, 512, 520])


@pytest.mark.parametrize("dt", ["f32s", "bf16"])
def test_vocabulary_gemm_tile_ranges_with_a_live_count(lib, dt):
    """The vocabulary GEMM of a 768-row pass: 3 x 120 tiles of 256 x 256 are more than one round of workgroups, so the launcher cuts
    them into a tile range of whole rounds and a tail of half tiles (two launches), numbered in bands because the matrix is wide.
    With a live count both launches number the LIVE tiles: counts on both sides of the row-tile boundaries, and counts that leave
    fewer tiles than the first range holds, against the launch over every row."""
    M, N, K = 768, 120 * 256, 128
    g = torch.Generator().manual_seed(N)
    A = _operand(lib, dt, torch.randn(M, K, generator=g))
    W = _weight(lib, dt, torch.randn(N, K, generator=g) / math.sqrt(K))
    bias = torch.randn(N, generator=g).cuda()

    def run(n_live):
        count = _count(n_live) if n_live is not None else None
        out = torch.full((M, N), NAN, device="cuda")
        _check(lib, lib.cap_op_gemm_live(TAG[dt], _p(A), _p(W), _p(bias), _p(out), M, N, K, 0, 1, 20, _p(count), _stream()))
        torch.cuda.synchronize()
        return out
    full = run(None)
    assert torch.isfinite(full).all()
    for n_live in (0, 1, 255, 257, 512, 513, 767, 768):
        got = run(n_live)
        assert _same_bits(got[:n_live], full[:n_live]), f"{dt} live={n_live}"
        assert torch.isnan(got[n_live:]).all(), f"rows from the count on were written: {dt} live={n_live}"
