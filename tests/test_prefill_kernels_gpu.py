"""GPU: the kernels that run once per prompt pass, one launch (or kernel pair) at a time through entry points of their own -
cap_op_prefill_self_attention, cap_op_opt_prefill_inputs, cap_op_opt_token_inputs, cap_op_rows_broadcast,
cap_op_dequant_i8_rowmajor, cap_op_scale_cols.  Before this file only whole cap_generate* calls on tiny models reached them.

Every output buffer starts as a sentinel (NaN words; the odd word 0x5A5A5A5B for the G8 containers compared as bit images; for
the K/V caches, which are read-modify-write state, the random bytes they held before) and is larger than what the kernel owns:
what it owns must be finite afterwards and every other byte unchanged.  A refused call names its launcher and writes nothing.

A. Prefill self-attention (attention.hip: prefill_kv_append_kernel, prefill_self_attention_kernel).
   Reference: float64 causal attention (scale 0.125) over q | k | v = (split-K slices summed in order + bias) in fp32, rounded
   through the cache type - the operands as the kernel stores them.  Bound: TOL_ATT of test_small_kernels_gpu.py, 1e-5 for an
   fp32 or G8 context and 2e-2 for a bf16 one; not a new number, because every row is also required to be BIT-EQUAL to the
   single step's output (cap_op_decode_attention_fused, append_kv, n_keys = p + 1), which that file holds to the same bound on
   the same input distribution.  Caches: torch.equal with the rounded sums at the written positions, the old bytes elsewhere.
   Chunks: one call over a + b captions against two calls - bytes.
   Measured on the MI355X, worst context error over the geometries: f32 2.424e-06, f32s 2.209e-06, bf16 1.561e-02.
B. OPT inputs and rows_broadcast (attention.hip).  One fp32 add, or a copy: tolerance 0 against torch in fp32 on the host.  A G8
   copy is compared with the bit image _elementwise_ref.encode builds and held to _elementwise_ref.store_error.
C. The int8 tiled route of opt_gemm (gemm_skinny.hip: dequant_i8_rowmajor_kernel, scale_cols_kernel).  The unpacked bf16
   integers are exact (torch.equal with _util.i8_unpack), scale_cols is one fp32 multiply (tolerance 0 against torch).  The
   route - pack, dequant, cap_op_gemm (bf16 operands, fp32 output, the launcher's own tile), scale_cols - against
   exact = (a64 @ q64^T) * scale with the bound test_blip2_int8_gpu.py::test_int8_weight_stream_gemm_against_integer_arithmetic
   holds the weight-streaming kernel to: |got - exact| <= mag 1e-6 + 1e-6, mag = (|a| @ |q|^T) * scale (fp32 accumulation of
   exact products).  Both routes' worst err / mag are printed; docs/experiments.md has the MI355X figures.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _elementwise_ref as E
from _util import NAN, att_dtype, check_rc, cur_stream, finish32, g8_decode, i8_pack, i8_pack_host, i8_unpack, nan_buf, nan_f32
from _util import operand_values, same_bits
from test_small_kernels_gpu import TOL_ATT

gpu = pytest.mark.gpu          # every test but the pure-Python check of the case list, which runs without a GPU too

TAG = {"f32": 0, "bf16": 1, "f32s": 2}
DTYPES = ["f32", "f32s", "bf16"]
TOL_CTX = {"f32": TOL_ATT["f32s"], "f32s": TOL_ATT["f32s"], "bf16": TOL_ATT["bf16"]}      # an fp32 or G8 context | a bf16 one
PREFILL_MAX_POS = 31


@pytest.fixture(scope="module")
def lib():
    from embodied_captioning_amd import _native
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _native.load_library()


def _vp(t, byte_offset=0):
    return C.c_void_p(t.data_ptr() + byte_offset) if t is not None else None


def _refused(lib, rc, needle, why):
    msg = lib.cap_last_error().decode()
    assert rc != 0, "accepted: " + why
    assert needle in msg, (why, msg)


# ---- A. prefill self-attention ------------------------------------------------------------------------------------------------
NPOS = [1, 8, 9, 16, 17, 31]          # both sides of the wave unit's n_keys <= 8 and <= 16 branches, and PREFILL_MAX_POS
# (n_caps, npos, H, S, part_ld - 3 H 64, kv_ld - npos, row0)
GEOMS = [
    (1, 3, 1, 2, 0, 0, 0),            # 3 units: a quarter of an attention workgroup, 24 lanes of the append kernel's first wave
    (3, 1, 3, 1, 8, 3, 2),            # one position per caption: every unit is another caption
    (2, 8, 3, 3, 0, 3, 0),            # 48 units: a second, half-filled workgroup of the append kernel
    (3, 9, 3, 4, 8, 0, 2),            # 81 units
    (2, 16, 3, 2, 8, 0, 0),           # 96 units: whole workgroups of both kernels
    (2, 17, 3, 1, 0, 3, 2),           # 102 units
    (3, 31, 3, 4, 8, 3, 0),           # 279 units
    (2, 5, 12, 3, 0, 3, 2),           # the production head count: 120 units
]


def test_prefill_geometry_list_covers_every_listed_value():
    assert {g[1] for g in GEOMS} >= set(NPOS) and max(g[1] for g in GEOMS) == PREFILL_MAX_POS
    assert {g[3] for g in GEOMS} == {1, 2, 3, 4}
    assert {g[4] for g in GEOMS} == {0, 8} and {g[5] for g in GEOMS} == {0, 3} and {g[6] for g in GEOMS} == {0, 2}
    units = [g[0] * g[1] * g[2] for g in GEOMS]
    assert any(u % 4 for u in units) and any(u > 32 and u % 32 for u in units) and any(u % 32 == 0 for u in units)
    assert (1, 3, 1) in {g[:3] for g in GEOMS} and {g[2] for g in GEOMS} == {1, 3, 12}
    # every branch of the wave unit (key counts 1..8, 9..16, 17..) in a call that is split into chunks too
    assert {min((g[1] - 1) // 8, 2) for g in GEOMS if g[0] >= 2} == {0, 1, 2}


class Prefill:
    """operands of one prefill self-attention call on the host, its float64 context and the caches it must leave"""

    def __init__(self, dt, geom, seed):
        self.dt, self.geom = dt, geom
        n_caps, npos, H, S, ld_pad, kv_pad, row0 = geom
        self.n_caps, self.npos, self.H, self.S, self.row0 = n_caps, npos, H, S, row0
        self.Dh, self.Rp, self.part_ld, self.kv_ld, self.caps = H * 64, n_caps * npos, 3 * H * 64 + ld_pad, npos + kv_pad, row0 + n_caps + 1
        ta, Dh = att_dtype(dt), self.Dh
        g = torch.Generator().manual_seed(seed)
        self.part = torch.randn(S, self.Rp, self.part_ld, generator=g)
        self.bias = torch.randn(3 * Dh, generator=g) * 0.5
        self.kc = torch.randn(self.caps, H, self.kv_ld, 64, generator=g).to(ta)
        self.vc = torch.randn(self.caps, H, self.kv_ld, 64, generator=g).to(ta)
        fin = finish32(self.part[:, :, :3 * Dh], self.bias).to(ta)                        # the operands as stored
        q, k, v = (fin[:, i * Dh:(i + 1) * Dh].reshape(n_caps, npos, H, 64) for i in range(3))
        self.want_k, self.want_v = self.kc.clone(), self.vc.clone()
        self.want_k[row0:row0 + n_caps, :, :npos] = k.permute(0, 2, 1, 3)
        self.want_v[row0:row0 + n_caps, :, :npos] = v.permute(0, 2, 1, 3)
        s = torch.einsum("cphd,cjhd->chpj", q.double(), k.double()) * 0.125
        s = s.masked_fill(torch.arange(npos)[None, :] > torch.arange(npos)[:, None], float("-inf"))      # row (c, p): keys 0..p of caption c
        self.ctx64 = torch.einsum("chpj,cjhd->cphd", torch.softmax(s, -1), v.double()).reshape(self.Rp, Dh)
        self.part_d, self.bias_d = self.part.cuda(), self.bias.cuda()

    def launch(self, lib, d_part, d_k, d_v, d_out, caps, first, **over):
        a = dict(S=self.S, part_ld=self.part_ld, kv_ld=self.kv_ld, npos=self.npos, H=self.H, n_caps=caps, row0=first, tag=TAG[self.dt],
                 part=_vp(d_part), bias=_vp(self.bias_d), k=_vp(d_k), v=_vp(d_v), out=_vp(d_out))
        a.update(over)
        rc = lib.cap_op_prefill_self_attention(a["tag"], a["part"], a["S"], a["bias"], a["part_ld"], a["k"], a["v"], a["kv_ld"], a["out"],
                                               a["n_caps"], a["npos"], a["row0"], a["H"], cur_stream())
        torch.cuda.synchronize()
        return rc

    def fresh(self, rows):
        return self.kc.cuda(), self.vc.cuda(), nan_buf(self.dt, rows + 2, self.Dh)


_WORST_CTX = {}


@gpu
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "caps{}-pos{}-H{}-S{}-ld{}-kv{}-row{}".format(*g))
@pytest.mark.parametrize("dt", DTYPES)
def test_prefill_self_attention(lib, dt, geom):
    x = Prefill(dt, geom, 1000 + GEOMS.index(geom))
    n_caps, npos, H, S, row0, Rp, Dh = x.n_caps, x.npos, x.H, x.S, x.row0, x.Rp, x.Dh
    kd, vd, out = x.fresh(Rp)
    sentinel = out.clone()
    check_rc(lib, x.launch(lib, x.part_d, kd, vd, out, n_caps, row0))
    # 1. the context against float64; rows past n_caps * npos keep the sentinel
    got = operand_values(dt, out[:Rp].contiguous())
    err = (got - x.ctx64).abs().max().item()
    _WORST_CTX[dt] = max(_WORST_CTX.get(dt, 0.0), err)
    print(f"MEASURE prefill context {dt} {geom}: err {err:.3e} (bound {TOL_CTX[dt]:.0e}); worst so far for {dt} {_WORST_CTX[dt]:.3e}")
    assert torch.isfinite(got).all() and same_bits(out[Rp:], sentinel[Rp:])
    assert err < TOL_CTX[dt]
    # 2. the caches: the rounded sums at positions 0 .. npos - 1 of captions row0 .. row0 + n_caps - 1, the old bytes everywhere else
    assert torch.equal(kd.cpu(), x.want_k) and torch.equal(vd.cpu(), x.want_v)
    # 3. the single steps: npos fused launches over the n_caps captions, the caches advanced by row0 captions
    ks, vs, _ = x.fresh(0)
    off = row0 * H * x.kv_ld * 64 * ks.element_size()
    steps = out[:Rp].view(n_caps, npos, Dh)
    for p in range(npos):
        part_p = x.part_d[:, p::npos].contiguous()                                       # rows c * npos + p
        assert part_p.shape[1] == n_caps
        out_p = nan_buf(dt, n_caps, Dh)
        check_rc(lib, lib.cap_op_decode_attention_fused(TAG[dt], _vp(part_p), S, _vp(x.bias_d), x.part_ld, 0, 1, _vp(ks, off), _vp(vs, off), None, 0,
                                                        1, x.kv_ld, p + 1, _vp(out_p), n_caps, H, 0, cur_stream()))
        torch.cuda.synchronize()
        assert same_bits(out_p, steps[:, p].contiguous()), f"position {p}"
    assert same_bits(ks, kd) and same_bits(vs, vd)
    # 4. chunks of captions, as run_prefill calls it when the workspace does not hold the batch
    if n_caps >= 2:
        a = n_caps // 2
        kb, vb, out_a = x.fresh(a * npos)
        out_b = nan_buf(dt, (n_caps - a) * npos + 2, Dh)
        check_rc(lib, x.launch(lib, x.part_d[:, :a * npos].contiguous(), kb, vb, out_a, a, row0))
        check_rc(lib, x.launch(lib, x.part_d[:, a * npos:].contiguous(), kb, vb, out_b, n_caps - a, row0 + a))
        assert same_bits(torch.cat([out_a[:a * npos], out_b[:(n_caps - a) * npos]]), out[:Rp])
        assert same_bits(out_a[a * npos:], sentinel[:2]) and same_bits(out_b[(n_caps - a) * npos:], sentinel[:2])
        assert same_bits(kb, kd) and same_bits(vb, vd)


@gpu
@pytest.mark.parametrize("dt", DTYPES)
def test_prefill_self_attention_refusals_name_the_launcher_and_write_nothing(lib, dt):
    x = Prefill(dt, (2, 5, 3, 2, 8, 3, 1), 7)
    kd, vd, out = x.fresh(x.Rp)
    k0, v0, out0 = kd.clone(), vd.clone(), out.clone()

    def attempt(why, needle, **over):
        _refused(lib, x.launch(lib, x.part_d, kd, vd, out, x.n_caps, x.row0, **over), needle, why)
        assert "prefill_self_attention" in lib.cap_last_error().decode(), why
        assert same_bits(kd, k0) and same_bits(vd, v0) and same_bits(out, out0), why

    attempt("npos = 0", "positions", npos=0)
    attempt("npos = 32", "positions", npos=32, kv_ld=40)
    attempt("npos > kv_ld", "positions", kv_ld=x.npos - 1)
    attempt("S = 0", "split-K slices", S=0)
    attempt("S = 5", "split-K slices", S=5)
    attempt("part_ld % 4", "split-K slices", part_ld=x.part_ld + 2)
    attempt("part_ld < 3 H 64", "split-K slices", part_ld=3 * x.Dh - 4)
    attempt("n_caps = 0", "positions", n_caps=0)
    attempt("row0 = -1", "positions", row0=-1)
    attempt("H = 0", "positions", H=0)
    for name in ("part", "bias", "k", "v", "out"):
        attempt("null " + name, "null", **{name: None})
    check_rc(lib, x.launch(lib, x.part_d, kd, vd, out, x.n_caps, x.row0))          # and the base call is taken
    assert torch.equal(kd.cpu(), x.want_k) and torch.isfinite(operand_values(dt, out[:x.Rp].contiguous())).all()


# ---- B. OPT inputs and rows_broadcast ----------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("B,nq,T", [(1, 1, 8), (3, 5, 100), (3, 32, 2560)])       # the last: 253 440 elements, four sweeps of the 256 x 256 grid
def test_opt_prefill_inputs(lib, B, nq, T):
    g = torch.Generator().manual_seed(B * 1000 + nq)
    V, bos = 7, 3                                                                  # bos neither row 0 nor the last
    proj, tok, pos = torch.randn(B * nq, T, generator=g), torch.randn(V, T, generator=g), torch.randn(nq + 3, T, generator=g)
    want = torch.empty(B, nq + 1, T)
    want[:, :nq] = proj.view(B, nq, T) + pos[2:nq + 2][None]                       # HF's offset of 2: row j gets position row j + 2
    want[:, nq] = tok[bos] + pos[nq + 2]
    rows = B * (nq + 1)
    x = nan_f32(rows + 2, T)
    pd, td, sd = proj.cuda(), tok.cuda(), pos.cuda()
    check_rc(lib, lib.cap_op_opt_prefill_inputs(_vp(pd), _vp(td), _vp(sd), _vp(x), B, nq, T, bos, cur_stream()))
    torch.cuda.synchronize()
    assert torch.equal(x[:rows].cpu(), want.view(rows, T)) and torch.isnan(x[rows:]).all()
    for why, args in [("null proj", (None, _vp(td), _vp(sd), _vp(x), B, nq, T, bos)), ("null x", (_vp(pd), _vp(td), _vp(sd), None, B, nq, T, bos)),
                      ("B = 0", (_vp(pd), _vp(td), _vp(sd), _vp(x), 0, nq, T, bos)), ("bos = -1", (_vp(pd), _vp(td), _vp(sd), _vp(x), B, nq, T, -1))]:
        before = x.clone()
        _refused(lib, lib.cap_op_opt_prefill_inputs(*args, cur_stream()), "cap_op_opt_prefill_inputs", why)
        torch.cuda.synchronize()
        assert same_bits(x, before), why


SEQ_LD = 9


@gpu
@pytest.mark.parametrize("cur", [0, 5, SEQ_LD - 1])
@pytest.mark.parametrize("B,T", [(1, 8), (5, 100), (70, 2560)])                   # the last: 179 200 elements, eleven sweeps of the 64 x 256 grid
def test_opt_token_inputs(lib, B, T, cur):
    g = torch.Generator().manual_seed(B * 100 + cur)
    V = B + 5
    room = torch.randn(V + 2, T, generator=g)                                      # the table is rows 1 .. V of this: a spare row on each side
    room[0], room[V + 1] = 1000.0, -1000.0
    tok, pos = room[1:V + 1], torch.randn(SEQ_LD + 2, T, generator=g)
    seq = torch.randint(0, V, (B, SEQ_LD), generator=g, dtype=torch.int32)
    seq[:, cur] = torch.randperm(V, generator=g)[:B].to(torch.int32)               # every row another id
    rd, sd = room.cuda(), pos.cuda()
    cases = [("ids in range", seq)]
    if B == 5 and cur == 5:
        out_of_range = seq.clone()
        out_of_range[1, cur], out_of_range[3, cur] = -1, V                          # must read rows 0 and V - 1 (a wrong clamp reads the spare rows)
        cases.append(("ids -1 and V", out_of_range))
    for why, ids in cases:
        want = tok[ids[:, cur].long().clamp(0, V - 1)] + pos[cur + 2][None]
        x = nan_f32(B + 2, T)
        qd = ids.cuda()
        check_rc(lib, lib.cap_op_opt_token_inputs(_vp(qd), SEQ_LD, cur, _vp(rd, T * 4), _vp(sd), _vp(x), B, T, V, cur_stream()))
        torch.cuda.synchronize()
        assert torch.equal(x[:B].cpu(), want) and torch.isnan(x[B:]).all(), why
    for why, args in [("null seq", (None, SEQ_LD, cur, _vp(rd, T * 4), _vp(sd), _vp(x), B, T, V)),
                      ("cur = seq_ld", (_vp(qd), SEQ_LD, SEQ_LD, _vp(rd, T * 4), _vp(sd), _vp(x), B, T, V)),
                      ("V = 0", (_vp(qd), SEQ_LD, cur, _vp(rd, T * 4), _vp(sd), _vp(x), B, T, 0))]:
        before = x.clone()
        _refused(lib, lib.cap_op_opt_token_inputs(*args, cur_stream()), "cap_op_opt_token_inputs", why)
        torch.cuda.synchronize()
        assert same_bits(x, before), why


def _sentinel_rows(kind, rows, cols):
    """the bit patterns _elementwise_ref compares: NaN words for fp32 / bf16, the odd word for a G8 container"""
    return torch.full((rows, cols), E.sentinel(kind), dtype=torch.int16 if kind == "bf16" else torch.int32, device="cuda")


@gpu
@pytest.mark.parametrize("B,n,D", [(1, 1, 8), (3, 32, 768), (40, 32, 768)])       # the last: 983 040 elements, fifteen sweeps of the grid
@pytest.mark.parametrize("dt", ["f32", "bf16", "f32s"])
def test_rows_broadcast(lib, dt, B, n, D):
    kind = E.KIND[dt]
    src = torch.randn(n, D, generator=torch.Generator().manual_seed(B + n + D))
    rows = B * n
    want = src.repeat(B, 1).numpy()                                                # row b * n + i = source row i
    dst_f, dst_t = _sentinel_rows("f32", rows + 2, D), _sentinel_rows(kind, rows + 2, D)
    sd = src.cuda()
    check_rc(lib, lib.cap_op_rows_broadcast(TAG[dt], _vp(sd), _vp(dst_f), _vp(dst_t), B, n, D, cur_stream()))
    torch.cuda.synchronize()
    for buf, k in ((dst_f, "f32"), (dst_t, kind)):
        image = np.concatenate([E.encode(k, want), _sentinel_rows(k, 2, D).cpu().numpy()])      # bit-equal rows, then the sentinel
        assert np.array_equal(buf.cpu().numpy(), image), (dt, k)
    if kind == "g8":
        vals = g8_decode(dst_t[:rows].cpu().numpy().view(np.float32))
        assert (np.abs(vals.astype(np.float64) - want) <= E.store_error("g8", want.astype(np.float64))).all()
    before_f, before_t = dst_f.clone(), dst_t.clone()
    for why, args in [("null src", (TAG[dt], None, _vp(dst_f), _vp(dst_t), B, n, D)), ("null dst_t", (TAG[dt], _vp(sd), _vp(dst_f), None, B, n, D)),
                      ("n = 0", (TAG[dt], _vp(sd), _vp(dst_f), _vp(dst_t), B, 0, D))]:
        _refused(lib, lib.cap_op_rows_broadcast(*args, cur_stream()), "cap_op_rows_broadcast", why)
    if dt == "f32s":
        _refused(lib, lib.cap_op_rows_broadcast(TAG[dt], _vp(sd), _vp(dst_f), _vp(dst_t), 1, 1, 4, cur_stream()), "D % 8", "G8 rows of 4")
    torch.cuda.synchronize()
    assert same_bits(dst_f, before_f) and same_bits(dst_t, before_t)


# ---- C. the int8 tiled route ----------------------------------------------------------------------------------------------------
def _dequant(lib, packed, rows, cols, tail=64):
    dst = torch.full((rows * cols + tail,), NAN, dtype=torch.bfloat16, device="cuda")
    check_rc(lib, lib.cap_op_dequant_i8_rowmajor(_vp(packed), _vp(dst), rows, cols, cur_stream()))
    torch.cuda.synchronize()
    assert torch.isnan(dst[rows * cols:]).all(), "bytes after rows * cols were written"
    return dst[:rows * cols].view(rows, cols)


@gpu
def test_dequant_every_byte_value_in_every_slot(lib):
    """a hand-made buffer: every 256 bytes the values shift by one, so each of the 256 values (-128 included) passes through each of
    the 8 slots of i8x8_to_bf16, in both k-steps of a lane"""
    rows, cols = 32, 128
    i = torch.arange(rows * cols)
    packed = ((i + i // 256) % 256).to(torch.uint8)
    q = i8_unpack(packed, rows, cols)
    for slot in range(8):
        assert len(set(packed[slot::8].tolist())) == 256
    assert torch.equal(i8_pack_host(q), packed)                                    # (the host packer used below is i8_unpack's inverse)
    got = _dequant(lib, packed.cuda(), rows, cols)
    assert torch.equal(got.cpu(), q.to(torch.bfloat16)) and torch.equal(got.cpu().float(), q.float())


@gpu
@pytest.mark.parametrize("rows,cols", [(16, 64), (96, 256)])
def test_dequant_of_a_quantised_matrix(lib, rows, cols):
    from embodied_captioning_amd import _native as N
    w = (torch.randn(rows, cols, generator=torch.Generator().manual_seed(rows + cols)) * 0.02).cuda()
    packed, _ = i8_pack(lib, N, w)
    got = _dequant(lib, packed, rows, cols)
    q = i8_unpack(packed, rows, cols)
    assert q.abs().max().item() == 127 and torch.equal(got.cpu(), q.to(torch.bfloat16))


@gpu
def test_dequant_production_matrix_past_one_grid_sweep(lib):
    """fc2 of OPT-2.7b: 160 x 160 = 25 600 blocks of 1 KiB, past the 4 x 4096 one sweep of the capped grid covers"""
    rows, cols = 2560, 10240
    assert (rows // 16) * (cols // 64) > 4 * 4096
    packed = torch.randint(0, 256, (rows * cols,), generator=torch.Generator().manual_seed(5), dtype=torch.uint8)
    got = _dequant(lib, packed.cuda(), rows, cols)
    assert torch.equal(got, i8_unpack(packed, rows, cols).cuda().to(torch.bfloat16))


@gpu
def test_dequant_refusals(lib):
    packed = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    dst = torch.full((4096,), NAN, dtype=torch.bfloat16, device="cuda")
    for why, needle, args in [("rows % 16", "dequant_i8", (_vp(packed), _vp(dst), 24, 64)), ("cols % 64", "dequant_i8", (_vp(packed), _vp(dst), 16, 96)),
                              ("rows = 0", "cap_op_dequant_i8_rowmajor", (_vp(packed), _vp(dst), 0, 64)),
                              ("null packed", "cap_op_dequant_i8_rowmajor", (None, _vp(dst), 16, 64)),
                              ("null dst", "cap_op_dequant_i8_rowmajor", (_vp(packed), None, 16, 64))]:
        _refused(lib, lib.cap_op_dequant_i8_rowmajor(*args, cur_stream()), needle, why)
    torch.cuda.synchronize()
    assert torch.isnan(dst).all()


def _scale_cols(lib, part, scale, M, N):
    rc = lib.cap_op_scale_cols(_vp(part), _vp(scale), M, N, cur_stream())
    torch.cuda.synchronize()
    return rc


@gpu
@pytest.mark.parametrize("M,N", [(1, 4), (33, 2560), (1056, 7680)])               # the last: 2 027 520 groups of 4, past the 4096 x 256 of one sweep
def test_scale_cols(lib, M, N):
    g = torch.Generator().manual_seed(M + N)
    part, scale = torch.randn(M, N, generator=g), torch.randn(N, generator=g)
    buf = nan_f32(M * N + 8)
    buf[:M * N] = part.view(-1).cuda()
    check_rc(lib, _scale_cols(lib, buf, scale.cuda(), M, N))
    assert torch.equal(buf[:M * N].cpu().view(M, N), part * scale[None, :]) and torch.isnan(buf[M * N:]).all()


@gpu
def test_scale_cols_refusals(lib):
    buf, scale = nan_f32(64), torch.ones(8, device="cuda")
    _refused(lib, _scale_cols(lib, buf, scale, 3, 6), "scale_cols: N % 4", "N = 6")
    _refused(lib, _scale_cols(lib, buf, scale, 0, 8), "cap_op_scale_cols", "M = 0")
    _refused(lib, _scale_cols(lib, None, scale, 3, 8), "cap_op_scale_cols", "null part")
    _refused(lib, _scale_cols(lib, buf, None, 3, 8), "cap_op_scale_cols", "null scale")
    assert torch.isnan(buf).all()


def _tiled_route(lib, a, packed, scale, M, N_, K):
    """opt_gemm's int8 prompt pass: the integers as a bf16 matrix, the tiled GEMM into fp32, the row scales on its output"""
    wq = _dequant(lib, packed, N_, K)
    out = nan_f32(M + 1, N_)
    check_rc(lib, lib.cap_op_gemm(TAG["bf16"], _vp(a), _vp(wq), None, None, _vp(out), M, N_, K, 0, 1, 0, cur_stream()))
    check_rc(lib, _scale_cols(lib, out, scale, M, N_))
    assert torch.isfinite(out[:M]).all() and torch.isnan(out[M:]).all()
    return out[:M]


@gpu
@pytest.mark.parametrize("M,N_,K", [(33, 256, 512), (70, 768, 256), (1056, 2560, 2560), (99, 2560, 10240)])
def test_int8_tiled_route_against_integer_arithmetic(lib, M, N_, K):
    """Measured on the MI355X, worst err / mag against the float64 value (docs/experiments.md has the same table); the bound of
    test_int8_weight_stream_gemm_against_integer_arithmetic, 1e-6, holds for both routes as it stands:

        (M, N, K)              tiled route   weight stream
        (33, 256, 512)         3.809e-08     2.521e-08
        (70, 768, 256)         3.913e-08     3.913e-08
        (1056, 2560, 2560)     7.157e-08     1.518e-08
        (99, 2560, 10240)      8.203e-08     6.639e-09
    """
    from embodied_captioning_amd import _native as Nn
    g = torch.Generator().manual_seed(N_ * 7 + K + M)
    w = (torch.randn(N_, K, generator=g) * 0.02).cuda()
    a = torch.randn(M, K, generator=g).cuda().bfloat16()
    packed, scale = i8_pack(lib, Nn, w)
    q = i8_unpack(packed, N_, K).cuda().double()
    exact = (a.double() @ q.T) * scale.double()[None, :]                           # integers x bf16 values: exact in fp64
    mag = (a.double().abs() @ q.abs().T) * scale.double()[None, :]
    got = _tiled_route(lib, a, packed, scale, M, N_, K)
    err = (got.double() - exact).abs()
    # the weight-streaming kernel's slice sums on the same inputs
    S = lib.cap_op_gemm_skinny_i8_slices(N_, K, 0)
    assert S >= 1
    part = nan_f32(S, M, N_)
    assert lib.cap_op_gemm_skinny_i8(_vp(a), _vp(packed), _vp(scale), None, 0, None, _vp(part), M, N_, K, cur_stream()) == S, Nn.last_error()
    torch.cuda.synchronize()
    err_ws = (part.double().sum(0) - exact).abs()
    floor = mag.clamp_min(1e-30)
    worst = ((err / floor).max().item(), (err_ws / floor).max().item())
    print(f"MEASURE int8 routes ({M}, {N_}, {K}): worst err / mag tiled {worst[0]:.3e} weight stream {worst[1]:.3e}; "
          f"worst err tiled {err.max().item():.3e} weight stream {err_ws.max().item():.3e}")
    assert (err <= mag * 1e-6 + 1e-6).all()                                        # fp32 accumulation of exact products
    # a row's result does not depend on the row count
    a1 = a[M - 1:].contiguous()
    assert torch.equal(_tiled_route(lib, a1, packed, scale, 1, N_, K)[0], got[M - 1])
