"""GPU: the four address-computing epilogues of the GEMM (csrc/gemm.h: EPI_PATCH, EPI_CROSSKV, EPI_QKVCACHE, EPI_PARTIAL) alone, on
every tile family launch_gemm can send them to, through cap_op_gemm_epi (launch_gemm with the whole of GemmParams).

Every output lives in a buffer of sentinels (NaN bit patterns) with GUARD sentinel elements on both sides, and every case compares
the WHOLE buffer with the expected bit image: class rows, pad columns N .. ldc, cache positions other than t, cache rows from M up
to the capacity, slices' rows beyond the live row tiles and the guards must still be the sentinel.

Two expectations per case:
 (a) bit identity with the plain store (EPI_STORE) of the same operands on the same tile in the output type the scatter uses, moved
     by the host index maps of tests/_gemm_epi_ref.py (checked on the CPU by tests/test_gemm_epi_ref_cpu.py).  Both epilogues form
     acc (* 2^-12 for G8 operands, exact) + bias; the patch epilogue adds the position row once more in fp32, which the host
     repeats with one fp32 add.  No tolerance.
 (b) distance to A64 @ W64.T + bias (+ pos) in float64, with the bound the plain-store test of the same dtype already has and no new
     number: test_kernels_gpu.py::test_gemm_bias_against_fp64's 2e-4 sqrt(K / 64) for fp32 outputs of f32 / bf16 operands (the
     reference takes the operands as rounded to bf16), 0.03 for bf16 rows as in test_cross_kv_gemm_scatters_into_the_cache_layout,
     test_split_gpu.py::test_split_gemm_is_fp32_grade's 1e-5 sqrt(max(K, 256) / 256) for G8 operands (as there, against the ORIGINAL
     fp32 operands); the patch epilogue gets 2^-23 max|ref| more for its one extra add; split-K sums get the bound times the slice
     count.  The bf16 rows' 0.03 is half an ulp of bf16 (2^-6 = 0.016 below 8) plus the sum's own error, so it stands for |v| < 8
     only: the operands here are N(0, 1) products plus a bias of N(0, 1/4), 7 standard deviations inside that.
Each test prints its worst error / bound ratio (MEASURE) before it asserts, with the tile its tile 0 launch resolves to.

bf16 and split-mode (G8) tiles agree bit for bit (test_split_gemm_tiles_are_bit_identical, Mma<bf16_t>::run16's contract), so for
those every tile's image must also equal tile 2's; fp32's 32x32x2 MFMA chains differ between tile families and are not compared.

The refusals - cap_op_gemm_epi's own, and launch_gemm's of EPI_PARTIAL with more than one slice on the 256x256 LDS-DMA kernel, which
has no slice loop - are checked by message with every output still all sentinel; the refused form is never launched."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import _elementwise_ref as E
import _gemm_epi_ref as G
from _util import G8_WSCALE, g8_encode

pytestmark = pytest.mark.gpu

TAG = {"f32": 0, "bf16": 1, "f32s": 2}
DTYPES = ["f32", "bf16", "f32s"]
GUARD = 64
BM = {1: 128, 2: 64, 4: 256}              # row tile of the register-staged kernels (launch_tile)


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


class Buf:
    """an output of `shape` elements of `kind` (f32 / bf16) filled with its NaN sentinel, guards on both sides"""

    def __init__(self, kind, *shape):
        self.kind, self.shape = kind, shape
        self.n = int(np.prod(shape))
        self.tdt = torch.int16 if kind == "bf16" else torch.int32
        self.raw = torch.full((self.n + 2 * GUARD,), E.sentinel(kind), dtype=self.tdt, device="cuda")
        self.ptr = self.raw.data_ptr() + GUARD * self.raw.element_size()

    def dev(self):
        """the payload as a device tensor of bit patterns; the guards are checked on the device"""
        torch.cuda.synchronize()
        s = E.sentinel(self.kind)
        assert bool((self.raw[:GUARD] == s).all()) and bool((self.raw[GUARD + self.n:] == s).all()), "a guard region was written"
        return self.raw[GUARD:GUARD + self.n].view(self.shape)

    def bits(self):
        return self.dev().cpu().numpy()

    def untouched(self):
        return bool((self.dev() == E.sentinel(self.kind)).all())


def _values(kind, bits):
    """bit patterns -> float64"""
    b = np.ascontiguousarray(bits)
    if kind == "f32":
        return b.view(np.float32).astype(np.float64)
    return torch.from_numpy(b).view(torch.bfloat16).double().numpy()


def _f32(kind, bits):
    """bit patterns -> the stored numbers as fp32 (exact for bf16) - what the host maps move"""
    return _values(kind, bits).astype(np.float32)


def _bits(kind, x32):
    """fp32 numbers that are values of `kind` -> their bit patterns"""
    x32 = np.ascontiguousarray(x32, dtype=np.float32)
    if kind == "f32":
        return x32.view(np.int32)
    return torch.from_numpy(x32).to(torch.bfloat16).view(torch.int16).numpy()


def _same(buf, want, what):
    got = buf.bits().reshape(want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} of {want.size} words differ, first at {bad[0].tolist()}: "
                             f"got {int(got[tuple(bad[0])]):#x}, want {int(want[tuple(bad[0])]):#x}")
    return got


def _operands(dt, A, W):
    """fp32 host matrices -> (device A, device W, the float64 values the reference multiplies)"""
    if dt == "f32":
        return A.cuda(), W.cuda(), A.double(), W.double()
    if dt == "bf16":
        Ab, Wb = A.to(torch.bfloat16), W.to(torch.bfloat16)
        return Ab.cuda(), Wb.cuda(), Ab.double(), Wb.double()
    return (torch.from_numpy(g8_encode(A.numpy())).cuda(), torch.from_numpy(g8_encode(W.numpy(), G8_WSCALE)).cuda(),
            A.double(), W.double())       # as test_split_gemm_is_fp32_grade: against the original fp32 operands


def _okind(dt):
    """storage of the cache-scatter outputs: the operand type, fp32 in the split mode"""
    return "bf16" if dt == "bf16" else "f32"


def _bound(dt, K, kind):
    if kind == "bf16":
        return 0.03
    if dt == "f32s":
        return 1e-5 * math.sqrt(max(K, 256) / 256)
    return 2e-4 * math.sqrt(K / 64)


def _auto_tile(dt, M, N, K):
    """launch_gemm's choice for tile 0 (csrc/gemm.hip)"""
    t256 = -(-M // 256) * -(-N // 256)
    t128 = -(-M // 128) * -(-N // 128)
    tile = 3 if (t256 >= 256 or (t256 >= 128 and M >= 256)) else (1 if t128 >= 256 else 2)
    if dt == "f32s" and tile == 2 and t128 >= 128 and K >= 2048:
        tile = 1
    return tile


def _ptr(x):
    if x is None:
        return None
    if isinstance(x, Buf):
        return x.ptr
    if isinstance(x, torch.Tensor):
        return x.data_ptr()
    return int(x)


def _gemm(lib, dt, epi, tile, A, W, bias, Cout, M, N, K, *, lda=None, ldw=None, ldc=None, C2=None, aux=None, out_f32=1, splitk=1,
          p=(0, 0, 0, 0), m_live=None, kv16=0):
    from embodied_captioning_amd._native import CapGemmEpi
    a = CapGemmEpi()
    a.A, a.lda, a.W, a.ldw, a.bias = _ptr(A), K if lda is None else lda, _ptr(W), K if ldw is None else ldw, _ptr(bias)
    a.C, a.ldc, a.C2, a.aux = _ptr(Cout), N if ldc is None else ldc, _ptr(C2), _ptr(aux)
    a.M, a.N, a.K, a.gelu, a.out_f32, a.epi, a.splitk = M, N, K, 0, out_f32, epi, splitk
    a.p0, a.p1, a.p2, a.p3 = p
    a.kv16, a.m_live, a.tile = kv16, _ptr(m_live), tile
    return lib.cap_op_gemm_epi(TAG[dt], C.byref(a), _stream())


def _plain(lib, dt, tile, Ad, Wd, bd, M, N, K, kind, what):
    """EPI_STORE of the same operands on the same tile in the scatter's output type -> the stored numbers as fp32 [M, N]"""
    out = Buf(kind, M, N)
    _ok(lib, _gemm(lib, dt, G.EPI_STORE, tile, Ad, Wd, bd, out, M, N, K, out_f32=0 if kind == "bf16" else 1))
    b = out.bits()
    assert not (b == E.sentinel(kind)).any(), what + ": the plain store left sentinels"
    return _f32(kind, b)


def _inputs(seed, M, N, K):
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) / math.sqrt(K)
    bias = torch.randn(N, generator=g) * 0.5
    return g, A, W, bias


def _tail_condition(M, N):
    """launch_pp_t's condition for running the last round of 256 x 256 tiles as half tiles in a second launch"""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    tiles = -(-M // 256) * -(-N // 256)
    rounds, tail = divmod(tiles, n_cu)
    return 1 <= rounds <= 4 and 0 < 2 * tail <= n_cu, (tiles, n_cu, rounds, tail)


# ---- EPI_PATCH -----------------------------------------------------------------------------------------------------------
# (B, P, N, K, ldc).  (1, 5, 64, 64): one partial tile, K below gemm_pp.hip's two bf16 stages (its fall-back kernel runs);
# (7, 49, 192, 128): P no multiple of 4 or 16, images begin mid-fragment, two ragged 256-row tiles; (3, 196, 328, 192): ragged N
# against 64 / 128 / 256; (2, 50, 128, 128, 160): ldc > N - the position table's pitch is N, the output's ldc
PATCH_GEOMS = [(1, 5, 64, 64, 64), (7, 49, 192, 128, 192), (3, 196, 328, 192, 328), (2, 50, 128, 128, 160)]


@pytest.mark.parametrize("geom", PATCH_GEOMS)
@pytest.mark.parametrize("dt", DTYPES)
def test_patch_epilogue(lib, dt, geom):
    """Row (b, p) -> row b (P + 1) + 1 + p, + pos[1 + p], fp32 output for every operand type; tiles 0 .. 6 (6: this epilogue's
    documented fall-back is tile 2), with and without a bias (CLIP's patch GEMM has none: on the LDS-DMA kernels the bias is a DMA
    into LDS, not a register load)."""
    B, P, N, K, ldc = geom
    M = B * P
    g, A, W, bias = _inputs(B * 1000 + P + N + K, M, N, K)
    pos = torch.randn(P + 1, N, generator=g)
    Ad, Wd, A64, W64 = _operands(dt, A, W)
    bd, pd = bias.cuda(), pos.cuda()
    prod64 = (A64 @ W64.T).numpy()
    auto = _auto_tile(dt, M, N, K)
    worst, where = 0.0, None
    for has_bias in (True, False):
        ref64, mask = G.patch_image(prod64 + (bias.double().numpy() if has_bias else 0.0), pos.numpy(), B, P, ldc)
        bound = _bound(dt, K, "f32") + 2.0 ** -23 * np.abs(ref64[mask]).max()
        images = {}
        for tile in (0, 1, 2, 3, 4, 5, 6):
            what = f"patch {dt} {geom} tile {tile} bias {has_bias}"
            b = bd if has_bias else None
            # (tile 6 is the decode rows kernel for plain stores, with sums in another order: the partner is the fall-back's)
            plain = _plain(lib, dt, 2 if tile == 6 else tile, Ad, Wd, b, M, N, K, "f32", what)
            out = Buf("f32", B * (P + 1), ldc)
            _ok(lib, _gemm(lib, dt, G.EPI_PATCH, tile, Ad, Wd, b, out, M, N, K, ldc=ldc, aux=pd, p=(P, 0, 0, 0)))
            img, m2 = G.patch_image(plain, pos.numpy(), B, P, ldc)
            images[tile] = _same(out, G.with_sentinel(_bits("f32", img), m2, E.NAN32), what + " vs the plain store + one fp32 add")
            r = np.abs(_values("f32", images[tile])[mask] - ref64[mask]).max() / bound
            if r > worst:
                worst, where = r, what
        assert np.array_equal(images[0], images[auto]), "tile 0 is not the launcher's documented choice"
        if dt != "f32":
            for tile, im in images.items():
                assert np.array_equal(im, images[2]), f"patch {dt} {geom} bias {has_bias}: tile {tile} differs from tile 2"
    print(f"MEASURE patch {dt} {geom}: worst fp64 error / bound {worst:.3f} ({where}); tile 0 -> {auto}")
    assert worst < 1.0


@pytest.mark.parametrize("dt", ["bf16", "f32s"])
def test_patch_epilogue_on_the_half_tile_tail_launch(lib, dt):
    """gemm_pp.hip runs a last round of 256 x 256 tiles that is at most half full as 128-row half tiles in a second launch
    (launch_pp_t: 1 <= rounds <= 4 and 0 < 2 tail <= CUs): B x 196 rows, N = 768, K = 192 on tile 3, B from the CU count (256 CUs:
    B = 337, 777 tiles).  Compared on the device with the plain store of the same launch shape + the position add; the fp64 bound
    of this kernel at such a size is test_gemm_bias_against_fp64's (70000, 768, 128) case."""
    P, N, K = 196, 768, 192
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    B = next(b for b in range(max(1, round(337 * n_cu / 256)), 100000) if _tail_condition(b * P, N)[0])
    M = B * P
    ok, figures = _tail_condition(M, N)
    assert ok, figures
    g, A, W, bias = _inputs(B, M, N, K)
    pos = torch.randn(P + 1, N, generator=g)
    Ad, Wd, _, _ = _operands(dt, A, W)
    bd, pd = bias.cuda(), pos.cuda()
    plain, out = Buf("f32", M, N), Buf("f32", B, P + 1, N)
    _ok(lib, _gemm(lib, dt, G.EPI_STORE, 3, Ad, Wd, bd, plain, M, N, K))
    _ok(lib, _gemm(lib, dt, G.EPI_PATCH, 3, Ad, Wd, bd, out, M, N, K, aux=pd, p=(P, 0, 0, 0)))
    v = plain.dev().view(torch.float32)
    assert bool(torch.isfinite(v).all())
    want = torch.full((B, P + 1, N), E.NAN32, dtype=torch.int32, device="cuda")
    want[:, 1:, :] = (v.view(B, P, N) + pd[1:]).view(torch.int32)
    print(f"MEASURE patch tail {dt}: B={B}, (tiles, CUs, rounds, tail) = {figures}")
    assert torch.equal(out.dev(), want)


# ---- EPI_CROSSKV ---------------------------------------------------------------------------------------------------------
# (n_img, tokens, heads, layers, K).  (9, 33, 1, 2): one head, two images inside one 16-row fragment
CROSS_GEOMS = [(2, 50, 2, 3, 128), (9, 33, 1, 2, 128), (3, 197, 12, 2, 256)]


@pytest.mark.parametrize("geom", CROSS_GEOMS)
@pytest.mark.parametrize("dt", DTYPES)
def test_crosskv_epilogue(lib, dt, geom):
    """[layer][k | v][image][head][token][64] in the operand type (fp32 in the split mode), kv16 = 0, tiles 1 .. 5 - the 128 x 128
    and 256 x 256 kernels the production batch runs and cap_op_gemm_crosskv's tile 0 never selects at test sizes; with and
    without a bias."""
    n_img, tokens, heads, layers, K = geom
    M, N = n_img * tokens, layers * 2 * heads * 64
    kind = _okind(dt)
    _, A, W, bias = _inputs(M + N + K, M, N, K)
    Ad, Wd, A64, W64 = _operands(dt, A, W)
    bd = bias.cuda()
    prod64 = (A64 @ W64.T).numpy()
    bound = _bound(dt, K, kind)
    worst, where = 0.0, None
    for has_bias in (True, False):
        ref64 = G.crosskv_image(prod64 + (bias.double().numpy() if has_bias else 0.0), n_img, tokens, heads, layers)
        images = {}
        for tile in (1, 2, 3, 4, 5):
            what = f"cross K/V {dt} {geom} tile {tile} bias {has_bias}"
            b = bd if has_bias else None
            plain = _plain(lib, dt, tile, Ad, Wd, b, M, N, K, kind, what)
            out = Buf(kind, layers, 2, n_img, heads, tokens, 64)
            _ok(lib, _gemm(lib, dt, G.EPI_CROSSKV, tile, Ad, Wd, b, out, M, N, K, ldc=0, out_f32=0 if kind == "bf16" else 1,
                           p=(tokens, heads, n_img, 0)))
            images[tile] = _same(out, _bits(kind, G.crosskv_image(plain, n_img, tokens, heads, layers)), what + " vs the plain store")
            r = np.abs(_values(kind, images[tile]) - ref64).max() / bound
            if r > worst:
                worst, where = r, what
        if dt != "f32":
            for tile, im in images.items():
                assert np.array_equal(im, images[2]), f"cross K/V {dt} {geom} bias {has_bias}: tile {tile} differs from tile 2"
    print(f"MEASURE cross K/V {dt} {geom}: worst fp64 error / bound {worst:.3f} ({where})")
    assert worst < 1.0


@pytest.mark.parametrize("dt", ["bf16", "f32s"])
def test_crosskv_epilogue_on_the_half_tile_tail_launch(lib, dt):
    """(4, 197, 12, 12, 128): 4 x 72 = 288 tiles of 256 x 256, on 256 CUs one round and a tail of 32 - gemm_pp.hip's half-tile
    launch with the scatter epilogue (bf16 rows / fp32 rows).  On the device against the plain store of the same launch shape."""
    n_img, tokens, heads, layers, K = 4, 197, 12, 12, 128
    M, N = n_img * tokens, layers * 2 * heads * 64
    ok, figures = _tail_condition(M, N)
    assert ok, figures
    kind = _okind(dt)
    f32out = 0 if kind == "bf16" else 1
    _, A, W, bias = _inputs(M + N, M, N, K)
    Ad, Wd, _, _ = _operands(dt, A, W)
    bd = bias.cuda()
    plain, out = Buf(kind, n_img, tokens, layers, 2, heads, 64), Buf(kind, layers, 2, n_img, heads, tokens, 64)
    _ok(lib, _gemm(lib, dt, G.EPI_STORE, 3, Ad, Wd, bd, plain, M, N, K, out_f32=f32out))
    _ok(lib, _gemm(lib, dt, G.EPI_CROSSKV, 3, Ad, Wd, bd, out, M, N, K, ldc=0, out_f32=f32out, p=(tokens, heads, n_img, 0)))
    pv = plain.dev()
    assert not bool((pv == E.sentinel(kind)).any())
    print(f"MEASURE cross K/V tail {dt}: (tiles, CUs, rounds, tail) = {figures}")
    assert torch.equal(out.dev(), pv.permute(2, 3, 0, 4, 1, 5).contiguous())


# ---- EPI_QKVCACHE --------------------------------------------------------------------------------------------------------
# (R, cap, H, K, Lmax, positions)
QKV_GEOMS = [(37, 40, 2, 128, 40, (0, 33, 39)), (300, 300, 12, 768, 48, (35,))]


@pytest.mark.parametrize("geom", QKV_GEOMS)
@pytest.mark.parametrize("dt", DTYPES)
def test_qkvcache_epilogue(lib, dt, geom):
    """q -> qbuf [R, H 64] (pitch H 64 whatever ldc says: a launch with another ldc leaves the same image), k / v -> position t of
    cache[k | v][row][head][.][64], whose row stride is the capacity p0, not M: positions other than t and rows from R to the
    capacity keep the sentinel.  Tiles 1 .. 5 (BLIP's un-fused step beyond 32 positions is the one product path here)."""
    R, cap, H, K, Lmax, ts = geom
    D, N = H * 64, 3 * H * 64
    kind = _okind(dt)
    f32out = 0 if kind == "bf16" else 1
    _, A, W, bias = _inputs(R + H + K, R, N, K)
    Ad, Wd, A64, W64 = _operands(dt, A, W)
    bd = bias.cuda()
    ref64 = (A64 @ W64.T + bias.double()).numpy()
    bound = _bound(dt, K, kind)
    worst, where = 0.0, None
    for t in ts:
        q64, c64, mask = G.qkvcache_image(ref64, cap, H, Lmax, t)
        images = {}
        for tile in (1, 2, 3, 4, 5):
            what = f"q|k|v {dt} {geom[:5]} t={t} tile {tile}"
            plain = _plain(lib, dt, tile, Ad, Wd, bd, R, N, K, kind, what)
            qw, cw, m2 = G.qkvcache_image(plain, cap, H, Lmax, t)
            cw = G.with_sentinel(_bits(kind, cw), m2, E.sentinel(kind))
            for ldc in (D, N) if tile in (2, 3) and t == ts[0] else (D,):
                qb, cb = Buf(kind, R, D), Buf(kind, 2, cap, H, Lmax, 64)
                _ok(lib, _gemm(lib, dt, G.EPI_QKVCACHE, tile, Ad, Wd, bd, qb, R, N, K, ldc=ldc, C2=cb, out_f32=f32out, p=(cap, H, Lmax, t)))
                qi = _same(qb, _bits(kind, qw), f"{what} ldc {ldc}: q vs the plain store")
                ci = _same(cb, cw, f"{what} ldc {ldc}: cache vs the plain store")
            images[tile] = (qi, ci)
            r = max(np.abs(_values(kind, qi) - q64).max(), np.abs(_values(kind, ci[mask]) - c64[mask]).max()) / bound
            if r > worst:
                worst, where = r, what
        if dt != "f32":
            for tile, (qi, ci) in images.items():
                assert np.array_equal(qi, images[2][0]) and np.array_equal(ci, images[2][1]), f"q|k|v {dt} t={t}: tile {tile} differs from tile 2"
    print(f"MEASURE q|k|v {dt} {geom[:5]}: worst fp64 error / bound {worst:.3f} ({where})")
    assert worst < 1.0


# ---- EPI_PARTIAL on the register-staged tiles ----------------------------------------------------------------------------
PARTIAL_SHAPES = [(37, 768, 768, 3), (5, 200, 384, 2), (300, 768, 3072, 4), (64, 2304, 768, 1)]


@pytest.mark.parametrize("shape", PARTIAL_SHAPES)
@pytest.mark.parametrize("dt", DTYPES)
def test_partial_epilogue_on_the_register_staged_tiles(lib, dt, shape):
    """Split-K on tiles 1 / 2 / 4 (the fp32 mode's decode projections run tile 2; the existing tests call tile 6 only): slice z is
    the plain store, without a bias, of the z-th K range of the operands (a view: lda = ldw = K) on the same tile, bit for bit; the
    slices summed in order in float64 match the product within the plain-store bound times S.  With a live-row count n (device
    int32) whole live row tiles are written: rows of tiles that start at or beyond n keep the sentinel in every slice, the rows
    below have the bits of the launch without a count."""
    M, N, K, S = shape
    Ks = K // S
    _, A, W, _ = _inputs(M + 3 * N + 7 * K + S, M, N, K)
    Ad, Wd, A64, W64 = _operands(dt, A, W)
    ref64 = (A64 @ W64.T).numpy()
    bound = S * _bound(dt, K, "f32")
    worst, where = 0.0, None
    images = {}
    for tile in (1, 2, 4):
        what = f"split-K {dt} {shape} tile {tile}"
        part = Buf("f32", S, M, N)
        _ok(lib, _gemm(lib, dt, G.EPI_PARTIAL, tile, Ad, Wd, None, part, M, N, K, splitk=S))
        slices = []
        for z in range(S):
            off = z * Ks * Ad.element_size()
            o = Buf("f32", M, N)
            _ok(lib, _gemm(lib, dt, G.EPI_STORE, tile, Ad.data_ptr() + off, Wd.data_ptr() + off, None, o, M, N, Ks, lda=K, ldw=K))
            slices.append(o.bits())
        img, mask = G.partial_image(slices, M, N)
        assert mask.all() and not (img == E.NAN32).any()
        images[tile] = full = _same(part, img, what + " vs the plain store of each K range")
        r = np.abs(_values("f32", full).sum(0) - ref64).max() / bound         # float64 sum over the slice axis, in slice order
        if r > worst:
            worst, where = r, what
        for n in sorted({0, 1, 64, 65, M}):
            nd = torch.tensor([n], dtype=torch.int32, device="cuda")
            lim = Buf("f32", S, M, N)
            _ok(lib, _gemm(lib, dt, G.EPI_PARTIAL, tile, Ad, Wd, None, lim, M, N, K, splitk=S, m_live=nd))
            wimg, wmask = G.partial_image(list(full), M, N, rows=G.live_rows(n, M, BM[tile]))
            _same(lim, G.with_sentinel(wimg, wmask, E.NAN32), f"{what} live rows {n}")
    if dt != "f32":
        for tile, im in images.items():
            assert np.array_equal(im, images[2]), f"split-K {dt} {shape}: tile {tile} differs from tile 2"
    print(f"MEASURE split-K {dt} {shape}: worst fp64 error / bound {worst:.3f} ({where})")
    assert worst < 1.0


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_hook_refuses_what_an_epilogue_cannot_address(lib):
    """cap_op_gemm_epi names itself and launches nothing for: null A / W / C; patch: null aux, p0 < 1, M % p0, ldc < N; cross K/V:
    p0 / p1 / p2 < 1, M != p0 p2, N % (2 p1 64); q|k|v: null C2, N != 3 p1 64, p0 < M, p3 outside [0, p2); split-K: splitk < 1
    (and a host-side slice index); an unknown epi."""
    M, N, K = 8, 128, 64
    A = torch.zeros(M, K, device="cuda")
    W = torch.zeros(3 * N, K, device="cuda")
    aux = torch.zeros(M + 1, 3 * N, device="cuda")
    out, out2 = Buf("f32", 4 * M, 3 * N), Buf("f32", 2, M, 2, 4, 64)
    me = "cap_op_gemm_epi"

    def call(epi, needles, A=A, W=W, Cout=out, M=M, N=N, **kw):
        _refused(lib, _gemm(lib, "f32", epi, 2, A, W, None, Cout, M, N, K, **kw), me, *needles)
        assert out.untouched() and out2.untouched()

    for epi in range(5):
        call(epi, ["null pointer"], A=None)
        call(epi, ["null pointer"], W=None)
        call(epi, ["null pointer"], Cout=None)
    patch = dict(aux=aux, p=(4, 0, 0, 0))
    call(G.EPI_PATCH, ["patch", "null aux"], p=(4, 0, 0, 0))
    call(G.EPI_PATCH, ["patch", "p0=0"], aux=aux, p=(0, 0, 0, 0))
    call(G.EPI_PATCH, ["patch", "p0=-4"], aux=aux, p=(-4, 0, 0, 0))
    call(G.EPI_PATCH, ["patch", "M=8", "p0=3"], aux=aux, p=(3, 0, 0, 0))
    call(G.EPI_PATCH, ["patch", "ldc=124 < N=128"], ldc=124, **patch)
    for p, needle in (((0, 2, 2, 0), "p0=0"), ((4, 0, 2, 0), "p1=0"), ((4, 1, 0, 0), "p2=0"), ((-4, 1, -2, 0), "p0=-4")):
        call(G.EPI_CROSSKV, ["cross K/V", needle], p=p)
    call(G.EPI_CROSSKV, ["cross K/V", "M=8 is not p0 * p2 = 3 * 2"], p=(3, 1, 2, 0))
    call(G.EPI_CROSSKV, ["cross K/V", "N=128", "2 * p1=2"], p=(4, 2, 2, 0))
    call(G.EPI_QKVCACHE, ["q|k|v", "null C2"], N=384, p=(M, 2, 4, 0))
    call(G.EPI_QKVCACHE, ["q|k|v", "N=128 is not 3 * p1=2"], C2=out2, p=(M, 2, 4, 0))
    call(G.EPI_QKVCACHE, ["q|k|v", "p0=7 rows, M=8"], N=384, C2=out2, p=(7, 2, 4, 0))
    call(G.EPI_QKVCACHE, ["q|k|v", "p3=-1"], N=384, C2=out2, p=(M, 2, 4, -1))
    call(G.EPI_QKVCACHE, ["q|k|v", "p3=4 outside [0, p2=4)"], N=384, C2=out2, p=(M, 2, 4, 4))
    call(G.EPI_PARTIAL, ["split-K", "splitk=0"], splitk=0)
    call(G.EPI_PARTIAL, ["split-K", "splitk=-2"], splitk=-2)
    call(G.EPI_PARTIAL, ["split-K", "p3=1"], splitk=2, p=(0, 0, 0, 1))
    call(5, ["unknown epi 5"])
    call(-1, ["unknown epi -1"])
    # the same struct with nothing wrong is taken: the refusals above are the hook's, not a broken fixture's
    _ok(lib, _gemm(lib, "f32", G.EPI_QKVCACHE, 2, A, W, None, out, M, 384, K, C2=out2, p=(M, 2, 4, 3)))
    assert not out.untouched() and not out2.untouched()


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_split_k_is_refused_on_the_kernel_without_a_slice_loop(lib, dt):
    """gemm_big_kernel (f32 / bf16 at tiles 3 and 5; bf16 reaches it once gemm_pp.hip has declined EPI_PARTIAL) walks the whole K
    and never reads splitk: with more than one slice it would put the full sum in slice 0 and leave the others alone.  launch_gemm
    refuses that, at tile 3, tile 5 and where tile 0 resolves to tile 3, through cap_op_gemm_partial and cap_op_gemm_epi alike -
    checked by message, nothing launched, the slices still all sentinel.  One slice stays legitimate on those kernels."""
    K, S = 256, 2
    for M, N, tiles in ((40, 64, (3, 5)), (256 * 128, 4, (0,))):           # 128 x 1 tiles of 256 x 256 with M >= 256: tile 0 -> 3
        assert 0 not in tiles or _auto_tile(dt, M, N, K) == 3
        _, A, W, _ = _inputs(M + N, M, N, K)
        Ad, Wd, _, _ = _operands(dt, A, W)
        for tile in tiles:
            part = Buf("f32", S, M, N)
            rc = lib.cap_op_gemm_partial(TAG[dt], Ad.data_ptr(), Wd.data_ptr(), part.ptr, M, N, K, S, tile, _stream())
            _refused(lib, rc, "launch_gemm", "split-K 2", "no K-slice loop")
            assert part.untouched()
            _refused(lib, _gemm(lib, dt, G.EPI_PARTIAL, tile, Ad, Wd, None, part, M, N, K, splitk=S), "launch_gemm", "no K-slice loop")
            assert part.untouched()
    # one slice on the same kernels: the plain product, the bits of the plain store without a bias on tile 3 / 5
    M, N = 40, 64
    _, A, W, _ = _inputs(M + N, M, N, K)
    Ad, Wd, _, _ = _operands(dt, A, W)
    for tile in (3, 5):
        one, plain = Buf("f32", 1, M, N), Buf("f32", M, N)
        _ok(lib, lib.cap_op_gemm_partial(TAG[dt], Ad.data_ptr(), Wd.data_ptr(), one.ptr, M, N, K, 1, tile, _stream()))
        _ok(lib, _gemm(lib, dt, G.EPI_STORE, tile, Ad, Wd, None, plain, M, N, K))
        assert not plain.untouched() and np.array_equal(one.bits()[0], plain.bits())


def test_split_k_on_the_split_modes_256_tile_keeps_its_slices(lib):
    """G8 operands at tiles 3 / 5 run the register-staged 256 x 256 tile (gemm_pp.hip declines EPI_PARTIAL), which has the slice
    loop: still accepted, and the bits of tile 2."""
    M, N, K, S = 40, 64, 256, 2
    _, A, W, _ = _inputs(7, M, N, K)
    Ad, Wd, _, _ = _operands("f32s", A, W)
    images = []
    for tile in (2, 3, 5):
        part = Buf("f32", S, M, N)
        _ok(lib, _gemm(lib, "f32s", G.EPI_PARTIAL, tile, Ad, Wd, None, part, M, N, K, splitk=S))
        images.append(part.bits())
    assert not (images[0] == E.NAN32).any()
    assert np.array_equal(images[0], images[1]) and np.array_equal(images[0], images[2])
