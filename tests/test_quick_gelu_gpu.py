"""GPU: activation 3 of the GEMM epilogues (quick GELU, x * sigmoid(1.702 x): CLIP's MLPs) through cap_op_gemm - against float64
on every tile in every operand type and output form, and bit-identical across the tile shapes that a row count selects (the
batch invariance of the CLIP towers rests on it).  Tile 3 is gemm_pp.hip for bf16 and split fp16: ragged M and N reach both its
interior (ACT = 3) and edge (ACT read per piece) epilogue bodies."""
import ctypes as C
import math

import pytest
import torch

from _util import G8_WSCALE, g8_decode, g8_encode

pytestmark = pytest.mark.gpu
QUICK_GELU = 3


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


def _qg(x):
    return x * torch.sigmoid(1.702 * x)


def _operands(dtype, M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    A, W, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / math.sqrt(K), torch.randn(N, generator=g)
    if dtype == "f32s":
        Ad = torch.from_numpy(g8_encode(A.numpy(), 1.0)).cuda()
        Wd = torch.from_numpy(g8_encode(W.numpy(), G8_WSCALE)).cuda()
        ref = A.double() @ W.double().T
    else:
        tdt = torch.float32 if dtype == "f32" else torch.bfloat16
        Ad, Wd = A.to(tdt).cuda(), W.to(tdt).cuda()
        ref = Ad.double().cpu() @ Wd.double().cpu().T
    return Ad, Wd, b.cuda(), _qg(ref + b.double())


TAG = {"f32": 0, "bf16": 1, "f32s": 2}


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f32s"])
@pytest.mark.parametrize("tile", [0, 1, 2, 3])
@pytest.mark.parametrize("out_f32", [0, 1])
@pytest.mark.parametrize("shape", [(600, 3072, 256), (197, 520, 192)])
def test_quick_gelu_epilogue_against_fp64(lib, dtype, tile, out_f32, shape):
    M, N, K = shape
    Ad, Wd, bd, want = _operands(dtype, M, N, K, M + N + tile)
    if out_f32 or dtype == "f32":
        out = torch.full((M, N), float("nan"), dtype=torch.float32, device="cuda")
    elif dtype == "bf16":
        out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device="cuda")
    else:
        out = torch.zeros((M, N), dtype=torch.float32, device="cuda")                   # G8 container
    _check(lib, lib.cap_op_gemm(TAG[dtype], _p(Ad), _p(Wd), _p(bd), None, _p(out), M, N, K, QUICK_GELU, out_f32, tile, _stream()))
    torch.cuda.synchronize()
    if dtype == "f32s" and not out_f32:
        got = torch.from_numpy(g8_decode(out.cpu().numpy())).double()
    else:
        got = out.double().cpu()
    assert torch.isfinite(got).all()
    tol = {"f32": 1e-4, "f32s": 1e-5}.get(dtype, 2e-2 if not out_f32 else 2e-4 * math.sqrt(K / 64))
    err = (got - want).abs().max().item()
    assert err < tol, err


@pytest.mark.parametrize("dtype", ["bf16", "f32s"])
@pytest.mark.parametrize("out_f32", [0, 1])
@pytest.mark.parametrize("shape", [(12800, 3072, 768), (1000, 520, 128), (9500, 2040, 64)])
def test_quick_gelu_epilogue_is_bit_identical_across_tiles(lib, dtype, out_f32, shape):
    """(12800, 3072, 768): CLIP ViT-B/32's fc1 at a micro-batch of 256 images; the other two have ragged edges both ways."""
    M, N, K = shape
    Ad, Wd, bd, _ = _operands(dtype, M, N, K, 7)
    outs = []
    for tile in (3, 1, 2):
        if out_f32 or dtype == "f32s":
            o = torch.full((M, N), float("nan"), dtype=torch.float32, device="cuda")
        else:
            o = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device="cuda")
        _check(lib, lib.cap_op_gemm(TAG[dtype], _p(Ad), _p(Wd), _p(bd), None, _p(o), M, N, K, QUICK_GELU, out_f32, tile, _stream()))
        outs.append(o)
    torch.cuda.synchronize()
    for t, o in zip((1, 2), outs[1:]):
        assert torch.equal(outs[0].view(torch.int16 if o.dtype == torch.bfloat16 else torch.int32),
                           o.view(torch.int16 if o.dtype == torch.bfloat16 else torch.int32)), t
