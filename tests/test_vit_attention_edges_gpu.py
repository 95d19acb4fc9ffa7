"""GPU: the seven MFMA ViT attention kernels (csrc/attention.hip on csrc/vit_attn_frag.h) at the token counts where their shared
mask / chunk / tail steps can go wrong: zero, one and 31 padding keys in the last key block, a chunk boundary, a chunk that ends
in key blocks past the end, head widths that end inside a 32-wide output block.  Every context buffer starts as NaN and must come
back finite; references are float64 softmax attention; the bars are the ones the other tests hold the same kernels to."""
import ctypes as C

import numpy as np
import pytest
import torch

from _util import g8_decode, g8_encode

pytestmark = pytest.mark.gpu
F32, BF16, SPLIT = 0, 1, 2
B, H = 2, 2


@pytest.fixture(scope="module")
def lib():
    from embodied_captioning_amd import _native
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _native.load_library()


def _p(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _check(lib, rc):
    assert rc == 0, lib.cap_last_error().decode()


def _qkv(N, hd, seed):
    return torch.randn(B * N, 3 * H * hd, generator=torch.Generator().manual_seed(seed)) * 1.5


def _attn_ref(qkv, N, hd, causal=False):
    x = qkv.double().view(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    s = (x[0] @ x[1].transpose(-1, -2)) / hd ** 0.5
    if causal:
        s = s + torch.full((N, N), float("-inf"), dtype=torch.float64).triu(1)
    return (torch.softmax(s, -1) @ x[2]).permute(0, 2, 1, 3).reshape(B * N, H * hd)


def _nan_ctx(N, hd, tdt=torch.float32):
    return torch.full((B * N, H * hd), float("nan"), dtype=tdt, device="cuda")


def _err(got, ref):
    """got: a float tensor on the host, every element finite; the largest distance to the float64 reference"""
    assert torch.isfinite(got).all()
    return (got.double() - ref).abs().max().item()


def _decode(ctx, dtype):
    return torch.from_numpy(g8_decode(ctx.cpu().numpy())) if dtype == SPLIT else ctx.float().cpu()


@pytest.mark.parametrize("N", [32, 33, 64, 193, 224, 288, 608])
def test_bf16_head64_padding_keys_of_the_last_block(lib, N):
    """vit_attention_mfma<1, 2, 7, 9> and vit_attention_flash<19, 5> (impl 2): 0, 31, 0, 31, 0, 0, 0 padding keys."""
    qkv = _qkv(N, 64, N).to(torch.bfloat16)
    qd, ctx = qkv.cuda(), _nan_ctx(N, 64, torch.bfloat16)
    _check(lib, lib.cap_op_vit_attention(BF16, _p(qd), _p(ctx), B, N, H, 2, _stream()))
    torch.cuda.synchronize()
    err = _err(ctx.float().cpu(), _attn_ref(qkv, N, 64))
    assert err < 3e-2, err


@pytest.mark.parametrize("N,hd,impl", [(288, 88, 0), (64, 88, 0), (32, 80, 8)])
def test_bf16_wide_heads_full_last_block_and_causal(lib, N, hd, impl):
    """vit_attention_flash_wide<9, 5> with no padding key, <2, 2> with two full blocks, and <2, 2> causal (impl bit 8) with one
    key block of its two."""
    qkv = _qkv(N, hd, N + hd).to(torch.bfloat16)
    qd, ctx = qkv.cuda(), _nan_ctx(N, hd, torch.bfloat16)
    _check(lib, lib.cap_op_vit_attention_hd(BF16, _p(qd), _p(ctx), B, N, H, hd, impl, _stream()))
    torch.cuda.synchronize()
    err = _err(ctx.float().cpu(), _attn_ref(qkv, N, hd, causal=bool(impl & 8)))
    assert err < 3e-2, err


@pytest.mark.parametrize("dtype", [F32, SPLIT])
@pytest.mark.parametrize("N", [32, 224, 288])
def test_fp32_head64_full_last_block(lib, dtype, N):
    """vit_attention_f32_mfma<1, 7, 9>: fp32 q | k | v in, fp32 or G8 context, no padding key."""
    qkv = _qkv(N, 64, N + 1)
    qd, ctx = qkv.cuda(), _nan_ctx(N, 64)
    _check(lib, lib.cap_op_vit_attention(dtype, _p(qd), _p(ctx), B, N, H, 0, _stream()))
    torch.cuda.synchronize()
    err = _err(_decode(ctx, dtype), _attn_ref(qkv, N, 64))
    assert err < 1e-5, err


@pytest.mark.parametrize("dtype", [F32, SPLIT])
@pytest.mark.parametrize("N,hd", [(96, 88), (97, 72), (192, 96)])
def test_fp32_wide_heads_at_the_96_key_chunk_boundary(lib, dtype, N, hd):
    """vit_attention_f32_mfma_wide<3, 3>: exactly one chunk, one key into a second chunk whose other blocks are past the end, two
    full chunks; head widths that end inside and at the end of the third output block."""
    qkv = _qkv(N, hd, N * 7 + hd)
    qd, ctx = qkv.cuda(), _nan_ctx(N, hd)
    _check(lib, lib.cap_op_vit_attention_hd(dtype, _p(qd), _p(ctx), B, N, H, hd, 0, _stream()))
    torch.cuda.synchronize()
    err = _err(_decode(ctx, dtype), _attn_ref(qkv, N, hd))
    assert err < 2e-5, err


@pytest.mark.parametrize("N", [256, 384, 385])
def test_split_g8_at_the_128_key_chunk_boundaries(lib, N):
    """vit_attention_split<4, false> (impl 3, G8 q | k | v in): two full chunks, three, and one key into a fourth."""
    qkv = _qkv(N, 64, N + 2)
    qd = torch.from_numpy(g8_encode(qkv.numpy(), 1.0)).cuda()
    ctx = _nan_ctx(N, 64)
    _check(lib, lib.cap_op_vit_attention(SPLIT, _p(qd), _p(ctx), B, N, H, 3, _stream()))
    torch.cuda.synchronize()
    err = _err(_decode(ctx, SPLIT), _attn_ref(qkv, N, 64))
    assert err < 1e-5, err
