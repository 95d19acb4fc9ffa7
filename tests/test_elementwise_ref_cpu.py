"""CPU: the host references of tests/_elementwise_ref.py against torch.nn.functional and numpy, so that the float64 side of
tests/test_elementwise_kernels_gpu.py is itself checked where there is no GPU."""
import numpy as np
import torch
import torch.nn.functional as F

import _elementwise_ref as E
from _util import g8_decode, g8_encode


def test_reference_helpers_match_torch_and_numpy():
    rng = np.random.default_rng(0)

    # LayerNorm
    y = (rng.standard_normal((5, 260)) * 3 + 1).astype(np.float32)
    gamma, beta = rng.standard_normal(260).astype(np.float32), rng.standard_normal(260).astype(np.float32)
    for eps in (1e-5, 1e-12):
        want = F.layer_norm(torch.from_numpy(y).double(), (260,), torch.from_numpy(gamma).double(), torch.from_numpy(beta).double(), eps)
        assert np.abs(E.layernorm64(y, gamma, beta, eps) - want.numpy()).max() < 1e-12

    # the embedding sums: fp32 adds in the stated order, ids clamped
    word, pos, type0 = (rng.standard_normal(s).astype(np.float32) for s in ((7, 8), (5, 8), (8,)))
    tok = np.array([0, 6, 3])
    assert np.array_equal(E.embed_sum32(word, pos, tok, 4), (torch.from_numpy(word)[tok] + torch.from_numpy(pos)[4]).numpy())
    ids = np.array([-1, 7, 2 ** 31 - 1, 3, 0], dtype=np.int32)
    want = (torch.from_numpy(word)[[0, 6, 6, 3, 0]] + torch.from_numpy(type0)) + torch.from_numpy(pos)[[0, 1, 0, 1, 0]]
    assert np.array_equal(E.embed_tokens_sum32(word, pos, type0, ids, 2), want.numpy())

    # prompt rows
    seq, fin, ln = E.init_prompt_seq(3, 4, np.array([[5, -2, 99]]), 10, 1)
    assert seq.tolist() == [[5, 0, 9, 1]] * 3 and fin.tolist() == [0, 0, 0] and ln.tolist() == [4, 4, 4]
    seq, _, _ = E.init_prompt_seq(2, 2, np.array([[1, 2], [3, 4]]), 10, 0)
    assert seq.tolist() == [[1, 2], [3, 4]]

    # split-K consumer: slice order in fp32
    part = rng.standard_normal((4, 3, 8)).astype(np.float32)
    bias = rng.standard_normal(8).astype(np.float32)
    t = torch.from_numpy(part)
    want = (((t[0] + t[1]) + t[2]) + t[3]) + torch.from_numpy(bias)
    assert np.array_equal(E.reduce_bias_act32(part, bias, 0), want.numpy())
    assert np.array_equal(E.reduce_bias_act32(part, bias, 2), want.clamp_min(0).numpy())
    assert np.array_equal(E.reduce_bias_act32(part[:1], None, 0), part[0])

    # mean pooling + F.normalize; lens clamped to [1, L]; a zero sentence gives zeros; the fp32 result is inside the bound
    x = rng.standard_normal((5, 7, 12)).astype(np.float32)
    x[4] = 0
    lens = [0, 1, 7, 12, 3]
    got, bound = E.mean_pool_normalize64(x, lens)
    for b, n in enumerate([1, 1, 7, 7, 3]):
        want = F.normalize(torch.from_numpy(x[b, :n]).double().mean(0), dim=0, eps=1e-12).numpy()
        assert np.abs(got[b] - want).max() < 1e-14
        f32 = F.normalize(torch.from_numpy(x[b, :n]).sum(0) * np.float32(1.0 / n), dim=0, eps=1e-12).numpy()
        assert (np.abs(f32 - got[b]) <= bound[b]).all()
    assert not got[4].any() and not bound[4].any()

    # patch order k = c ps^2 + dy ps + dx: F.unfold's
    for ps, img, B in ((14, 28, 2), (16, 48, 1)):
        px = rng.standard_normal((B, 3, img, img)).astype(np.float32)
        want = F.unfold(torch.from_numpy(px), kernel_size=ps, stride=ps).transpose(1, 2).reshape(-1, 3 * ps * ps)
        assert np.array_equal(E.patch_gather(px, ps), want.numpy())

    # u8 normalisation: float64 value, and the fp32 evaluation (contracted or not) is inside the bound
    u8 = rng.integers(0, 256, (2, 6, 6, 3), dtype=np.uint8)
    mean, std = np.array([0.48, 0.45, 0.40], np.float32), np.array([0.27, 0.26, 0.28], np.float32)
    v, bound = E.normalise_u8_64(u8, mean, std)
    want = ((torch.from_numpy(u8).double() / 255 - torch.from_numpy(mean).double()) / torch.from_numpy(std).double()).permute(0, 3, 1, 2)
    assert np.abs(v - want.numpy()).max() < 1e-15
    f32 = ((u8.astype(np.float32) * np.float32(1.0 / 255.0) - mean) / std).transpose(0, 3, 1, 2)
    assert (np.abs(f32 - v) <= bound).all()
    fma = (((u8.astype(np.float64) * np.float64(np.float32(1.0 / 255.0)) - mean.astype(np.float64)).astype(np.float32)) / std).transpose(0, 3, 1, 2)
    assert (np.abs(fma - v) <= bound).all()

    # the encodings: dense rows are _util's / torch's, pad columns keep the sentinel (half by half inside a cut G8 group)
    a = (rng.standard_normal((3, 12)) * 5).astype(np.float32)
    assert np.array_equal(E.encode("f32", a).view(np.float32), a)
    assert np.array_equal(E.encode("bf16", a), torch.from_numpy(a).to(torch.bfloat16).view(torch.int16).numpy())
    a16 = (rng.standard_normal((3, 16)) * 5).astype(np.float32)
    assert np.array_equal(E.encode("g8", a16), g8_encode(a16).view(np.int32))
    e = E.encode("g8", a, ld=16)
    h = e.view(np.int16).reshape(3, 2, 2, 8)
    full = g8_encode(np.pad(a, ((0, 0), (0, 4)))).view(np.int16).reshape(3, 2, 2, 8)
    assert np.array_equal(h[:, 0], full[:, 0]) and np.array_equal(h[:, 1, :, :4], full[:, 1, :, :4])
    assert np.array_equal(h[:, 1, :, 4:].reshape(-1).view(np.uint16) >> 8, np.full(3 * 2 * 4, 0x5A, np.uint16))
    assert np.abs(g8_decode(E.encode("g8", a16).view(np.float32)) - a16).max() <= np.abs(a16).max() * 2.0 ** -22
    e = E.encode("f32", a, ld=16)
    assert (e[:, 12:] == E.NAN32).all() and np.isnan(e.view(np.float32)[:, 12:]).all()
    bf = torch.from_numpy(a16).to(torch.bfloat16).float().numpy()
    assert (np.abs(bf - a16) <= E.store_error("bf16", a16)).all()
    assert (np.abs(g8_decode(g8_encode(a16)) - a16) <= E.store_error("g8", a16)).all()

    # compaction, absmax, selection
    fin = np.array([0, 1, 0, 2, -1, 0], np.int32)
    assert E.compact_rows(fin).tolist() == [0, 2, 5] and E.compact_rows(fin).dtype == np.int32
    assert E.absmax_bits(np.array([1.0, -3.5, -0.0], np.float32)) == int(np.float32(3.5).view(np.uint32))
    assert E.absmax_bits(np.array([-0.0], np.float32)) == 0
    assert E.absmax_bits(np.array([1.0, -np.inf], np.float32)) == 0x7F800000
    assert E.absmax_bits(np.array([1.0, np.nan], np.float32)) is None
    inf, nan = float("inf"), float("nan")
    z = np.array([[-inf, -inf, -inf, 9.0], [1.0, 1.0, 1.0, 9.0], [-inf, 2.0, -inf, 9.0], [nan, -inf, 1.0, 9.0], [nan, nan, nan, 9.0]], np.float32)
    assert E.greedy_expected(z, 3, 1, False).tolist() == [0, 0, 1, 2, 0]
    assert E.greedy_expected(z, 3, 1, True).tolist() == [0, 0, 0, 2, 0]
    assert int(torch.argmax(torch.full((5,), -inf))) == 0
