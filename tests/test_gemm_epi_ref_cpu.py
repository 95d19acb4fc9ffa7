"""CPU: the host index maps of tests/_gemm_epi_ref.py against a second, loop-written form of each map (one element at a time, from
the layouts csrc/gemm.h documents), at the small geometries of tests/test_gemm_epilogues_gpu.py - so that the expected images of
the GPU tests are themselves checked where there is no GPU.  Every source element must land exactly once and on an owned element:
mask and owned elements partition the buffer."""
import numpy as np
import pytest

import _gemm_epi_ref as G

FILL = -7


def _ids(M, N):
    """a matrix whose every element is its own flat index: an image of it shows where each element went"""
    return np.arange(M * N, dtype=np.int64).reshape(M, N)


def _partition(img, mask, n_src):
    """the owned elements hold every source index exactly once; the others hold the fill"""
    assert mask.sum() == n_src
    assert np.array_equal(np.sort(img[mask]), np.arange(n_src))
    assert (img[~mask] == FILL).all()


@pytest.mark.parametrize("B,P,N,ldc", [(1, 5, 64, 64), (7, 49, 192, 192), (3, 196, 328, 328), (2, 50, 128, 160)])
def test_patch_image(B, P, N, ldc):
    plain = _ids(B * P, N)
    img, mask = G.patch_image(plain, None, B, P, ldc, fill=FILL)
    want = np.full((B * (P + 1), ldc), FILL, dtype=np.int64)
    for b in range(B):
        for p in range(P):
            for c in range(N):
                want[b * (P + 1) + 1 + p, c] = plain[b * P + p, c]
    assert np.array_equal(img, want)
    assert np.array_equal(mask, want != FILL)
    _partition(img, mask, B * P * N)
    assert not mask.reshape(B, P + 1, ldc)[:, 0].any() and not mask[:, N:].any()      # class rows and pad columns
    # the position row: token 1 + p, pitch N, one add in the dtype of `plain`
    rng = np.random.default_rng(B + P)
    x = rng.standard_normal((B * P, N)).astype(np.float32)
    pos = rng.standard_normal((P + 1, N)).astype(np.float32)
    got, _ = G.patch_image(x, pos, B, P, ldc)
    assert got.dtype == np.float32
    for b, p in ((0, 0), (B - 1, P - 1), (B // 2, P // 2)):
        assert np.array_equal(got[b * (P + 1) + 1 + p, :N], x[b * P + p] + pos[1 + p])
    got64, _ = G.patch_image(x.astype(np.float64), pos, B, P, ldc)
    assert got64.dtype == np.float64 and np.array_equal(got64[-1, :N], x[-1].astype(np.float64) + pos[P].astype(np.float64))


@pytest.mark.parametrize("n_img,tokens,heads,layers", [(2, 50, 2, 3), (9, 33, 1, 2), (3, 197, 12, 2)])
def test_crosskv_image(n_img, tokens, heads, layers):
    M, N = n_img * tokens, layers * 2 * heads * 64
    plain = _ids(M, N)
    img = G.crosskv_image(plain, n_img, tokens, heads, layers)
    assert img.shape == (layers, 2, n_img, heads, tokens, 64)
    want = np.full(img.shape, FILL, dtype=np.int64)
    for l in range(layers):
        for kv in range(2):
            for h in range(heads):
                col0 = (l * 2 + kv) * heads * 64 + h * 64
                for b in range(n_img):
                    for t in range(tokens):
                        want[l, kv, b, h, t] = plain[b * tokens + t, col0:col0 + 64]
    assert np.array_equal(img, want)
    _partition(img, np.ones(img.shape, dtype=bool), M * N)


@pytest.mark.parametrize("R,cap,H,Lmax,t", [(37, 40, 2, 40, 0), (37, 40, 2, 40, 33), (37, 40, 2, 40, 39), (300, 300, 12, 48, 35)])
def test_qkvcache_image(R, cap, H, Lmax, t):
    D = H * 64
    plain = _ids(R, 3 * D)
    q, cache, mask = G.qkvcache_image(plain, cap, H, Lmax, t, fill=FILL)
    want_q = np.full((R, D), FILL, dtype=np.int64)
    want_c = np.full((2, cap, H, Lmax, 64), FILL, dtype=np.int64)
    for r in range(R):
        for c in range(3 * D):
            part, hd = divmod(c, D)
            if part == 0:
                want_q[r, c] = plain[r, c]
            else:
                want_c[part - 1, r, hd // 64, t, hd % 64] = plain[r, c]
    assert np.array_equal(q, want_q) and np.array_equal(cache, want_c) and np.array_equal(mask, want_c != FILL)
    # q and the owned cache elements together hold every source element once
    both = np.concatenate([q.reshape(-1), cache[mask]])
    assert np.array_equal(np.sort(both), np.arange(R * 3 * D))
    assert (cache[~mask] == FILL).all()
    assert not mask[:, R:].any() and not np.delete(mask, t, axis=3).any()             # rows up to the capacity, other positions


@pytest.mark.parametrize("M,N,S,ldc", [(37, 768, 3, 768), (5, 200, 2, 200), (300, 768, 4, 768), (64, 2304, 1, 2304), (5, 200, 2, 208)])
def test_partial_image(M, N, S, ldc):
    src = _ids(S * M, N).reshape(S, M, N)
    for rows in (None, 0, 1, M):
        img, mask = G.partial_image(list(src), M, N, ldc=ldc, rows=rows, fill=FILL)
        n = M if rows is None else rows
        want = np.full((S, M, ldc), FILL, dtype=np.int64)
        for z in range(S):
            for r in range(n):
                for c in range(N):
                    want[z, r, c] = src[z, r, c]
        assert np.array_equal(img, want) and np.array_equal(mask, want != FILL)
        if n == M:
            _partition(img, mask, S * M * N)


def test_live_rows_and_sentinel_image():
    # whole row tiles that start below the count, cut at M
    assert [G.live_rows(n, 300, 64) for n in (0, 1, 64, 65, 300)] == [0, 64, 64, 128, 300]
    assert [G.live_rows(n, 300, 128) for n in (0, 1, 64, 65, 300)] == [0, 128, 128, 128, 300]
    assert [G.live_rows(n, 300, 256) for n in (0, 1, 64, 65, 300, 999)] == [0, 256, 256, 256, 300, 300]
    assert [G.live_rows(n, 5, 64) for n in (0, 1, 64)] == [0, 5, 5]
    img = np.array([[1, 2], [3, 4]], dtype=np.int32)
    mask = np.array([[True, False], [False, True]])
    assert G.with_sentinel(img, mask, 0x7FC00000).tolist() == [[1, 0x7FC00000], [0x7FC00000, 4]]
    assert G.with_sentinel(img.astype(np.int16), mask, 0x7FC0).dtype == np.int16
