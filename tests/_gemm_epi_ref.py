"""Host index maps of the GEMM's address-computing epilogues (csrc/gemm.h: EPI_PATCH, EPI_CROSSKV, EPI_QKVCACHE, EPI_PARTIAL),
for tests/test_gemm_epilogues_gpu.py: each turns the row-major [M, N] matrix a plain store leaves into the image the epilogue
should leave in its buffer, with the mask of the elements it owns (everything else must keep the sentinel).  Written with views,
permutes and fancy indexing of whole arrays - no per-element offset arithmetic, which is the kernels' way and the thing under test;
tests/test_gemm_epi_ref_cpu.py checks each map against a loop-written form.  The maps move values of any dtype (bit patterns,
fp32, float64) and never round, except for patch_image's one add, which happens in the dtype of `plain`.  Never imported by the
product package."""
import numpy as np

EPI_STORE, EPI_PATCH, EPI_CROSSKV, EPI_QKVCACHE, EPI_PARTIAL = range(5)


def patch_image(plain, pos, B, P, ldc, fill=0):
    """plain [B * P, N] (row = image b, patch p), pos [P + 1, N] or None -> (image [B * (P + 1), ldc], mask): token row 1 + p of image
    b holds plain + pos[1 + p] (one add in plain's dtype); the class rows (token 0) and the pad columns N .. ldc are not owned"""
    plain = np.asarray(plain)
    N = plain.shape[1]
    assert plain.shape[0] == B * P and ldc >= N
    v = plain.reshape(B, P, N)
    if pos is not None:
        pos = np.asarray(pos, dtype=plain.dtype)
        assert pos.shape == (P + 1, N)
        v = (v + pos[None, 1:, :]).astype(plain.dtype)
    img = np.full((B, P + 1, ldc), fill, dtype=plain.dtype)
    mask = np.zeros((B, P + 1, ldc), dtype=bool)
    img[:, 1:, :N] = v
    mask[:, 1:, :N] = True
    return img.reshape(B * (P + 1), ldc), mask.reshape(B * (P + 1), ldc)


def crosskv_image(plain, n_img, tokens, heads, layers):
    """plain [n_img * tokens, layers * 2 * heads * 64] (column = layer, k | v, head, d) -> [layer][k | v][image][head][token][64]:
    a permutation, every element of the cache is owned"""
    plain = np.asarray(plain)
    assert plain.shape == (n_img * tokens, layers * 2 * heads * 64)
    return np.ascontiguousarray(plain.reshape(n_img, tokens, layers, 2, heads, 64).transpose(2, 3, 0, 4, 1, 5))


def qkvcache_image(plain, cap, H, Lmax, t, fill=0):
    """plain [M, 3 * H * 64] (q | k | v) -> (qbuf [M, H * 64], cache [k | v][cap][H][Lmax][64], mask of the cache): position t of
    the first M of the cache's `cap` rows is owned; qbuf is owned whole"""
    plain = np.asarray(plain)
    M = plain.shape[0]
    assert plain.shape[1] == 3 * H * 64 and M <= cap and 0 <= t < Lmax
    q, k, v = (plain[:, i * H * 64:(i + 1) * H * 64] for i in range(3))
    cache = np.full((2, cap, H, Lmax, 64), fill, dtype=plain.dtype)
    mask = np.zeros(cache.shape, dtype=bool)
    cache[0, :M, :, t, :] = k.reshape(M, H, 64)
    cache[1, :M, :, t, :] = v.reshape(M, H, 64)
    mask[:, :M, :, t, :] = True
    return np.ascontiguousarray(q), cache, mask


def partial_image(slices, M, N, ldc=None, rows=None, fill=0):
    """slices: S matrices [M, N] -> (image [S][M][ldc], mask): slice z holds slices[z]; with rows (the count-limited launch:
    whole live row tiles) only the first `rows` rows of every slice are owned; pad columns N .. ldc never are"""
    ldc = N if ldc is None else ldc
    rows = M if rows is None else rows
    S = len(slices)
    first = np.asarray(slices[0])
    assert ldc >= N and 0 <= rows <= M and all(np.asarray(s).shape == (M, N) for s in slices)
    img = np.full((S, M, ldc), fill, dtype=first.dtype)
    mask = np.zeros((S, M, ldc), dtype=bool)
    img[:, :rows, :N] = np.stack([np.asarray(s) for s in slices])[:, :rows]
    mask[:, :rows, :N] = True
    return img, mask


def live_rows(n, M, BM):
    """rows a launch with the live-row count n writes: the row tiles of height BM that start below n, cut at M"""
    return min(M, -(-min(n, M) // BM) * BM)


def with_sentinel(img_bits, mask, sentinel):
    """the bit image of a buffer that held `sentinel` everywhere and had the owned elements stored"""
    return np.where(mask, img_bits, np.array(sentinel).astype(img_bits.dtype))
