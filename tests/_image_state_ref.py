"""numpy restatement of the image-state record layout of include/captioner_hip.h ("image state") for the cross K/V cache kinds.

cache: the bytes of a cross-attention K/V cache packed for B images, [slot][k | v][image][head][token][64]; every (slot, k | v) block
holds the B * heads * tokens head rows one after the other - kind 0: 256-byte fp32 rows, kind 1: 128-byte bf16 rows, kind 2 (KV16):
groups of 32 rows = [32 x 128 bytes][32 fp32 scales] = 4224 bytes, the block padded to whole groups.
record: per image, for each slot k then v: the heads * tokens row payloads in [head][token] order, then (kind 2) the rows' fp32 scales
padded to 16 bytes; the record padded with zeros to a multiple of 256 bytes."""
import numpy as np

ROW_BYTES = {0: 256, 1: 128, 2: 128}
KV16_GROUP_ROWS, KV16_GROUP_BYTES = 32, 32 * 128 + 32 * 4


def _up(n, m):
    return (n + m - 1) // m * m


def section_bytes(kind, heads, tokens):
    rows = heads * tokens
    return rows * ROW_BYTES[kind] + (_up(rows * 4, 16) if kind == 2 else 0)


def record_bytes(kind, slots, heads, tokens):
    return _up(2 * slots * section_bytes(kind, heads, tokens), 256)


def block_bytes(kind, n_rows):
    """one (slot, k | v) block of the cache holding n_rows head rows"""
    return _up(n_rows, KV16_GROUP_ROWS) // KV16_GROUP_ROWS * KV16_GROUP_BYTES if kind == 2 else n_rows * ROW_BYTES[kind]


def cache_bytes(kind, slots, heads, tokens, B):
    return 2 * slots * block_bytes(kind, B * heads * tokens)


def _row_offsets(kind, ri):
    """byte offsets, inside a block, of the payloads (and for kind 2 the scales) of the head rows `ri`"""
    ri = np.asarray(ri, dtype=np.int64)
    if kind != 2:
        return ri * ROW_BYTES[kind], None
    g, r = ri // KV16_GROUP_ROWS, ri % KV16_GROUP_ROWS
    return g * KV16_GROUP_BYTES + r * 128, g * KV16_GROUP_BYTES + 32 * 128 + r * 4


def _gather(offsets, width):
    return (offsets[:, None] + np.arange(width, dtype=np.int64)[None, :]).reshape(-1)


def pack(cache, kind, slots, heads, tokens, B):
    """cache bytes (packed for B images) -> uint8 [B, record_bytes], padding zero"""
    cache = np.asarray(cache, dtype=np.uint8).reshape(-1)
    rows, rb = heads * tokens, ROW_BYTES[kind]
    blk, sec = block_bytes(kind, B * rows), section_bytes(kind, heads, tokens)
    out = np.zeros((B, record_bytes(kind, slots, heads, tokens)), dtype=np.uint8)
    for b in range(B):
        pay, sc = _row_offsets(kind, b * rows + np.arange(rows))
        for s in range(2 * slots):
            out[b, s * sec: s * sec + rows * rb] = cache[s * blk + _gather(pay, rb)]
            if sc is not None:
                out[b, s * sec + rows * rb: s * sec + rows * rb + rows * 4] = cache[s * blk + _gather(sc, 4)]
    return out


def unpack(state, cache, kind, slots, heads, tokens):
    """records uint8 [B, record_bytes] -> a copy of `cache` (at least cache_bytes(.., B) bytes) with the B images' rows, laid out for
    B images, written over it; every other byte as it was"""
    state = np.asarray(state, dtype=np.uint8)
    B = state.shape[0]
    assert state.shape[1] == record_bytes(kind, slots, heads, tokens)
    out = np.array(cache, dtype=np.uint8).reshape(-1).copy()
    rows, rb = heads * tokens, ROW_BYTES[kind]
    blk, sec = block_bytes(kind, B * rows), section_bytes(kind, heads, tokens)
    assert out.size >= 2 * slots * blk
    for b in range(B):
        pay, sc = _row_offsets(kind, b * rows + np.arange(rows))
        for s in range(2 * slots):
            out[s * blk + _gather(pay, rb)] = state[b, s * sec: s * sec + rows * rb]
            if sc is not None:
                out[s * blk + _gather(sc, 4)] = state[b, s * sec + rows * rb: s * sec + rows * rb + rows * 4]
    return out
