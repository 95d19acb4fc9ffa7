"""CPU: the image-state record layout as the header states it (tests/_image_state_ref.py), the ABI surface of the feature, and the
host check of a state handed back to an engine.  No GPU call is made."""
import os
import re

import numpy as np
import pytest
import torch

import _image_state_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(2, 2, 37), (2, 2, 8), (1, 1, 1), (3, 4, 17)]          # slots, heads, tokens
KINDS = [0, 1, 2]


def _header():
    return open(os.path.join(ROOT, "include", "captioner_hip.h")).read()


def _header_formula(kind, slots, heads, tokens):
    """section_bytes = rows * row_bytes + (kind 2 ? round_up(rows * 4, 16) : 0); record_bytes = round_up(2 * slots * section_bytes, 256)"""
    rows, row_bytes = heads * tokens, {0: 256, 1: 128, 2: 128}[kind]
    section = rows * row_bytes + ((rows * 4 + 15) // 16 * 16 if kind == 2 else 0)
    return (2 * slots * section + 255) // 256 * 256


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("slots,heads,tokens", SHAPES)
def test_record_size_is_the_headers_formula(kind, slots, heads, tokens):
    n = R.record_bytes(kind, slots, heads, tokens)
    assert n == _header_formula(kind, slots, heads, tokens)
    assert n % 256 == 0 and R.section_bytes(kind, heads, tokens) % 16 == 0
    assert "round_up(2 * slots * section_bytes, 256)" in _header() and "round_up(rows * 4, 16)" in _header()


def test_a_blip_base_kv16_record_is_about_seven_and_a_half_megabytes():
    """12 layers, 12 heads, 197 image tokens: the byte count the bandwidth figures in the documents start from"""
    assert abs(R.record_bytes(2, 12, 12, 197) / 1e6 - 7.5) < 0.05


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("slots,heads,tokens", SHAPES)
def test_pack_then_unpack_round_trips_and_touches_nothing_else(kind, slots, heads, tokens):
    rng = np.random.default_rng(kind * 100 + tokens)
    B, rows = 5, heads * tokens
    n = R.cache_bytes(kind, slots, heads, tokens, B)
    cache = rng.integers(0, 256, size=n, dtype=np.uint8)
    rec = R.pack(cache, kind, slots, heads, tokens, B)
    assert rec.shape == (B, R.record_bytes(kind, slots, heads, tokens))
    assert not rec[:, 2 * slots * R.section_bytes(kind, heads, tokens):].any()          # the closing padding is zeros
    # the same images back into a cache for the same B, over two different fills: what differs from both fills was written
    back_a = R.unpack(rec, np.full(n + 512, 0xA5, dtype=np.uint8), kind, slots, heads, tokens)
    back_b = R.unpack(rec, np.full(n + 512, 0x5A, dtype=np.uint8), kind, slots, heads, tokens)
    touched = (back_a != 0xA5) | (back_b != 0x5A)
    assert int(touched.sum()) == B * 2 * slots * rows * (R.ROW_BYTES[kind] + (4 if kind == 2 else 0))          # rows and scales, nothing else
    assert not touched[n:].any()
    assert np.array_equal(back_a[:n][touched[:n]], cache[touched[:n]]) and np.array_equal(back_b[:n][touched[:n]], cache[touched[:n]])
    assert np.array_equal(R.pack(back_a[:n], kind, slots, heads, tokens, B), rec)
    # a selection of images for another batch size: packing what was unpacked gives the selected records
    sel = [4, 0, 0, 2]
    other = R.unpack(rec[sel], back_a, kind, slots, heads, tokens)
    assert np.array_equal(R.pack(other[: R.cache_bytes(kind, slots, heads, tokens, len(sel))], kind, slots, heads, tokens, len(sel)), rec[sel])


def test_kv16_rows_of_one_image_move_with_the_batch():
    """74 rows per image: image 1 starts inside a group of 32, so its record lands on other offsets as the only image of another call"""
    kind, slots, heads, tokens = 2, 1, 2, 37
    rng = np.random.default_rng(7)
    cache = rng.integers(0, 256, size=R.cache_bytes(kind, slots, heads, tokens, 2), dtype=np.uint8)
    rec = R.pack(cache, kind, slots, heads, tokens, 2)
    assert np.array_equal(rec[1, :128], cache[(74 // 32) * 4224 + (74 % 32) * 128:][:128])          # head row 74 of the block: group 2, row 10
    assert np.array_equal(rec[1, 74 * 128: 74 * 128 + 4], cache[(74 // 32) * 4224 + 4096 + (74 % 32) * 4:][:4])          # and its scale
    alone = R.unpack(rec[1:2], np.zeros(R.cache_bytes(kind, slots, heads, tokens, 1), dtype=np.uint8), kind, slots, heads, tokens)
    assert np.array_equal(alone[:128], rec[1, :128])          # there it is head row 0
    assert np.array_equal(R.pack(alone, kind, slots, heads, tokens, 1), rec[1:2])


def test_header_native_exports_and_pixel_format_agree():
    from embodied_captioning_amd import _native as N
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"enum\s*\{([^}]*CAP_PIX_IMAGE_STATE[^}]*)\}", text)
    assert m, "the header declares CAP_PIX_IMAGE_STATE beside the other pixel formats"
    vals = {k.strip(): int(v) for k, v in (item.split("=") for item in m.group(1).split(","))}
    assert vals == {"CAP_PIX_F32_NCHW": N.CAP_PIX_F32_NCHW, "CAP_PIX_U8_NHWC": N.CAP_PIX_U8_NHWC, "CAP_PIX_IMAGE_STATE": N.CAP_PIX_IMAGE_STATE}
    assert N.CAP_PIX_IMAGE_STATE == 2
    declared = set(re.findall(r"\b(cap_[a-z0-9_]+)\s*\(", text))
    for name in ("cap_image_state_bytes", "cap_encode_image_state", "cap_op_image_state_pack", "cap_op_image_state_unpack"):
        assert name in declared and name in N.EXPORTS
    # the request struct did not grow: callers fill it without a size field
    body = re.search(r"typedef struct CapGenerateArgs \{(.*?)\} CapGenerateArgs;", text, flags=re.S).group(1)
    fields = [re.sub(r"[\*\s]", "", d.split()[-1]) for d in body.split(";") if d.strip()]
    assert fields == [f[0] for f in N.CapGenerateArgs._fields_] and len(fields) == 18


def test_a_state_is_told_from_frames_by_its_two_dimensions():
    from embodied_captioning_amd.engine import is_image_state
    assert is_image_state(torch.zeros((3, 512), dtype=torch.uint8))
    assert not is_image_state(torch.zeros((3, 16, 16, 3), dtype=torch.uint8))
    assert not is_image_state(torch.zeros((3, 512), dtype=torch.float32))
    assert not is_image_state([[0, 1]])


def test_a_state_of_another_row_size_is_refused_with_both_sizes_named():
    from embodied_captioning_amd.engine import validate_image_state
    validate_image_state(torch.zeros((2, 1024), dtype=torch.uint8), 1024)
    with pytest.raises(ValueError) as e:
        validate_image_state(torch.zeros((2, 768), dtype=torch.uint8), 1024)
    msg = str(e.value)
    assert "768" in msg and "1024" in msg
    assert "architecture" in msg and "compute type" in msg and "cross-cache kind" in msg
    with pytest.raises(ValueError):
        validate_image_state(torch.zeros((0, 1024), dtype=torch.uint8), 1024)
    with pytest.raises(ValueError):
        validate_image_state(torch.zeros((2, 4, 4, 3), dtype=torch.uint8), 1024)


def test_wrappers_take_images_or_a_state_never_both_or_neither():
    from embodied_captioning_amd.engine import images_or_state
    st = torch.zeros((2, 256), dtype=torch.uint8)
    assert images_or_state(None, st, "generate_batch") is st
    assert images_or_state("images", None, "generate_batch") == "images"
    for images, state in ((None, None), ("images", st)):
        with pytest.raises(ValueError, match="generate_batch"):
            images_or_state(images, state, "generate_batch")
    with pytest.raises(ValueError, match="image_state"):
        images_or_state(None, torch.zeros((2, 4, 4, 3), dtype=torch.uint8), "score_captions")
