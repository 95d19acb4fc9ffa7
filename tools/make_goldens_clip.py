#!/usr/bin/env python
"""Golden fixtures of the CLIP scorer (tests/golden/clip_tiny.npz, clip_b32.npz) from HF `CLIPModel` in float64.

    python tools/make_goldens_clip.py            # writes both files
    python tools/make_goldens_clip.py --check    # recomputes and compares with the committed files

The independent implementation is transformers' `CLIPModel` (eager attention, float64), built from
`weights.procedural_clip_state_dict(arch, seed)` - the weights are re-drawn from the seed, never stored.  Images are
`weights.synthetic_frames_u8` frames (also re-drawn: the fixture keeps the seed, and for the tiny geometry the bytes), normalised
with the OpenAI mean / std in fp32 exactly as the device's CAP_PIX_U8_NHWC path does; captions are seeded id rows
`<sot> w.. <eot>` right padded with the EOT id (what `CLIPTokenizer(padding=True)` does).  Stored: pixel_values, ids, lens (the
pooled EOT position + 1), image_embeds / text_embeds (normalised), logits_per_image, and for a few synthetic groups of
(image, caption) pairs HF's ranking by paired logit (stable, descending) and the top-1 margin.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from embodied_captioning_amd.config import ClipArch  # noqa: E402
from embodied_captioning_amd.weights import procedural_clip_state_dict, synthetic_frames_u8  # noqa: E402

OPENAI_CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
OPENAI_CLIP_STD = (0.26862954, 0.26130258, 0.27577711)

# name -> (arch, weight seed, images, captions, frame seed, groups x pairs per group, store frames)
FIXTURES = {
    "clip_tiny": (ClipArch.tiny(), 3, 8, 12, 5, (4, 5), True),
    "clip_b32": (ClipArch(), 11, 16, 24, 13, (4, 6), False),
}


def hf_config_dict(a: ClipArch) -> dict:
    """The `CLIPConfig` of an arch (what `ClipArch.from_hf_config` reads back)."""
    common = dict(hidden_act=a.hidden_act, layer_norm_eps=a.eps)
    return dict(
        projection_dim=a.projection_dim, logit_scale_init_value=2.6592,
        text_config=dict(hidden_size=a.t_hidden, num_hidden_layers=a.t_layers, num_attention_heads=a.t_heads, intermediate_size=a.t_ffn,
                         vocab_size=a.vocab, max_position_embeddings=a.max_pos, bos_token_id=a.bos_token_id,
                         eos_token_id=a.eos_token_id, pad_token_id=a.pad_token_id, projection_dim=a.projection_dim, **common),
        vision_config=dict(hidden_size=a.v_hidden, num_hidden_layers=a.v_layers, num_attention_heads=a.v_heads, intermediate_size=a.v_mlp,
                           image_size=a.image_size, patch_size=a.patch_size, projection_dim=a.projection_dim, **common))


def hf_model(a: ClipArch, seed: int, dtype=torch.float64):
    from transformers import CLIPConfig, CLIPModel
    cfg = CLIPConfig(**hf_config_dict(a))
    cfg._attn_implementation = "eager"
    cfg.text_config._attn_implementation = "eager"
    cfg.vision_config._attn_implementation = "eager"
    m = CLIPModel(cfg).eval()
    sd = procedural_clip_state_dict(a, seed)
    missing, unexpected = m.load_state_dict(sd, strict=False)
    missing = [k for k in missing if not k.endswith("position_ids")]
    assert not missing and not unexpected, (missing, unexpected)
    return m.to(dtype)


def normalise_u8(frames: np.ndarray) -> np.ndarray:
    """uint8 [B, S, S, 3] -> fp32 [B, 3, S, S]: (x / 255 - mean) / std in fp32 (the device's CAP_PIX_U8_NHWC arithmetic)."""
    x = frames.astype(np.float32) / np.float32(255.0)
    x = (x - np.asarray(OPENAI_CLIP_MEAN, np.float32)) / np.asarray(OPENAI_CLIP_STD, np.float32)
    return np.ascontiguousarray(x.transpose(0, 3, 1, 2)).astype(np.float32)


def caption_ids(a: ClipArch, n: int, seed: int):
    """Seeded ragged captions: <sot> w.. <eot>, right padded with <eot> (the tokenizer's pad); lens = pooled position + 1."""
    rng = np.random.Generator(np.random.PCG64([seed, 0xC11F]))
    L = a.max_pos
    lens = rng.integers(3, min(L, 40) + 1, size=n)
    lens[0] = L
    if n > 3:
        lens[3] = 3
    ids = np.full((n, L), a.eos_token_id, dtype=np.int64)
    for b in range(n):
        k = int(lens[b])
        ids[b, 0] = a.bos_token_id
        ids[b, 1:k - 1] = rng.integers(1, min(a.bos_token_id, a.eos_token_id), size=k - 2)
    return ids, lens.astype(np.int64)


def groups_of(n_img: int, n_txt: int, shape, seed: int):
    rng = np.random.Generator(np.random.PCG64([seed, 0x6A0]))
    G, k = shape
    gi = np.stack([rng.choice(n_img, size=k, replace=n_img < k) for _ in range(G)])
    gt = np.stack([rng.choice(n_txt, size=k, replace=False) for _ in range(G)])
    return gi.astype(np.int64), gt.astype(np.int64)


def compute(name: str) -> dict:
    a, wseed, ni, nt, fseed, gshape, keep_frames = FIXTURES[name]
    frames = synthetic_frames_u8(ni, a.image_size, a.image_size, seed=fseed).numpy()
    px = normalise_u8(frames)
    ids, lens = caption_ids(a, nt, wseed)
    m = hf_model(a, wseed)
    with torch.no_grad():
        out = m(input_ids=torch.from_numpy(ids), pixel_values=torch.from_numpy(px).double())
    img = out.image_embeds.numpy()
    txt = out.text_embeds.numpy()
    lpi = out.logits_per_image.numpy()
    gi, gt = groups_of(ni, nt, gshape, wseed)
    scores = lpi[gi, gt]
    rank = np.stack([np.argsort(-s, kind="stable") for s in scores])
    srt = -np.sort(-scores, axis=1)
    res = dict(seed=np.int64(wseed), frame_seed=np.int64(fseed), n_images=np.int64(ni), pixel_values=px, ids=ids, lens=lens,
               image_embeds=img, text_embeds=txt, logits_per_image=lpi, group_images=gi, group_captions=gt, group_rank=rank,
               group_margin=srt[:, 0] - srt[:, 1], logit_scale=np.float64(float(m.logit_scale.item())))
    if keep_frames:
        res["frames"] = frames
    else:
        del res["pixel_values"]      # re-drawn from frame_seed (16 frames of 224 px would be 2.4 MB)
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    for name in FIXTURES:
        res = compute(name)
        path = os.path.join(ROOT, "tests", "golden", f"{name}.npz")
        if args.check:
            ref = np.load(path)
            for k in ("image_embeds", "text_embeds", "logits_per_image"):
                d = float(np.abs(ref[k] - res[k]).max())
                print(f"{name} {k}: max |diff| {d:.3g}")
        else:
            np.savez_compressed(path, **res)
            print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
