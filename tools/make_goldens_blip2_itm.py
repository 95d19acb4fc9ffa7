#!/usr/bin/env python
"""Golden fixtures of the BLIP-2 image-text scorer (tests/golden/blip2_itm_tiny.npz, blip2_itm_width.npz) from HF
`Blip2ForImageTextRetrieval` in float64.

    python tools/make_goldens_blip2_itm.py            # writes both files
    python tools/make_goldens_blip2_itm.py --check    # recomputes and compares with the committed files

The independent implementation is transformers' `Blip2ForImageTextRetrieval` (eager attention, float64), built from
`weights.procedural_blip2_itm_state_dict(arch, seed)` - the weights are re-drawn from the seed, never stored; the parity the
fixtures pin is therefore parity on PROCEDURAL weights.  Images are `weights.synthetic_frames_u8` frames (re-drawn from the
stored seed), normalised with the OpenAI CLIP mean / std in fp32 exactly as the device's CAP_PIX_U8_NHWC path does; captions are
seeded ragged id rows `[CLS] w.. [SEP]` right padded with the pad id, with their attention mask as `lens`.

Stored: ids, lens, ITC image / text features and the full ITC matrix, ITM logits and probabilities of the paired rows (image i
with caption i for i < n_images), synthetic groups of (image, caption) pairs with HF's ranking (stable, descending) and top-1
margin under both heads, and the reference's own rounding: the same model run in float32 and in bfloat16 on the CPU, per output
the maximum difference from float64 (`ref_err_fp32`, `ref_err_bf16`, entries in the order of ERR_KEYS; the features also as 1 -
cosine, which is what the bf16 bar uses as in the CLIP test) - the GPU tests' bars are multiples of these.  `blip2_itm_width` (production widths, two layers per tower) keeps compact outputs: the features as float32 and a second
geometry, 364 px (677 image tokens), under the `s364_` keys.
"""
from __future__ import annotations

import argparse
import dataclasses
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from embodied_captioning_amd.config import Blip2ItmArch  # noqa: E402
from embodied_captioning_amd.weights import procedural_blip2_itm_state_dict, synthetic_frames_u8  # noqa: E402

OPENAI_CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
OPENAI_CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
# the reference-error records: maximum absolute difference of each output, then 1 - cosine of the two feature sets
ERR_KEYS = ("itc_image", "itc_text", "itc_scores", "itm_logits", "itm_prob", "itc_image_cos", "itc_text_cos")

# name -> (arch, weight seed, images, captions, frame seed, groups x pairs per group, compact, extra image sizes)
FIXTURES = {
    "blip2_itm_tiny": (Blip2ItmArch.tiny(), 3, 8, 12, 5, (8, 5), False, ()),
    "blip2_itm_width": (Blip2ItmArch.width(224), 11, 3, 8, 13, (4, 4), True, (364,)),
}


def hf_model(a: Blip2ItmArch, seed: int, dtype=torch.float64, sd=None):
    from transformers import Blip2Config, Blip2ForImageTextRetrieval
    cfg = Blip2Config(**a.hf_config_dict())
    for c in (cfg, cfg.vision_config, cfg.qformer_config):
        c._attn_implementation = "eager"
    m = Blip2ForImageTextRetrieval(cfg).eval()
    sd = sd if sd is not None else procedural_blip2_itm_state_dict(a, seed)
    missing, unexpected = m.load_state_dict(sd, strict=False)
    missing = [k for k in missing if not k.endswith("position_ids")]
    assert not missing and not unexpected, (missing, unexpected)
    return m.to(dtype)


def normalise_u8(frames: np.ndarray) -> np.ndarray:
    """uint8 [B, S, S, 3] -> fp32 [B, 3, S, S]: (x / 255 - mean) / std in fp32 (the device's CAP_PIX_U8_NHWC arithmetic)."""
    x = frames.astype(np.float32) / np.float32(255.0)
    x = (x - np.asarray(OPENAI_CLIP_MEAN, np.float32)) / np.asarray(OPENAI_CLIP_STD, np.float32)
    return np.ascontiguousarray(x.transpose(0, 3, 1, 2)).astype(np.float32)


def caption_ids(a: Blip2ItmArch, n: int, seed: int):
    """Seeded ragged captions [CLS] w.. [SEP] (ids 1 / 2 stand for them; word ids from 3), right padded with the pad id; lens =
    tokens per row.  Row 0 has the full max_text_len tokens, row 3 two, row 5 one, row 6 three."""
    rng = np.random.Generator(np.random.PCG64([seed, 0xB11F]))
    L = a.max_text_len
    lens = rng.integers(4, L + 1, size=n)
    lens[0] = L
    for row, k in ((3, 2), (5, 1), (6, 3)):
        if n > row:
            lens[row] = k
    ids = np.full((n, L), a.pad, dtype=np.int64)
    for b in range(n):
        k = int(lens[b])
        ids[b, :k] = rng.integers(3, a.vocab, size=k)
        ids[b, 0] = 1
        if k > 1:
            ids[b, k - 1] = 2
    return ids, lens.astype(np.int64)


def groups_of(n_img: int, n_txt: int, shape, seed: int):
    rng = np.random.Generator(np.random.PCG64([seed, 0x6A0]))
    G, k = shape
    gi = np.stack([rng.choice(n_img, size=k, replace=n_img < k) for _ in range(G)])
    gt = np.stack([rng.choice(n_txt, size=k, replace=False) for _ in range(G)])
    return gi.astype(np.int64), gt.astype(np.int64)


def run_hf(m, px: np.ndarray, ids: np.ndarray, lens: np.ndarray, pairs_i: np.ndarray, pairs_t: np.ndarray, dtype) -> dict:
    """ITC features / matrix of all images x all captions and the ITM logits / probabilities of the listed (image, caption) pairs,
    returned as float64 arrays whatever `dtype` the model runs in."""
    mask = (np.arange(ids.shape[1])[None, :] < lens[:, None]).astype(np.int64)
    ids_t, mask_t, px_t = torch.from_numpy(ids), torch.from_numpy(mask), torch.from_numpy(px).to(dtype)
    with torch.no_grad():
        # the ITC features of either side do not depend on the other, so one call carries all images and all captions
        itc = m(pixel_values=px_t, input_ids=ids_t, attention_mask=mask_t)
        img, txt = itc.image_embeds.double(), itc.text_embeds.double()
        scores = torch.einsum("iqp,tp->iqt", img, txt).max(dim=1).values
        pi, pt = torch.from_numpy(pairs_i), torch.from_numpy(pairs_t)
        itm = m(pixel_values=px_t[pi], input_ids=ids_t[pt], attention_mask=mask_t[pt], use_image_text_matching_head=True)
        logits = itm.logits_per_image.double()
        prob = torch.softmax(itm.logits_per_image, dim=1)[:, 1].double()
    return dict(itc_image=img.numpy(), itc_text=txt.numpy(), itc_scores=scores.numpy(), itm_logits=logits.numpy(), itm_prob=prob.numpy())


def _cos_err(a: np.ndarray, b: np.ndarray) -> float:
    num = (a * b).sum(-1)
    den = np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1)
    return float((1.0 - num / den).max())


def ref_errors(ref: dict, low: dict) -> np.ndarray:
    """Per entry of ERR_KEYS: the maximum absolute difference, or for the `_cos` entries the largest 1 - cosine over the rows."""
    return np.array([_cos_err(ref[k[:-4]], low[k[:-4]]) if k.endswith("_cos") else float(np.abs(ref[k] - low[k]).max())
                     for k in ERR_KEYS], dtype=np.float64)


def _one_geometry(a: Blip2ItmArch, wseed: int, ni: int, nt: int, fseed: int, gshape, sd) -> dict:
    frames = synthetic_frames_u8(ni, a.image_size, a.image_size, seed=fseed).numpy()
    px = normalise_u8(frames)
    ids, lens = caption_ids(a, nt, wseed)
    gi, gt = groups_of(ni, nt, gshape, wseed)
    # ITM pairs: the diagonal (image i, caption i) first, then every pair of every group
    pairs_i = np.concatenate([np.arange(ni), gi.reshape(-1)])
    pairs_t = np.concatenate([np.arange(ni), gt.reshape(-1)])
    m = hf_model(a, wseed, torch.float64, sd)
    ref = run_hf(m, px, ids, lens, pairs_i, pairs_t, torch.float64)
    errs = {}
    for nm, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        errs[nm] = ref_errors(ref, run_hf(m.to(dt), px, ids, lens, pairs_i, pairs_t, dt))
    G, k = gshape
    itm_g = ref["itm_prob"][ni:].reshape(G, k)
    itc_g = ref["itc_scores"][gi, gt]
    res = dict(ids=ids, lens=lens, itc_image=ref["itc_image"], itc_text=ref["itc_text"], itc_scores=ref["itc_scores"],
               itm_logits=ref["itm_logits"][:ni], itm_prob=ref["itm_prob"][:ni], group_images=gi, group_captions=gt,
               group_itm_logits=ref["itm_logits"][ni:].reshape(G, k, 2), ref_err_fp32=errs["fp32"], ref_err_bf16=errs["bf16"])
    for nm, s in (("itm", itm_g), ("itc", itc_g)):
        srt = -np.sort(-s, axis=1)
        res[f"group_{nm}"] = s
        res[f"group_{nm}_rank"] = np.stack([np.argsort(-r, kind="stable") for r in s])
        res[f"group_{nm}_margin"] = srt[:, 0] - srt[:, 1]
    return res


def compute(name: str) -> dict:
    a, wseed, ni, nt, fseed, gshape, compact, extra = FIXTURES[name]
    sd = procedural_blip2_itm_state_dict(a, wseed)
    res = _one_geometry(a, wseed, ni, nt, fseed, gshape, sd)
    res.update(seed=np.int64(wseed), frame_seed=np.int64(fseed), n_images=np.int64(ni), image_size=np.int64(a.image_size))
    for S in extra:
        # the same weights at another image size: only the position table differs (drawn for its own number of tokens)
        b = dataclasses.replace(a, image_size=S)
        sub = _one_geometry(b, wseed, 2, 4, fseed, (2, 2), procedural_blip2_itm_state_dict(b, wseed))
        res.update({f"s{S}_{k}": v for k, v in sub.items()})
    if compact:
        for k in list(res):
            if k.endswith(("itc_image", "itc_text")):
                res[k] = res[k].astype(np.float32)      # 256-wide unit vectors: fp32 storage costs 6e-8, far below every bar
    return res


FLOAT_KEYS = ("itc_image", "itc_text", "itc_scores", "itm_logits", "itm_prob", "group_itm", "group_itc", "group_itm_margin",
              "group_itc_margin", "group_itm_logits", "ref_err_fp32", "ref_err_bf16")
INT_KEYS = ("ids", "lens", "group_images", "group_captions", "group_itm_rank", "group_itc_rank")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    for name in FIXTURES:
        if args.only and name != args.only:
            continue
        res = compute(name)
        path = os.path.join(ROOT, "tests", "golden", f"{name}.npz")
        if args.check:
            ref = np.load(path)
            for k in sorted(res):
                if k.split("_", 1)[-1] in FLOAT_KEYS or k in FLOAT_KEYS:
                    print(f"{name} {k}: max |diff| {float(np.abs(ref[k].astype(np.float64) - res[k].astype(np.float64)).max()):.3g}")
        else:
            np.savez_compressed(path, **res)
            print(f"wrote {path} ({os.path.getsize(path)} bytes)")
        for k in ("ref_err_fp32", "ref_err_bf16", "s364_ref_err_fp32", "s364_ref_err_bf16"):
            if k in res:
                print(f"  {k}: " + "  ".join(f"{n}={v:.3g}" for n, v in zip(ERR_KEYS, res[k])))
        for k in ("group_itm_margin", "group_itc_margin"):
            print(f"  {k}: {np.array2string(res[k], precision=4)}")


if __name__ == "__main__":
    main()
