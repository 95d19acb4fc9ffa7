"""BLIP-2 image-text matching (ITM) and contrastive (ITC) scoring on the device - what the reference's `--method blip2_itm |
blip2_itc` runs per (crop, caption) pair with the LAVIS `blip2_image_text_matching` model
(experimenting_env/captioner/pseudocaptioner.py:34-37, :193-308), for whole lists of pairs; the arithmetic is HF
`Blip2ForImageTextRetrieval.forward`, the HF port of that model.

Images: PIL images or uint8 HWC RGB arrays are resized on the device as LAVIS `blip_image_eval` does (a straight BICUBIC resize to
S x S, bit-exact with Pillow, then the CLIP mean / std); uint8 [n, S, S, 3] and normalised [n, 3, S, S] tensors go in as they are.
Captions: the checkpoint's BERT tokenizer with the reference's settings (`truncation=True, max_length=32`: a long caption is
TRUNCATED, as the reference does - unlike the CLIP scorer, which refuses).  `procedural-blip2-itm[-tiny][:seed]` names a seeded
checkpoint without a vocabulary: captions are then id rows ([CLS] w.. [SEP]).  Only HF-format checkpoint directories are read (LAVIS
`.pth` key names are not).
"""
from __future__ import annotations

from typing import List, Sequence, Union

import torch

from ..config import Blip2ItmArch
from ..preprocess import pad_rows, pixel_batches

PROCEDURAL = "procedural-blip2-itm"
HEADS = ("itm", "itc")


def _parse_procedural(name: str):
    base, _, seed = name.partition(":")
    if base not in (PROCEDURAL, PROCEDURAL + "-tiny"):
        return None
    return (Blip2ItmArch.tiny() if base.endswith("-tiny") else Blip2ItmArch()), int(seed or 0)


def tokenize_captions(tokenizer, captions: Sequence[Union[str, Sequence[int]]], max_length: int = 32) -> List[List[int]]:
    """Captions -> id rows incl. [CLS] / [SEP], as the reference tokenises (:292): `tokenizer(c, truncation=True,
    max_length=max_length)`.  tokenizer None: captions must be id rows, which are cut to max_length the same way (the last kept id
    is the row's last id, as BERT truncation keeps [SEP])."""
    rows = []
    for c in captions:
        if isinstance(c, str):
            if tokenizer is None:
                raise TypeError("this checkpoint has no vocabulary: pass captions as id rows")
            r = [int(v) for v in tokenizer(c, truncation=True, max_length=max_length)["input_ids"]]
        else:
            r = [int(v) for v in c]
            if len(r) > max_length:
                r = r[:max_length - 1] + r[-1:]
        if not r:
            raise ValueError("empty caption id row")
        rows.append(r)
    return rows


class Blip2ItmScorer:
    """name: a local HF `Blip2ForImageTextRetrieval` directory, a cached hub id (e.g. "Salesforce/blip2-itm-vit-g-coco", the
    checkpoint the reference's LAVIS "coco" type names) or procedural-blip2-itm[-tiny][:seed]."""

    def __init__(self, name: str = "Salesforce/blip2-itm-vit-g-coco", device: str = "cuda:0", dtype: str = "f32s", batch_size: int = 256):
        from ..engine import Blip2ItmEngine
        if batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        if dtype not in ("f32", "f32s", "bf16"):
            raise ValueError(f"dtype {dtype!r}: the BLIP-2 image-text scorer runs 'f32', 'f32s' or 'bf16' (no int8)")
        self.name, self.device, self.batch_size = name, torch.device(device), int(batch_size)
        proc = _parse_procedural(name)
        self.tokenizer = None
        if proc is not None:
            self.arch, seed = proc
            sd = None                      # drawn once the engine exists: without a GPU nothing is drawn
        else:
            from ..weights import load_hf_blip2_itm_checkpoint, resolve_hf_dir
            path = resolve_hf_dir(name)
            if path is None:
                raise FileNotFoundError(f"BLIP-2 ITM checkpoint {name!r} is neither a directory nor in the local HF cache "
                                        f"(HF-format directories only; LAVIS .pth files are not read)")
            self.arch, sd = load_hf_blip2_itm_checkpoint(path)
            from transformers import AutoTokenizer
            self.tokenizer = AutoTokenizer.from_pretrained(path)
        self.engine = Blip2ItmEngine(self.arch, dtype=dtype, max_batch=self.batch_size, device=self.device)
        if sd is None:
            from ..weights import procedural_blip2_itm_state_dict
            sd = procedural_blip2_itm_state_dict(self.arch, seed)
        self.engine.load_state_dict(sd)

    def close(self) -> None:
        self.engine.close()

    # ------------------------------------------------------------------------------------------ text
    def tokenize(self, captions) -> List[List[int]]:
        return tokenize_captions(self.tokenizer, captions, self.arch.max_text_len)

    def get_text_features(self, captions) -> torch.Tensor:
        """-> fp32 [n, projection_dim] on the device, L2-normalised (HF's ITC `text_embeds`)."""
        rows = self.tokenize(captions)
        outs = [self.engine.itc_text_features(*pad_rows(rows[i:i + self.batch_size], self.arch.pad))
                for i in range(0, len(rows), self.batch_size)]
        if not outs:
            return torch.empty((0, self.arch.projection_dim), device=self.device)
        return outs[0] if len(outs) == 1 else torch.cat(outs)

    # ------------------------------------------------------------------------------------------ images
    def _pixel_batches(self, images):
        return pixel_batches(images, self.arch.image_size, self.batch_size, self.device, center_crop=False)

    def get_image_features(self, images) -> torch.Tensor:
        """-> fp32 [n, num_query_tokens, projection_dim] on the device, rows L2-normalised (HF's ITC `image_embeds`)."""
        outs = []
        for px in self._pixel_batches(images):
            self.engine.encode_images(px)
            outs.append(self.engine.itc_image_features())
        if not outs:
            return torch.empty((0, self.arch.num_query_tokens, self.arch.projection_dim), device=self.device)
        return outs[0] if len(outs) == 1 else torch.cat(outs)

    # ------------------------------------------------------------------------------------------ scores
    def score_pairs(self, images, captions, head: str = "itm", return_logits: bool = False) -> torch.Tensor:
        """Image i against caption i -> fp32 [n] on the device: head "itm" = softmax(ITM logits)[:, 1], head "itc" = max over the
        queries of the cosine similarity - the reference's `itm_score` / `itc_score` of each pair alone.  The ViT-g runs once per
        image.  return_logits (itm only): the [n, 2] logits as well."""
        if head not in HEADS:
            raise ValueError(f"head must be one of {HEADS}, got {head!r}")
        if return_logits and head != "itm":
            raise ValueError("return_logits is for head 'itm'")
        rows = self.tokenize(captions)
        outs, logits, i = [], [], 0
        for px in self._pixel_batches(images):
            n = px.shape[0]
            chunk = rows[i:i + n]
            if len(chunk) != n:
                break
            i += n
            self.engine.encode_images(px)
            ids, lens = pad_rows(chunk, self.arch.pad)
            if head == "itm":
                lg, pr = self.engine.itm(ids, lens)
                outs.append(pr)
                logits.append(lg)
            else:
                outs.append(self.engine.itc_scores(self.engine.itc_image_features(), self.engine.itc_text_features(ids, lens), paired=True))
        n_img = sum(o.shape[0] for o in outs)
        if i != len(rows) or n_img != len(rows):
            raise ValueError(f"{len(rows)} captions against a different number of images")
        if not outs:
            empty = torch.empty((0,), device=self.device)
            return (empty, torch.empty((0, 2), device=self.device)) if return_logits else empty
        sc = outs[0] if len(outs) == 1 else torch.cat(outs)
        if return_logits:
            return sc, (logits[0] if len(logits) == 1 else torch.cat(logits))
        return sc

    def itc_matrix(self, images, captions) -> torch.Tensor:
        """fp32 [n_images, n_captions] on the device (HF's ITC `logits_per_image`)."""
        return self.engine.itc_scores(self.get_image_features(images), self.get_text_features(captions), paired=False)
