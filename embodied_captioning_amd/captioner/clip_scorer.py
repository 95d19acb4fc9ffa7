"""CLIP image-caption scoring on the device - what the reference's `--method clip` runs per (crop, caption) pair with HF
`CLIPModel` / `CLIPProcessor` (experimenting_env/captioner/pseudocaptioner.py:39-46, :352-357), for whole lists of pairs.

Images: PIL images or uint8 HWC RGB arrays are resized on the device with HF `CLIPImageProcessorPil`'s geometry (shortest edge to
the image size with the long side truncated, centre crop; bit-exact with Pillow's BICUBIC - preprocess.hf_shortest_edge_geometry),
normalised tensors [n, 3, S, S] go in as they are.  Captions: the checkpoint's own tokenizer (`transformers.CLIPTokenizer`), the
pooled row by HF's rule (`eos_token_id == 2`: argmax of the ids, the legacy OpenAI configs; otherwise the first `eos_token_id`).
A caption longer than the text tower's positions is refused by name, never truncated.  `procedural-clip[-tiny][:seed]` names a
seeded checkpoint without a vocabulary: captions are then id sequences (<sot> .. <eot>), as SentenceEncoder takes them.
"""
from __future__ import annotations

from typing import List, Sequence, Union

import numpy as np
import torch

from ..config import ClipArch
from ..preprocess import pad_rows, pixel_batches

PROCEDURAL = "procedural-clip"


def _parse_procedural(name: str):
    base, _, seed = name.partition(":")
    if base not in (PROCEDURAL, PROCEDURAL + "-tiny"):
        return None
    return (ClipArch.tiny() if base.endswith("-tiny") else ClipArch()), int(seed or 0)


def pooled_positions(ids: Sequence[Sequence[int]], eos_token_id: int) -> List[int]:
    """HF CLIPTextTransformer's pooled row of each id row: argmax(ids) when eos_token_id == 2, else the first eos_token_id (a row
    without one pools at argmax of (ids == eos) = 0, as HF does)."""
    out = []
    for row in ids:
        r = np.asarray(row, dtype=np.int64)
        out.append(int(r.argmax()) if eos_token_id == 2 else int((r == eos_token_id).argmax()))
    return out


def tokenize_captions(tokenizer, captions: Sequence[Union[str, Sequence[int]]], max_pos: int) -> List[List[int]]:
    """Captions -> id rows incl. <sot> / <eot> through the checkpoint's tokenizer (None: captions must be id sequences).  A row
    longer than `max_pos` raises, naming the caption."""
    rows = []
    for c in captions:
        if isinstance(c, str):
            if tokenizer is None:
                raise TypeError("this checkpoint has no vocabulary: pass captions as id sequences")
            rows.append([int(v) for v in tokenizer(c)["input_ids"]])
        else:
            rows.append([int(v) for v in c])
        if len(rows[-1]) > max_pos:
            raise ValueError(f"caption {c!r} is {len(rows[-1])} tokens; the CLIP text tower takes at most {max_pos} (it is not truncated)")
        if not rows[-1]:
            raise ValueError("empty caption id row")
    return rows


class ClipScorer:
    """name: a local HF CLIP directory, a cached hub id (e.g. "openai/clip-vit-base-patch32") or procedural-clip[-tiny][:seed]."""

    def __init__(self, name: str = "openai/clip-vit-base-patch32", device: str = "cuda:0", dtype: str = "f32s", batch_size: int = 256):
        from ..engine import ClipEngine
        if batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        self.name, self.device, self.batch_size = name, torch.device(device), int(batch_size)
        proc = _parse_procedural(name)
        self.tokenizer = None
        if proc is not None:
            from ..weights import procedural_clip_state_dict
            self.arch, seed = proc
            sd = procedural_clip_state_dict(self.arch, seed)
        else:
            from ..weights import load_hf_clip_checkpoint, resolve_hf_dir
            path = resolve_hf_dir(name)
            if path is None:
                raise FileNotFoundError(f"CLIP checkpoint {name!r} is neither a directory nor in the local HF cache")
            self.arch, sd = load_hf_clip_checkpoint(path)
            from transformers import CLIPTokenizer
            self.tokenizer = CLIPTokenizer.from_pretrained(path)
        self.engine = ClipEngine(self.arch, dtype=dtype, max_batch=self.batch_size, device=self.device)
        self.engine.load_state_dict(sd)

    def close(self) -> None:
        self.engine.close()

    # ------------------------------------------------------------------------------------------ text
    def tokenize(self, captions: Sequence[Union[str, Sequence[int]]]) -> List[List[int]]:
        """-> id rows incl. <sot> / <eot>.  A procedural scorer takes id sequences only."""
        return tokenize_captions(self.tokenizer, captions, self.arch.max_pos)

    def get_text_features(self, captions) -> torch.Tensor:
        """-> fp32 [n, projection_dim] on the device, L2-normalised (HF's `text_embeds`)."""
        rows = self.tokenize(captions)
        pos = pooled_positions(rows, self.arch.eos_token_id)
        outs = []
        for i in range(0, len(rows), self.batch_size):
            ids, _ = pad_rows(rows[i:i + self.batch_size], self.arch.pad_token_id)
            lens = torch.tensor([q + 1 for q in pos[i:i + self.batch_size]], dtype=torch.int32)      # up to the pooled row, not the row's end
            outs.append(self.engine.embed_text(ids, lens))
        if not outs:
            return torch.empty((0, self.arch.projection_dim), device=self.device)
        return outs[0] if len(outs) == 1 else torch.cat(outs)

    # ------------------------------------------------------------------------------------------ images
    def get_image_features(self, images) -> torch.Tensor:
        """-> fp32 [n, projection_dim] on the device, L2-normalised (HF's `image_embeds`)."""
        batches = pixel_batches(images, self.arch.image_size, self.batch_size, self.device, center_crop=True, geometry="hf")
        outs = [self.engine.embed_images(px) for px in batches]
        if not outs:
            return torch.empty((0, self.arch.projection_dim), device=self.device)
        return outs[0] if len(outs) == 1 else torch.cat(outs)

    # ------------------------------------------------------------------------------------------ scores
    def score_pairs(self, images, captions) -> torch.Tensor:
        """Image i against caption i: fp32 [n] on the device = HF `logits_per_image` of each pair alone (what the reference scores)."""
        img = self.get_image_features(images)
        txt = self.get_text_features(captions)
        if img.shape[0] != txt.shape[0]:
            raise ValueError(f"{img.shape[0]} images against {txt.shape[0]} captions")
        if img.shape[0] == 0:
            return torch.empty((0,), device=self.device)
        return self.engine.logits(img, txt, paired=True)

    def logits_per_image(self, images, captions) -> torch.Tensor:
        """fp32 [n_images, n_captions] on the device (HF's `logits_per_image`)."""
        return self.engine.logits(self.get_image_features(images), self.get_text_features(captions), paired=False)
