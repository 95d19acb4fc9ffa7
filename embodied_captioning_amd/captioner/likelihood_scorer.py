"""The captioner's own likelihood as an image-caption scorer: the mean token log-prob of a GIVEN caption under BLIP / BLIP-2, teacher-forced
(`BLIP.score_captions` -> `CaptionerEngine.score`).  It has the surface the pseudo-caption scorers share (`arch`, `device`,
`score_pairs(images, captions)`, `close()` - captioner/clip_scorer.py, captioner/blip2_itm_scorer.py), so it needs no second model to
select a pseudo-caption, plus `score_matrix`: every caption against every image with ONE image-side pass per image.

BLIP and, with family="blip2", BLIP-2; CoCa is refused by name (its wrapper's `score_captions`)."""
from __future__ import annotations

from typing import List, Sequence

import logging

import torch

logger = logging.getLogger(__name__)


class CaptionLikelihoodScorer:
    def __init__(self, name: str = "Salesforce/blip-image-captioning-base", device: str = "cuda:0", dtype: str = "f32s", batch_size: int = 32,
                 max_length: int = 32, candidates: int = 8, model=None, family: str = "blip"):
        """name: what the BLIP wrapper's `model_name` takes (a checkpoint directory, a cached hub id, `procedural[-tiny]:<seed>`).
        max_length: the longest caption scored, in tokens with BOS and [SEP] (at most 32); candidates: captions per image one pass is
        sized for (the arena reserves batch_size x candidates x (max_length - 1) decoder rows, capped at 4096).
        model: an existing BLIP wrapper to score with instead (its engine's capacities then hold)."""
        if model is None and family == "blip2":
            # BLIP-2: the caption pass lives in the prompt pass's buffers (batch_size x 33 rows); max_new_tokens = the tokens behind BOS
            from .models.blip2.blip2 import BLIP2
            from .utils.utils import Configuration
            cfg = Configuration(arch_name="blip2", model_name=name, checkpoint_name=None, height=None, width=None, dtype=dtype,
                                batch_size=int(batch_size), device=device, max_new_tokens=int(max_length) - 1, num_beams=1)
            model = BLIP2(cfg.captioner)
            self._own = True
        elif model is None:
            if family != "blip":
                raise ValueError(f"CaptionLikelihoodScorer: family {family!r} is not scored (blip, blip2)")
            from .models.blip.blip import BLIP
            from .utils.utils import Configuration
            rows = min(int(batch_size) * max(int(candidates), 1) * (int(max_length) - 1), 4096)
            cfg = Configuration(arch_name="blip", model_name=name, checkpoint_name=None, height=None, width=None, dtype=dtype,
                                batch_size=int(batch_size), device=device, max_length=int(max_length), num_beams=min(max(int(candidates), 1), 8),
                                max_score_rows=max(rows, int(max_length) - 1))
            model = BLIP(cfg.captioner)
            # num_beams above only sizes the arena (batch_size x candidates caption rows per pass): this wrapper still generates greedily
            model.num_beams = 1
            self._own = True
        else:
            if not hasattr(model, "score_captions"):
                raise ValueError(f"CaptionLikelihoodScorer: {type(model).__name__} does not score given captions (BLIP, BLIP-2)")
            self._own = False
        self.model = model
        self.arch = model.arch
        self.device = model.device

    def close(self) -> None:
        if self._own and getattr(self.model, "engine", None) is not None:
            self.model.engine.close()

    @torch.no_grad()
    def score_pairs(self, images, captions) -> torch.Tensor:
        """Pair i = (image i, caption i) -> float64 [n]: the mean log-prob of the caption's tokens (its [SEP] included)."""
        return self.model.score_captions(images, list(captions))["logprob_mean"]

    @torch.no_grad()
    def score_matrix(self, images, captions: Sequence) -> torch.Tensor:
        """Every caption against every image -> float64 [n_images, n_captions] of mean token log-probs.  Each image is encoded
        once; a caption that occurs several times is scored once per image and its column copied.  A caption longer than the
        engine scores (`engine.score_limit` tokens, BOS and [SEP] included) is not scored: its column is -inf, so it ranks last, and
        a warning names it - one long caption does not end a whole selection run.  `images` may be the model's image state
        (`model.image_state(crops)`, a uint8 [n, image_state_bytes] tensor): the image side then does not run at all."""
        captions = list(captions)
        key = [c if isinstance(c, str) else tuple(int(i) for i in c) for c in captions]
        limit = int(self.model.engine.score_limit)
        distinct: List = []
        col = {}
        for k, c in zip(key, captions):
            if k in col:
                continue
            if len(self.model.caption_ids(c)) > limit:
                logger.warning("caption %r is longer than the %d tokens scored: left out (score -inf)", c, limit)
                col[k] = -1
                continue
            col[k] = len(distinct)
            distinct.append(c)
        n = int(images.shape[0]) if isinstance(images, torch.Tensor) else len(images)
        res = torch.full((n, len(captions)), float("-inf"), dtype=torch.float64)
        if n == 0 or not distinct:
            return res
        out = self.model.score_captions(images, [list(distinct) for _ in range(n)])
        m = out["logprob_mean"].reshape(n, out["captions_per_image"])[:, : len(distinct)]
        for j, k in enumerate(key):
            if col[k] >= 0:
                res[:, j] = m[:, col[k]]
        return res
