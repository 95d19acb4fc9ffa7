"""`Captioner` plugin - mirror of the reference's ``experimenting_env/utils/predictor_utils.py:166-208``: same
constructor signature, `.forward(x) -> str`, `get_captioner(cfg)` dispatch on ``cfg.arch_name``; plus a batched
`caption_batch` for the pseudo-labeler driver."""
from __future__ import annotations

import logging

import torch

from ..captioner.captioning_predictor import _Base
from ..captioner.utils.utils import Configuration
from ..captioner.utils.utils_captioner import select_captioner

logger = logging.getLogger(__name__)


class Captioner(_Base):
    def __init__(self, cfg=None, input_format=None, load_checkpoint=False, checkpoint_path=None, metadata=None,
                 model=None):
        super().__init__()
        if model is None:
            self.model = self.get_captioner(cfg.captioner)
        else:
            self.model = model
        self.model.eval()
        assert self.model is not None, "No model provided"
        logger.info("Captioner model loaded successfully")
        if load_checkpoint and checkpoint_path is not None:
            checkpoint = torch.load(checkpoint_path, map_location="cpu", weights_only=True)
            res = self.model.load_checkpoint_state_dict(checkpoint["model"], strict=False)
            logger.info(f"Captioner model checkpoint loaded successfully from {checkpoint_path} "
                        f"({res['matched']} tensors, {len(res['unknown'])} not stored by this architecture)")

    def get_captioner(self, cfg):
        """Get the captioner model based on the configuration settings (reference :190-202)."""
        extra = {k: getattr(cfg, k) for k in ("num_beams", "max_length", "max_new_tokens", "dtype", "batch_size", "device",
                                              "streams", "early_exit_poll", "image_size", "num_beam_groups", "tokenizer_dir",
                                              "coalesce_rows", "cross_cache", "strict_range", "prompt", "prompt_ids", "max_prompt",
                                              "max_score_rows", "bad_words_ids", "bad_words", "bad_words_mode",
                                              "repetition_penalty", "no_repeat_ngram_size", "do_sample", "temperature", "top_k",
                                              "top_p", "sample_seed", "num_return_sequences")
                 if hasattr(cfg, k)}
        captioner_cfg = Configuration(arch_name=cfg.arch_name, model_name=cfg.model_name,
                                      checkpoint_name=getattr(cfg, "checkpoint_name", None), height=cfg.height,
                                      width=cfg.width, **extra)
        return select_captioner(captioner_cfg.captioner).eval()

    def forward(self, x):
        out = self.model(x)
        caption = out["text"]
        return caption

    def caption_batch(self, images, return_perplexity: bool = False, prompt=None, prompt_ids=None):
        """Batched extension: list of PIL images / uint8 tensor -> list of captions; return_perplexity: -> (captions, float64 [n]
        perplexities), the number the reference gets from `compute_perplexity()` after every one-crop call.
        prompt / prompt_ids (BLIP): the text prompt of this call instead of the configured captioner.prompt / captioner.prompt_ids
        (which every call without them uses - the box driver's included)."""
        kw = {k: v for k, v in (("prompt", prompt), ("prompt_ids", prompt_ids)) if v is not None}
        if return_perplexity:
            out = self.model.generate_batch(images, output_perplexity=True, **kw)
            return out["texts"], out["perplexities"]
        return self.model.generate_batch(images, **kw)["texts"]

    def score_batch(self, crops, captions) -> dict:
        """Likelihood of GIVEN captions under the captioner (BLIP): crops as for `caption_batch`, captions one per crop or a list of
        candidates per crop -> the model's `score_captions` dict (token_logprobs, n_tokens, logprob_sum, logprob_mean, perplexity,
        top_perplexity).  Architectures without it (CoCa, BLIP-2) refuse by name."""
        fn = getattr(self.model, "score_captions", None)
        if fn is None:
            raise ValueError(f"score_batch: {type(self.model).__name__} does not score given captions (built for BLIP)")
        return fn(crops, captions)

    @property
    def direct_resize_size(self):
        """Side of the processor's plain square resize (BLIP / BLIP-2), or None (CoCa: aspect-preserving resize + centre
        crop): lets the box driver crop + resize on the device (pseudolabeler.BatchedBoxCaptioner)."""
        return getattr(self.model, "direct_resize_size", None)

    @property
    def shorter_side_resize_size(self):
        """CoCa: side of the aspect-preserving resize + centre crop (None for the square-resize processors)."""
        return getattr(self.model, "shorter_side_resize_size", None)

    @property
    def crop_device(self):
        return getattr(self.model, "device", "cuda:0")
