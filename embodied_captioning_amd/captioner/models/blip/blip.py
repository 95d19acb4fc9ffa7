"""BLIP captioner wrapper with the reference's wrapper shape (``captioner/models/blip2/blip2.py:16-29``,
``captioner/models/coca/coca.py:19-33``): ``BLIP(cfg)`` with ``cfg.model_name`` / ``cfg.checkpoint_name``;
``forward(PIL.Image) -> {"text": str, "logits": tuple of per-step fp32 [n_rows, vocab]}`` also kept in ``self.outputs``.

All arithmetic runs in libcaptioner_hip.so (``CaptionerEngine``); this file only resolves the checkpoint, resizes /
uploads frames and detokenises.

model_name forms:
  * a local HF directory or a hub id present in the offline HF cache (``config.json`` + ``model.safetensors`` /
    ``pytorch_model.bin`` + tokenizer files) - e.g. ``Salesforce/blip-image-captioning-base``;
  * ``procedural:<seed>[:<eos_boost>]`` - seeded random weights of BLIP-base shape at 224x224 (what tests/bench use:
    no checkpoint exists offline); ``procedural-tiny:<seed>`` for the fixture-sized architecture.
checkpoint_name (optional): a ``torch.save({'model': state_dict})`` / state-dict / safetensors file that overrides the
weights (reference: ``utils/predictor_utils.py:182-185``).
"""
from __future__ import annotations

import logging
from typing import List, Sequence

import numpy as np
import torch

from ...captioning_predictor import CaptioningPredictor
from ....config import BlipArch
from ....engine import CaptionerEngine, images_or_state
from ....weights import (load_hf_blip_checkpoint, load_state_dict_file, procedural_blip_state_dict, resolve_hf_dir,
                         BLIP_TIED)

logger = logging.getLogger(__name__)


def resolve_prompt(prompt, prompt_ids, tokenizer, arch):
    """The wrapper's two prompt keys -> token ids for `CaptionerEngine.generate(prompt_ids=)`, or None when neither is given.
    prompt (str): tokenized with the checkpoint's tokenizer as HF's BlipProcessor does (`[CLS] words [SEP]`), then what HF
    `BlipForConditionalGeneration.generate` does to it (modeling_blip.py:858-932): BOS replaces [CLS], the trailing [SEP] is dropped.
    prompt_ids (list of ints [P], or rows [N, P]): taken as they are - for directories without a tokenizer and the procedural
    models; column 0 must be BOS (the engine checks).  Giving both, or a string without a tokenizer, raises."""
    if prompt is not None and prompt_ids is not None:
        raise ValueError("captioner.prompt and captioner.prompt_ids are both given: give the prompt as a string OR as token ids")
    if prompt is not None:
        if not isinstance(prompt, str):
            raise ValueError(f"captioner.prompt must be a string, got {type(prompt).__name__} (token ids go to captioner.prompt_ids)")
        if tokenizer is None:
            raise ValueError("captioner.prompt is a string but this model has no tokenizer (a procedural model, or a checkpoint "
                             "directory without tokenizer files): give captioner.prompt_ids instead")
        ids = list(tokenizer(prompt, add_special_tokens=True)["input_ids"])
        if len(ids) < 3:
            raise ValueError(f"captioner.prompt {prompt!r} tokenizes to no word: a prompt needs at least one token")
        return [int(arch.bos)] + [int(i) for i in ids[1:-1]]
    if prompt_ids is None:
        return None
    t = torch.as_tensor(prompt_ids)
    return t.tolist()


class BLIP(CaptioningPredictor):
    def __init__(self, cfg=None):
        super().__init__(cfg)
        name = cfg.model_name or "Salesforce/blip-image-captioning-base"
        self.num_beams = int(getattr(cfg, "num_beams", 1) or 1)
        self.length_penalty = self._length_penalty(cfg)
        self.max_length = int(getattr(cfg, "max_length", 20) or 20)
        self.batch_size = int(getattr(cfg, "batch_size", 8) or 8)
        # default arithmetic: split-fp16 GEMMs ("f32s") - token-identical to the reference's fp32 CPU path; "bf16" is ~2x
        # faster and leaves the reference's token path at near-ties
        dtype = getattr(cfg, "dtype", None) or "f32s"
        self._device = torch.device(getattr(cfg, "device", "cuda:0") or "cuda:0")
        self.tokenizer = None
        if name.startswith("procedural"):
            parts = name.split(":")
            seed = int(parts[1]) if len(parts) > 1 else 0
            boost = float(parts[2]) if len(parts) > 2 else 0.0
            self.arch = BlipArch.tiny() if parts[0] == "procedural-tiny" else BlipArch()
            sd = procedural_blip_state_dict(self.arch, seed, eos_boost=boost)
        else:
            model_dir = resolve_hf_dir(name)
            if model_dir is None:
                raise RuntimeError(f"Pretrained BLIP checkpoint '{name}' not found locally (offline); pass a directory "
                                   f"with config.json + model.safetensors, or 'procedural:<seed>'")
            self.arch, sd = load_hf_blip_checkpoint(model_dir)
            try:
                from transformers import AutoTokenizer
                self.tokenizer = AutoTokenizer.from_pretrained(model_dir)
            except Exception as e:  # noqa: BLE001
                logger.warning("no tokenizer under %s (%s): captions are returned as space-separated token ids", model_dir, e)
        # captioner.prompt (string) / captioner.prompt_ids (token ids): every caption starts with it (HF's conditional captioning)
        self.prompt_ids = resolve_prompt(getattr(cfg, "prompt", None), getattr(cfg, "prompt_ids", None), self.tokenizer, self.arch)
        if self.prompt_ids is not None and self.prompt_ids and isinstance(self.prompt_ids[0], (list, tuple)):
            if len(self.prompt_ids) != 1:
                raise ValueError(f"captioner.prompt_ids has {len(self.prompt_ids)} rows: the configured prompt is ONE prompt for every "
                                 f"caption ([P] or [1, P]); one prompt per image is a per-call argument (generate_batch(prompt_ids=[N, P]))")
            self.prompt_ids = list(self.prompt_ids[0])
        # captioner.max_prompt: prompt capacity of the arena (a full batch prefills in one pass up to this many prompt tokens);
        # default = the configured prompt's length, 0 without one (prompts given per call then prefill in chunks of captions)
        mp = getattr(cfg, "max_prompt", None)
        self.max_prompt = int(mp) if mp is not None else (len(self._prompt_row(self.prompt_ids)) if self.prompt_ids is not None else 0)
        if self.prompt_ids is not None:
            from ....engine import prompt_token_limit, validate_prompt_ids
            validate_prompt_ids(self._prompt_row(self.prompt_ids), self.arch, 1, self.max_length, self.num_beams, None,
                                prompt_token_limit(self.batch_size, self.num_beams, self.max_prompt))
        # captioner.bad_words_ids / captioner.bad_words: HF generate(bad_words_ids=) for every caption (engine.set_bad_words);
        # validated here, before an engine exists
        from ...bad_words import resolve_bad_words
        self.bad_words_ids = resolve_bad_words(cfg, self.tokenizer, self.arch)
        # captioner.repetition_penalty / captioner.no_repeat_ngram_size: HF generate's two repetition controls for every caption
        # (engine.set_repeat_controls); validated here, before an engine exists
        from ...repeat_controls import resolve_repeat_controls
        self.repetition_penalty, self.no_repeat_ngram_size = resolve_repeat_controls(cfg, self.arch, self.max_length)
        # captioner.do_sample / temperature / top_k / top_p / sample_seed / num_return_sequences: HF generate(do_sample=True, ...) for
        # every caption (engine.set_sampling); validated here, before an engine exists
        from ...sampling import resolve_sampling
        (self.do_sample, self.temperature, self.top_k, self.top_p, self.sample_seed,
         self.num_return_sequences) = resolve_sampling(cfg, self.arch, self.batch_size, self.num_beams, "BLIP(cfg)")
        if getattr(cfg, "checkpoint_name", None):
            over = load_state_dict_file(cfg.checkpoint_name)
            for dst, src in BLIP_TIED.items():
                if dst not in over and src in over:
                    over[dst] = over[src]
            sd.update(over)
            logger.info("Captioner model checkpoint loaded successfully from %s", cfg.checkpoint_name)
        self.engine = CaptionerEngine(self.arch, dtype=dtype, max_batch=self.batch_size, max_beams=self.num_beams,
                                      max_len=self.max_length, device=self._device,
                                      cross_cache=self._cross_cache_for(cfg, sd, dtype), max_prompt=self.max_prompt,
                                      max_score_rows=int(getattr(cfg, "max_score_rows", None) or 0))
        # HF generate stops once every caption has its EOS; look every few steps (cfg early_exit_poll, 0 = never)
        poll = getattr(cfg, "early_exit_poll", None)
        poll = 4 if poll is None else int(poll)
        self.engine.set_early_exit(poll)
        self.engine.load_state_dict(sd)
        self.strict_range = bool(getattr(cfg, "strict_range", False))
        self.device_resize = getattr(cfg, "device_resize", None) is not False
        # cfg.streams > 1: micro-batches of one generate_batch call rotate over that many engines / HIP streams and overlap
        # (engine.EnginePool; same captions; one arena per engine, ONE copy of the weights: the pool's engines attach to
        # this engine's weight store)
        self.pool = None
        n_streams = int(getattr(cfg, "streams", 1) or 1)
        # cfg.coalesce_rows (with streams > 1): dynamic batching - the pool merges consecutive micro-batches of one
        # generate_batch call into passes of at most that many rows (EnginePool.generate_many(coalesce_rows=); a frame decodes
        # to the same bits alone, in its micro-batch and in a merged pass, so the captions are those of the unmerged call and
        # the decode chain's per-launch costs are paid once per pass).  None = on: four micro-batches, at most 1024 rows (the
        # arenas of the pool's engines are sized for it); 0 = every micro-batch its own pass.
        cr = getattr(cfg, "coalesce_rows", None)
        self.coalesce_rows = 0
        if n_streams > 1:
            self.coalesce_rows = min(4 * self.batch_size, 1024) if cr is None else max(0, int(cr))
            if self.coalesce_rows <= self.batch_size:
                self.coalesce_rows = 0
            from ....engine import EnginePool
            self.pool = EnginePool(self.arch, n=n_streams, device=self._device, dtype=dtype,
                                   max_batch=max(self.batch_size, self.coalesce_rows),
                                   max_beams=getattr(self, "num_beams", 1), max_len=self.engine.max_len, weights_of=self.engine,
                                   cross_cache=self.engine.cross_cache, max_prompt=self.max_prompt)
            self.pool.set_early_exit(poll)
        elif cr:
            logger.warning("captioner.coalesce_rows is the engine pool's dynamic batching: it needs captioner.streams > 1 - ignored")
        if self.bad_words_ids:
            self.engine.set_bad_words(self.bad_words_ids)
            if self.pool is not None:
                self.pool.set_bad_words(self.bad_words_ids)
        if self.repetition_penalty != 1.0 or self.no_repeat_ngram_size:
            self.engine.set_repeat_controls(self.repetition_penalty, self.no_repeat_ngram_size)
            if self.pool is not None:
                self.pool.set_repeat_controls(self.repetition_penalty, self.no_repeat_ngram_size)
        if self.do_sample:
            self.engine.set_sampling(True, self.temperature, self.top_k, self.top_p, self.sample_seed)
            if self.pool is not None:
                self.pool.set_sampling(True, self.temperature, self.top_k, self.top_p, self.sample_seed)

    @staticmethod
    def _length_penalty(cfg) -> float:
        """captioner.length_penalty: the beam search's (HF `generate(length_penalty=)`; absent = 1.0, the greedy loop does not read it)."""
        lp = getattr(cfg, "length_penalty", None)
        return 1.0 if lp is None else float(lp)

    # nn.Module surface the callers use; weights live in the engine, so .to() only re-targets host-side tensors
    @property
    def device(self):
        return self._device

    @property
    def direct_resize_size(self) -> int:
        """Side of the square the processor resizes every image to, with no aspect handling (HF BlipImageProcessor): callers
        that hold uint8 frames may resize crops on the device (preprocess.crop_resize_u8) and pass uint8 [n, S, S, 3]."""
        return self.arch.image_size

    def to(self, *args, **kwargs):
        return self

    # ------------------------------------------------------------------------------------------ preprocessing
    def preprocess(self, images) -> torch.Tensor:
        """PIL image(s) / uint8 [B,H,W,3] / float [B,3,S,S] -> what the engine takes.  Resize = bicubic to the model's
        square input (HF `BlipImageProcessor`: HF:models/blip/image_processing_pil_blip.py:22-31); rescale and
        OPENAI-CLIP normalisation are fused into the patch-gather kernel for uint8 input."""
        S = self.arch.image_size
        if isinstance(images, torch.Tensor):
            t = images
            if t.dtype == torch.uint8 and t.dim() == 2:        # an image state (`image_state`): the engine takes it as it is
                return t
            if t.dtype == torch.uint8:
                if t.dim() == 3:
                    t = t[None]
                if t.shape[1] != S or t.shape[2] != S:         # Pillow's bicubic, bit-exact, on the device
                    from ....preprocess import crop_resize_u8
                    H, W = int(t.shape[1]), int(t.shape[2])
                    t = torch.cat([crop_resize_u8(f, [(0, 0, W, H)], S, device=self._device) for f in t])
                return t
            return t if t.dim() == 4 else t[None]
        from PIL import Image
        if isinstance(images, Image.Image):
            images = [images]
        if getattr(self, "device_resize", True):
            # Pillow's bicubic resize on the device, bit-exact (csrc/preprocess.hip; tests/test_preprocess_gpu.py): one small upload and
            # two launches per image - 256 crops of 40-400 px: 26 ms against 130 ms of host PIL on one core (tools/pil_list_bench.py)
            from ....preprocess import resize_u8_list
            return resize_u8_list([np.asarray(im.convert("RGB")) for im in images], S, device=self._device)
        frames = [np.asarray(im.convert("RGB").resize((S, S), resample=Image.BICUBIC)) for im in images]
        return torch.from_numpy(np.stack(frames))

    @staticmethod
    def _prompt_row(ids):
        """First row of a prompt given as [P] or [N, P] (what the configuration-time checks look at)."""
        return ids[0] if ids and isinstance(ids[0], (list, tuple)) else ids

    def _call_prompt(self, prompt, prompt_ids, n_rows: int):
        """Prompt of one call: the call's own `prompt` / `prompt_ids` when given, else the configured one -> None, or a function
        (row0, rows) -> the ids of those rows ([P] shared, or the rows' slice of [n_rows, P])."""
        ids = resolve_prompt(prompt, prompt_ids, self.tokenizer, self.arch) if (prompt is not None or prompt_ids is not None) \
            else getattr(self, "prompt_ids", None)
        if ids is None:
            return None
        if ids and isinstance(ids[0], (list, tuple)) and len(ids) > 1:
            if len(ids) != n_rows:
                raise ValueError(f"prompt_ids has {len(ids)} rows for {n_rows} images: give one prompt or one per image")
            return lambda r0, n: ids[r0:r0 + n]
        return lambda r0, n: ids

    def decode(self, ids: Sequence[int]) -> str:
        ids = [int(i) for i in ids]
        if self.tokenizer is not None:
            return self.tokenizer.decode(ids, skip_special_tokens=True).strip()
        a = self.arch
        return " ".join(str(i) for i in ids if i not in (a.bos, a.eos, a.pad))

    # ------------------------------------------------------------------------------------------ forward
    @torch.no_grad()
    def image_state(self, images) -> torch.Tensor:
        """The image side alone, once: images as `generate_batch` takes them (the same preprocessing) -> uint8 [N, image_state_bytes]
        on the device (`CaptionerEngine.image_state`).  `generate_batch(image_state=...)` and `score_captions(image_state=...)`
        decode from it - or from any selection of its rows - without running the image side again, to the bits of the calls on the
        images.  It belongs to this model's weights and configuration."""
        return self.engine.image_state(self.preprocess(images).to(self._device))

    @torch.no_grad()
    def generate_batch(self, images=None, output_logits: bool = False, output_perplexity: bool = False,
                       output_vocab_maxprob: bool = False, prompt=None, prompt_ids=None, image_state=None,
                       num_return_sequences=None) -> dict:
        """num_return_sequences = n (with captioner.do_sample; default = captioner.num_return_sequences): n sampled captions per image
        from ONE image pass - texts / sequences hold N * n entries, image-major (HF's order); the images go in chunks of
        batch_size // n so that every call's rows fit the engine.
        image_state: the tensor `image_state(images)` returned (or rows of it), in place of images: the image side does not run.
        prompt (string) / prompt_ids (token ids [P], or [N, P] one row per image): the text every caption starts with, for this
        call; without them the configured captioner.prompt / captioner.prompt_ids (if any).  Texts and sequences include the prompt,
        per-step outputs cover the generated steps.
        Batched extension: any number of frames -> {"texts": [str], "sequences": int32 [N, L], "lengths", "scores"}.
        output_perplexity (greedy): adds "perplexities" float64 [N] - what `forward` + `compute_perplexity()` give one crop at a
        time - and "token_logprobs" fp32 [N, steps] / "scored_steps" int32 [N] they are computed from (engine.generate,
        output_logprobs); the pool, its dynamic batching and the preprocessing overlap work as without it.
        output_vocab_maxprob (greedy): adds "vocab_maxprob" fp32 [N, vocab] ON THE DEVICE (engine.generate, output_vocab_maxprob -
        the input of `engine.fuse_vocab_groups`) with "token_logprobs" / "scored_steps" on the host; wired as output_perplexity."""
        texts: List[str] = []
        kw = {"output_logprobs": True} if output_perplexity else {}
        if output_vocab_maxprob:
            kw["output_vocab_maxprob"] = True
        kw["length_penalty"] = self.length_penalty
        seqs, lens, scores, logits = [], [], [], []
        pool = getattr(self, "pool", None)
        images = images_or_state(images, image_state, "generate_batch")
        n_images = int(images.shape[0]) if isinstance(images, torch.Tensor) and (images.dim() == 4 or image_state is not None) else \
            len(images) if isinstance(images, (list, tuple)) else 1
        pk = self._call_prompt(prompt, prompt_ids, n_images)
        bs = self.batch_size
        nret = int(num_return_sequences if num_return_sequences is not None else getattr(self, "num_return_sequences", 1) or 1)
        if nret < 1 or (nret > 1 and not getattr(self, "do_sample", False)):
            raise ValueError(f"generate_batch: num_return_sequences = {nret} needs captioner.do_sample (and a count >= 1): the arg-max "
                             f"loop returns one caption per image")
        if nret > bs:
            raise ValueError(f"generate_batch: num_return_sequences = {nret} exceeds batch_size = {bs}: one image's captions are rows of one call")
        if nret > 1:
            pool, bs = None, bs // nret          # images per call; the engine expands every image's state to nret decode rows
            kw["num_return_sequences"] = nret

        def pkw(row0, n_rows):      # prompt_ids of the micro-batches that cover rows row0 .. row0 + n_rows - 1 (generate_many's list form)
            return {} if pk is None else {"prompt_ids": [pk(i, min(bs, row0 + n_rows - i)) for i in range(row0, row0 + n_rows, bs)]}

        # a long list of PIL crops on a pool: in rounds of one pass per engine, the next round's crops are preprocessed (host
        # `Image.convert` + pack, upload, device resize) by a helper thread while the current round generates
        rnd = len(pool) * max(self.batch_size, self.coalesce_rows) if pool is not None else 0
        if (pool is not None and not output_logits and not isinstance(images, torch.Tensor) and isinstance(images, (list, tuple))
                and len(images) > rnd):
            from concurrent.futures import ThreadPoolExecutor
            groups = [images[i:i + rnd] for i in range(0, len(images), rnd)]
            outs = []
            with ThreadPoolExecutor(max_workers=1) as ex:
                nxt = ex.submit(self.preprocess, groups[0])
                for g in range(len(groups)):
                    px = nxt.result()
                    if g + 1 < len(groups):
                        nxt = ex.submit(self.preprocess, groups[g + 1])
                    chunks = [px[i:i + self.batch_size].to(self._device) for i in range(0, px.shape[0], self.batch_size)]
                    outs += self.pool.generate_many(chunks, threads=True, coalesce_rows=self.coalesce_rows, num_beams=self.num_beams,
                                                    max_length=self.max_length, **kw, **pkw(g * rnd, int(px.shape[0])))
        else:
            px = self.preprocess(images)
            chunks = [px[i:i + bs].to(self._device) for i in range(0, px.shape[0], bs)]
            if pool is not None and len(chunks) > 1 and not output_logits:
                outs = self.pool.generate_many(chunks, threads=True, coalesce_rows=self.coalesce_rows, num_beams=self.num_beams,
                                               max_length=self.max_length, **kw, **pkw(0, int(px.shape[0])))
            else:
                outs = [self.engine.generate(c, num_beams=self.num_beams, max_length=self.max_length, output_logits=output_logits,
                                             prompt_ids=None if pk is None else pk(i * bs, int(c.shape[0])), **kw)
                        for i, c in enumerate(chunks)]
        for out in outs:
            seqs.append(out["sequences"]); lens.append(out["lengths"])
            if "sequences_scores" in out:
                scores.append(out["sequences_scores"])
            if output_logits:
                logits.append(out["logits"])
        seq = torch.cat(seqs).cpu()
        ln = torch.cat(lens).cpu()
        self._range_tick()
        for r, n in zip(seq.tolist(), ln.tolist()):
            texts.append(self.decode(r[:n]))
        res = {"texts": texts, "sequences": seq, "lengths": ln}
        if scores:
            res["scores"] = torch.cat(scores).cpu()
        if output_logits:
            res["logits"] = logits
        if output_perplexity:
            from ....engine import perplexity_from_logprobs
            res["token_logprobs"] = torch.cat([o["token_logprobs"] for o in outs]).cpu()
            res["scored_steps"] = torch.cat([o["scored_steps"] for o in outs]).cpu()
            res["perplexities"] = perplexity_from_logprobs(res["token_logprobs"], res["scored_steps"])
        if output_vocab_maxprob:
            res["vocab_maxprob"] = torch.cat([o["vocab_maxprob"] for o in outs])
            if not output_perplexity:
                res["token_logprobs"] = torch.cat([o["token_logprobs"] for o in outs]).cpu()
                res["scored_steps"] = torch.cat([o["scored_steps"] for o in outs]).cpu()
        return res

    def caption_ids(self, caption) -> List[int]:
        """One caption as the decoder's tokens for scoring: a string goes through the checkpoint's tokenizer (`[CLS] words [SEP]`)
        with BOS in place of [CLS] and the closing [SEP] kept, so the end of the caption is scored; a list of token ids (models
        without a tokenizer) is taken as it is, BOS put in front when it does not start with it."""
        if isinstance(caption, str):
            if self.tokenizer is None:
                raise ValueError("score_captions: a caption string needs a tokenizer and this model has none (a procedural model, or a "
                                 "checkpoint directory without tokenizer files): give lists of token ids")
            ids = [int(i) for i in self.tokenizer(caption, add_special_tokens=True)["input_ids"]]
            return [int(self.arch.bos)] + ids[1:]
        ids = [int(i) for i in caption]
        return ids if ids and ids[0] == self.arch.bos else [int(self.arch.bos)] + ids

    @torch.no_grad()
    def score_captions(self, images=None, captions=None, image_state=None) -> dict:
        """image_state: the tensor `image_state(images)` returned (or rows of it), in place of images.
        Teacher-forced likelihood of GIVEN captions under this captioner (`CaptionerEngine.score`; HF `model(pixel_values,
        input_ids=...)` reduced to log-probs).  captions: one per image (strings, or token-id lists for models without a tokenizer),
        or a list of candidates per image (a list of lists; images may have different numbers of candidates).
        -> host tensors, caption-major ([image 0's candidates, image 1's, ...], images with fewer candidates padded with absent
        slots): "token_logprobs" fp32 [N, L - 1], "n_tokens" int64 [N] (scored tokens: the caption's without BOS; 0 = absent slot),
        "logprob_sum" / "logprob_mean" / "perplexity" (exp(-mean) of the given tokens) / "top_perplexity" (the reference's max-softmax
        form on the same rows) float64 [N] (nan for absent slots), "top_ids" int32 [N, L - 1], "captions_per_image" int.  Captions
        longer than the engine takes (`engine.score_limit`) are refused; scoring longer than batch_size x num_beams tokens needs
        captioner.max_score_rows."""
        from ....engine import score_summary
        images = images_or_state(images, image_state, "score_captions")
        if captions is None:
            raise ValueError("score_captions: no caption to score")
        captions = list(captions)
        nested = bool(captions) and all(isinstance(c, (list, tuple)) and (len(c) == 0 or isinstance(c[0], (str, list, tuple))) for c in captions)
        groups = [list(c) for c in captions] if nested else [[c] for c in captions]
        px = self.preprocess(images)
        if int(px.shape[0]) != len(groups):
            raise ValueError(f"score_captions: {int(px.shape[0])} images but {len(groups)} captions / candidate lists")
        Cn = max((len(g) for g in groups), default=0)
        if Cn < 1:
            raise ValueError("score_captions: no caption to score")
        rows = [[self.caption_ids(c) for c in g] for g in groups]
        L = max(2, max(len(r) for g in rows for r in g))
        ids = np.full((len(groups) * Cn, L), self.arch.pad, dtype=np.int32)
        lens = np.zeros(len(groups) * Cn, dtype=np.int32)
        for b, g in enumerate(rows):
            for c, r in enumerate(g):
                ids[b * Cn + c, : len(r)] = r
                lens[b * Cn + c] = len(r)
        out = self.engine.score(px.to(self._device), ids, lens, captions_per_image=Cn)
        self._range_tick()
        res = {"token_logprobs": out["token_logprobs"].cpu(), "top_logprobs": out["top_logprobs"].cpu(), "top_ids": out["top_ids"].cpu(),
               "captions_per_image": Cn}
        res.update(score_summary(res["token_logprobs"], res["top_logprobs"], out["scored"]))
        return res

    @torch.no_grad()
    def forward(self, inputs):
        px = self.preprocess(inputs)[:1]
        # the configured prompt, as HF's `generate(pixel_values, input_ids=...)`: the text includes the prompt's words (HF
        # `decode(out[0], skip_special_tokens=True)`), the logits are the generated steps
        pr = None if self.prompt_ids is None else self._prompt_row(self.prompt_ids)
        out = self.engine.generate(px.to(self._device), num_beams=self.num_beams, max_length=self.max_length,
                                   length_penalty=self.length_penalty, output_logits=True, prompt_ids=pr)
        n = int(out["lengths"][0])
        ids = out["sequences"][0, :n].tolist()
        self._range_tick()
        # new objects every call: callers keep references to outputs["logits"] across calls
        # (reference generate_pseudo_caption_from_file.py:152)
        self.outputs = {"text": self.decode(ids),
                        "logits": tuple(out["logits"][t] for t in range(max(n - (len(pr) if pr is not None else 1), 1)))}
        return self.outputs
