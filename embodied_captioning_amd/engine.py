"""Host orchestration over the C ABI: builds a handle, streams checkpoint tensors in, exposes encode / generate on
torch CUDA tensors.  PyTorch here is plumbing only (device buffers, streams); all arithmetic runs in
libcaptioner_hip.so.  Mirrors what the reference's wrappers call on their torch models:
`model.generate(...)` (captioner/models/blip2/blip2.py:26, coca/coca.py:29) and `_encode_image` (coca_model.py:152-155).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import json
import logging
import math
import numbers
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _native as N
from .config import Blip2Arch, Blip2ItmArch, BlipArch, ClipArch, CocaArch, MiniLMArch
from .captioner.bad_words import validate_bad_words_ids  # noqa: F401 - the host check of set_bad_words, public here
from .captioner.repeat_controls import validate_repeat_controls  # noqa: F401 - the host check of set_repeat_controls, public here
from .captioner.sampling import default_sample_keys, keys_tensor, return_sequence_keys, validate_sampling  # noqa: F401 - public here

logger = logging.getLogger(__name__)

OPENAI_CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
OPENAI_CLIP_STD = (0.26862954, 0.26130258, 0.27577711)

# "f32s" = CAP_F32_SPLIT: fp32 values carried into every GEMM as two fp16 halves, three fp16 MFMAs per product (fp32-grade
# products, token-identical to the fp32 reference on the goldens, several times faster than "f32"); BLIP, BLIP-2 and CoCa.
_DTYPES = {"f32": N.CAP_F32, "fp32": N.CAP_F32, "float32": N.CAP_F32, "bf16": N.CAP_BF16, "bfloat16": N.CAP_BF16,
           "f32s": N.CAP_F32_SPLIT, "split": N.CAP_F32_SPLIT, "f32_split": N.CAP_F32_SPLIT}


def _stream_ptr(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def perplexity_from_logprobs(token_logprobs: torch.Tensor, scored_steps: torch.Tensor) -> torch.Tensor:
    """Per-caption perplexity, float64 [B], from `generate(..., output_logprobs=True)`: exp(-sum_{j < scored} lp_j / scored) -
    the reference's `compute_perplexity` (captioning_predictor.py:34-47: exp(-sum_t log max softmax(logits_t) / T)) with the
    per-step term taken on the device.  token_logprobs [B, steps], scored_steps int [B]; entries from `scored` on (zeros after a
    caption's end) do not enter.  Host arithmetic in float64; a caption with no scored step gives nan."""
    lp = torch.as_tensor(token_logprobs).detach().cpu().to(torch.float64)
    n = torch.as_tensor(scored_steps).detach().cpu().to(torch.int64)
    if lp.dim() != 2 or n.shape != (lp.shape[0],):
        raise ValueError(f"token_logprobs must be [B, steps] and scored_steps [B], got {tuple(lp.shape)} / {tuple(n.shape)}")
    if lp.shape[0] and (int(n.min()) < 0 or int(n.max()) > lp.shape[1]):
        raise ValueError(f"scored_steps must be within 0..{lp.shape[1]}")
    keep = torch.arange(lp.shape[1])[None, :] < n[:, None]
    total = torch.where(keep, lp, torch.zeros_like(lp)).sum(dim=1)
    return torch.exp(-total / n.to(torch.float64))


def vocab_group_csr(groups: Sequence[Sequence[int]], n_rows: int):
    """Groups of row indices -> the CSR pair the group kernel takes: (group_rows int32 [M], group_off int32 [G + 1]) on the host.
    Members keep the caller's order and need not be contiguous; an empty group is legal; a row may belong to one group only."""
    rows: List[int] = []
    off = [0]
    for g, members in enumerate(groups):
        for r in members:
            r = int(r)
            if not 0 <= r < n_rows:
                raise ValueError(f"groups[{g}]: row {r} is outside the {n_rows} rows of vocab_maxprob")
            rows.append(r)
        off.append(len(rows))
    if len(set(rows)) != len(rows):
        dup = sorted({r for r in rows if rows.count(r) > 1})
        raise ValueError(f"groups: row(s) {dup[:8]} are listed more than once (a row belongs to one group only)")
    return torch.tensor(rows, dtype=torch.int32), torch.tensor(off, dtype=torch.int32)


def fusion_max_tokens(steps: int, th: float, vocab: int) -> int:
    """Capacity per group that the kept tokens cannot exceed: ceil(steps / th), at most the vocabulary (`fuse_vocab_groups`)."""
    if not th > 0:
        return int(vocab)
    return max(1, min(int(vocab), int(math.ceil(steps / th))))


def prompt_token_limit(max_batch: int, max_beams: int = 1, max_prompt: int = 0) -> int:
    """Longest prompt (tokens, BOS included) an engine of that capacity takes: a prompt of P tokens runs P - 1 prefill rows per
    caption through the decoder's pass buffers, which hold max(max_batch * max_beams, max_batch * (max_prompt - 1)) rows; never
    more than the library's CAP_MAX_PROMPT.  With max_prompt >= P a full batch is one pass, else captions go in chunks."""
    rows = max(int(max_batch) * int(max_beams), int(max_batch) * max(int(max_prompt) - 1, 0))
    return min(N.CAP_MAX_PROMPT, rows + 1)


def _arch_family(arch) -> str:
    return "coca" if isinstance(arch, CocaArch) else "blip2" if isinstance(arch, Blip2Arch) else "blip"


def validate_prompt_ids(prompt_ids, arch, batch: int, max_length: int, num_beams: int = 1, num_beam_groups: Optional[int] = None,
                        limit: int = N.CAP_MAX_PROMPT) -> torch.Tensor:
    """The host check of `generate(..., prompt_ids=)`: a list or tensor [P], [1, P] or [batch, P] -> int32 host tensor [rows, P],
    rows 1 (shared) or batch.  Raises, naming the fault, BEFORE anything is uploaded or launched: a prompt for an architecture that
    takes none (CoCa's `text=`, BLIP-2), beam search, an id outside [0, vocab), column 0 not BOS, EOS or pad inside the prompt, P
    outside [2, limit] or not below max_length, a row count that is neither 1 nor the batch.  Needs no GPU."""
    fam = _arch_family(arch)
    if fam == "coca":
        raise ValueError("prompt_ids: a text prompt for a CoCa handle is not built (the reference's `text=`, coca_model.py:207, stays "
                         "refused); prompts are BLIP's")
    if fam == "blip2":
        raise ValueError("prompt_ids: a text prompt for a BLIP-2 handle is not built (HF `Blip2ForConditionalGeneration.generate("
                         "input_ids=)`); prompts are BLIP's")
    if num_beam_groups is not None or int(num_beams) != 1:
        raise ValueError(f"prompt_ids: a prompt is taken by greedy decoding only; num_beams = {num_beams}"
                         + (f", num_beam_groups = {num_beam_groups}" if num_beam_groups is not None else "") + " is beam search")
    t = torch.as_tensor(prompt_ids)
    if t.is_floating_point() or t.dtype == torch.bool or t.is_complex():
        raise ValueError(f"prompt_ids must hold integer token ids, got dtype {t.dtype}")
    t = t.detach().cpu().to(torch.int64)
    if t.dim() == 1:
        t = t[None, :]
    if t.dim() != 2:
        raise ValueError(f"prompt_ids must be [P], [1, P] or [batch, P], got shape {tuple(t.shape)}")
    rows, P = int(t.shape[0]), int(t.shape[1])
    if rows != 1 and rows != int(batch):
        raise ValueError(f"prompt_ids has {rows} rows: the row count must be 1 (one prompt for every caption) or the batch size {batch}")
    if P < 2:
        raise ValueError(f"prompt_ids has {P} token(s) per row: a prompt is BOS plus at least one token (P >= 2)")
    if P > int(limit):
        raise ValueError(f"prompt_ids has {P} tokens per row: too long, the limit is {limit} tokens (BOS included) for this engine")
    if P >= int(max_length):
        raise ValueError(f"prompt_ids has {P} tokens per row but max_length is {max_length}: max_length counts the prompt and must "
                         f"leave room for a generated token (P < max_length)")
    lo, hi = int(t.min()), int(t.max())
    if lo < 0 or hi >= arch.vocab:
        raise ValueError(f"prompt_ids holds token id {lo if lo < 0 else hi}, out of range [0, {arch.vocab}) of the vocabulary")
    if bool((t[:, 0] != arch.bos).any()):
        raise ValueError(f"prompt_ids column 0 must be BOS ({arch.bos}) in every row, got {sorted(set(t[:, 0].tolist()))[:4]}")
    for name, tid in (("EOS", arch.eos), ("pad", arch.pad)):
        if bool((t[:, 1:] == tid).any()):
            raise ValueError(f"prompt_ids holds the {name} token ({tid}) inside the prompt: a prompt is an open caption prefix")
    return t.to(torch.int32).contiguous()


def score_summary(token_logprobs, top_logprobs, scored) -> Dict[str, torch.Tensor]:
    """Per-caption numbers from `score`'s outputs, float64 on the host: n_tokens int64 [N] (= scored), logprob_sum, logprob_mean,
    perplexity = exp(-mean) of the GIVEN tokens, and top_perplexity = the reference's `compute_perplexity` on the teacher-forced
    rows (exp(-mean log max softmax), `perplexity_from_logprobs`).  A caption with no scored token (an absent slot) gives nan."""
    lp = torch.as_tensor(token_logprobs).detach().cpu().to(torch.float64)
    n = torch.as_tensor(scored).detach().cpu().to(torch.int64)
    if lp.dim() != 2 or n.shape != (lp.shape[0],):
        raise ValueError(f"token_logprobs must be [N, L - 1] and scored [N], got {tuple(lp.shape)} / {tuple(n.shape)}")
    keep = torch.arange(lp.shape[1])[None, :] < n[:, None]
    total = torch.where(keep, lp, torch.zeros_like(lp)).sum(dim=1)
    mean = total / n.to(torch.float64)
    return {"n_tokens": n, "logprob_sum": total, "logprob_mean": mean, "perplexity": torch.exp(-mean),
            "top_perplexity": perplexity_from_logprobs(top_logprobs, n)}


SCORE_MAX_TOKENS = 32     # tokens per caption (BOS included) cap_score_captions takes: one prefill pass covers 31 positions


def validate_score_ids(ids, lens, arch, n_images: int, captions_per_image: int = 1, limit: int = SCORE_MAX_TOKENS):
    """The host check of `score(pixels, ids, lens)`: -> (ids int32 [N, L], lens int32 [N]) host tensors, N = n_images *
    captions_per_image.  Raises ValueError, naming the fault, BEFORE anything is uploaded or launched: an architecture that is not
    scored (CoCa), captions_per_image < 1, ids not an integer [N, L] array or lens not an integer [N] array, L outside
    [2, limit], lens[n] outside [2, L] (0 = an absent slot, only with captions_per_image > 1), an id outside [0, vocab), column 0 of
    a present caption not BOS, pad or EOS INSIDE a caption (EOS as its last token is allowed).  Columns from lens[n] on are padding:
    only the range of their ids is checked.  Needs no GPU."""
    fam = _arch_family(arch)
    if fam == "coca":
        raise ValueError("score: scoring given captions is not built for CoCa; it is BLIP's and BLIP-2's")
    C_ = int(captions_per_image)
    if C_ < 1:
        raise ValueError(f"score: captions_per_image = {captions_per_image} must be at least 1")
    t, ln = torch.as_tensor(ids), torch.as_tensor(lens)
    for name, x in (("ids", t), ("lens", ln)):
        if x.is_floating_point() or x.dtype == torch.bool or x.is_complex():
            raise ValueError(f"score: {name} must hold integers, got dtype {x.dtype}")
    t, ln = t.detach().cpu().to(torch.int64), ln.detach().cpu().to(torch.int64)
    n = int(n_images) * C_
    if t.dim() != 2 or int(t.shape[0]) != n:
        raise ValueError(f"score: ids must be [N, L] with N = {n_images} images x {C_} captions = {n}, got shape {tuple(t.shape)}")
    if ln.dim() != 1 or int(ln.shape[0]) != n:
        raise ValueError(f"score: lens must be [N] with N = {n}, got shape {tuple(ln.shape)}")
    if n < 1:
        raise ValueError(f"score: nothing to score ({n_images} images x {C_} captions)")
    L = int(t.shape[1])
    if L < 2:
        raise ValueError(f"score: ids has {L} column(s): a caption is BOS plus at least one scored token (L >= 2)")
    if L > int(limit):
        raise ValueError(f"score: ids has {L} columns: too long, the limit is {limit} tokens (BOS included) for this engine")
    absent = ln == 0
    if bool(absent.any()) and C_ == 1:
        raise ValueError(f"score: lens[{int(absent.nonzero()[0])}] = 0 marks an absent slot, which exists only with captions_per_image > 1")
    bad = ~absent & ((ln < 2) | (ln > L))
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        raise ValueError(f"score: lens[{i}] = {int(ln[i])} is outside [2, L = {L}] (BOS plus at least one token; 0 = absent slot)")
    lo, hi = int(t.min()), int(t.max())
    if lo < 0 or hi >= arch.vocab:
        raise ValueError(f"score: ids holds token id {lo if lo < 0 else hi}, out of range [0, {arch.vocab}) of the vocabulary")
    if bool((t[~absent, 0] != arch.bos).any()):
        raise ValueError(f"score: ids column 0 must be BOS ({arch.bos}) in every caption, got {sorted(set(t[~absent, 0].tolist()))[:4]}")
    col = torch.arange(L)[None, :]
    inside = (col >= 1) & (col < (ln[:, None] - 1))          # tokens 1 .. lens - 2: behind BOS, before the last
    last = (col == (ln[:, None] - 1)) & ~absent[:, None]
    if bool((inside & (t == arch.pad)).any() or (last & (t == arch.pad) & (arch.pad != arch.eos)).any()):
        raise ValueError(f"score: ids holds the pad token ({arch.pad}) inside a caption (padding starts at lens[n])")
    if bool((inside & (t == arch.eos)).any()):
        raise ValueError(f"score: ids holds the EOS token ({arch.eos}) inside a caption: EOS is allowed as the last token only")
    return t.to(torch.int32).contiguous(), ln.to(torch.int32).contiguous()


def is_image_state(x) -> bool:
    """What `generate` / `score` read as an image state (`CaptionerEngine.image_state`): a uint8 tensor of two dimensions.  uint8
    frames have four."""
    return isinstance(x, torch.Tensor) and x.dtype == torch.uint8 and x.dim() == 2


def validate_image_state(state: torch.Tensor, image_state_bytes: int) -> None:
    """The host check of a state handed to `generate` / `score`: its row size must be the engine's `image_state_bytes`.  Needs no
    GPU.  A size is all that can be checked: see `CaptionerEngine.image_state`."""
    if not is_image_state(state):
        raise ValueError(f"an image state is a uint8 [B, image_state_bytes] tensor, got {tuple(state.shape)} {state.dtype}")
    if int(state.shape[1]) != int(image_state_bytes):
        raise ValueError(f"image state rows of {int(state.shape[1])} bytes do not fit this engine, whose image_state_bytes is "
                         f"{int(image_state_bytes)}: a state belongs to engines of the same architecture, compute type and "
                         f"cross-cache kind as the one that made it")
    if int(state.shape[0]) < 1:
        raise ValueError("an image state needs at least one row")


def images_or_state(images, image_state, who: str):
    """The wrappers' `images` / `image_state=` pair -> the one that was given (exactly one must be)."""
    if (images is None) == (image_state is None):
        raise ValueError(f"{who}: give images or image_state=, one of the two")
    if image_state is None:
        return images
    if not is_image_state(image_state):
        raise ValueError(f"{who}: image_state is the uint8 [N, image_state_bytes] tensor `image_state(images)` returns")
    return image_state


def _launch(lib, device, entry: str, *args) -> None:
    """One native call on `device` and its current stream: tensors go in as their data pointers (None = NULL), everything else as it
    is; the stream is the entry point's last argument; a non-zero status raises under the entry point's name."""
    with torch.cuda.device(device):
        argv = [C.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else a for a in args]
        N.check(getattr(lib, entry)(*argv, C.c_void_p(_stream_ptr(device))), entry)


def _ids_shape(ids: torch.Tensor, lens: torch.Tensor):
    if ids.dim() != 2 or lens.shape != (ids.shape[0],):
        raise ValueError(f"ids must be [B, L] and lens [B], got {tuple(ids.shape)} / {tuple(lens.shape)}")
    return ids.shape


@contextlib.contextmanager
def _deriving_tensors():
    """Around the preparations of a `load_state_dict` that compute tensors from the checkpoint's own: a key they need and do not find
    is named as the library's error."""
    try:
        yield
    except KeyError as e:
        raise N.CaptionerHipError(f"state dict lacks {e}: this architecture derives tensors from the checkpoint at load "
                                  f"and needs the complete dict (keys with a 'model.' / 'module.' prefix? see "
                                  f"weights.strip_wrapper_prefixes)") from e


def _with_qformer_x0(sd: Dict[str, torch.Tensor], q_eps: float) -> Dict[str, torch.Tensor]:
    """The Q-Former's input = LayerNorm(query_tokens) is a constant of the checkpoint: computed once here (`derived.qformer_x0`)."""
    if "derived.qformer_x0" in sd:
        return sd
    sd = dict(sd)
    q = sd["query_tokens"].float()[0]
    sd["derived.qformer_x0"] = torch.nn.functional.layer_norm(
        q, (q.shape[-1],), sd["qformer.layernorm.weight"].float(), sd["qformer.layernorm.bias"].float(), q_eps)
    return sd


class _Engine:
    """One native handle on one GPU, bound to torch's current stream of `device` at each call: what the captioner and the three
    scorer engines share - creation, lifetime and diagnostics, the weight stream, the checks of frames and of ids / lens, and the
    form of a native call.  A subclass fills its own fields of the CapConfig and adds its forward calls."""

    _NO_GPU = "needs a GPU"

    def __init__(self, arch, dtype: str, max_batch: int, max_len: int, device: str | torch.device):
        if not torch.cuda.is_available():
            raise N.CaptionerHipError(f"{type(self).__name__} {self._NO_GPU}; there is no CPU fallback in the product path")
        self.lib = N.load_library()
        self.arch, self.dtype, self.device = arch, dtype, torch.device(device)
        self.max_batch, self.max_len = max_batch, max_len

    # ------------------------------------------------------------------------------------------ creation
    def _config(self, arch_kind: int, max_beams: int = 1) -> N.CapConfig:
        cfg = N.CapConfig()
        cfg.struct_size = C.sizeof(N.CapConfig)
        cfg.arch = arch_kind
        cfg.compute_dtype = _DTYPES[self.dtype]
        cfg.max_batch, cfg.max_beams, cfg.max_len = self.max_batch, max_beams, self.max_len
        return cfg

    def _vision_tower(self, cfg: N.CapConfig, eps: float) -> None:
        a = self.arch
        cfg.image_size, cfg.patch_size = a.image_size, a.patch_size
        cfg.v_hidden, cfg.v_layers, cfg.v_heads, cfg.v_mlp, cfg.v_eps = a.v_hidden, a.v_layers, a.v_heads, a.v_mlp, eps
        for i in range(3):
            cfg.pix_mean[i] = OPENAI_CLIP_MEAN[i]
            cfg.pix_std[i] = OPENAI_CLIP_STD[i]

    def _text_tower(self, cfg: N.CapConfig, max_pos: int, eps: float, tokens=None) -> None:
        """tokens: (bos, eos, pad) of a tower that has special tokens."""
        a = self.arch
        cfg.t_hidden, cfg.t_layers, cfg.t_heads, cfg.t_ffn = a.t_hidden, a.t_layers, a.t_heads, a.t_ffn
        cfg.vocab, cfg.max_pos, cfg.t_eps = a.vocab, max_pos, eps
        if tokens is not None:
            cfg.bos, cfg.eos, cfg.pad = tokens

    def _qformer(self, cfg: N.CapConfig) -> None:
        a = self.arch
        cfg.q_hidden, cfg.q_layers, cfg.q_heads, cfg.q_ffn = a.q_hidden, a.q_layers, a.q_heads, a.q_ffn
        cfg.q_cross_freq, cfg.num_query_tokens, cfg.q_eps = a.q_cross_freq, a.num_query_tokens, a.q_eps

    def _create(self, cfg: N.CapConfig, share_weights_with: "_Engine | None") -> None:
        self._h = C.c_void_p()
        self.shares_weights = share_weights_with is not None
        with torch.cuda.device(self.device):
            if share_weights_with is not None:
                N.check(self.lib.cap_create_shared(C.byref(cfg), share_weights_with._h, C.byref(self._h)), "cap_create_shared")
            else:
                N.check(self.lib.cap_create(C.byref(cfg), C.byref(self._h)), "cap_create")

    def _call(self, entry: str, *args) -> None:
        """`_launch` of an entry point that takes this handle first."""
        _launch(self.lib, self.device, entry, self._h, *args)

    # ------------------------------------------------------------------------------------------ lifetime
    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            with torch.cuda.device(self.device):          # cap_destroy synchronises and frees on the CURRENT device
                self.lib.cap_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    @property
    def device_bytes(self) -> int:
        return int(self.lib.cap_device_bytes(self._h))

    def saturations(self, reset: bool = False) -> int:
        """Split mode ("f32s") only has a finite range: values beyond +-65000 at a GEMM input are clamped - and counted.
        Returns the count on this engine's GPU since the last reset (0 = every value was inside the fp32-grade envelope);
        synchronises the device.  Weights outside the mode's range never get this far: load_state_dict raises."""
        with torch.cuda.device(self.device):
            n = int(self.lib.cap_g8_saturations(int(reset)))
        if n < 0:
            raise N.CaptionerHipError(f"cap_g8_saturations: {N.last_error()}")
        return n

    # ------------------------------------------------------------------------------------------ weights
    def _stream_weights(self, sd: Dict[str, torch.Tensor], strict: bool) -> Dict[str, object]:
        """What every `load_state_dict` ends in, once its dict is prepared: each tensor through cap_load_weight, then
        cap_finalize_weights; the rules and the report are those of `CaptionerEngine.load_state_dict`."""
        matched, unknown = 0, []
        with torch.cuda.device(self.device):
            s = _stream_ptr(self.device)
            for name, t in sd.items():
                t = t.detach()
                if t.dtype != torch.float32:
                    t = t.float()
                t = t.contiguous()
                shape = (C.c_int64 * max(t.dim(), 1))(*(t.shape if t.dim() else (1,)))
                rc = self.lib.cap_load_weight(self._h, name.encode(), C.c_void_p(t.data_ptr()), int(t.is_cuda),
                                              max(t.dim(), 1), shape, C.c_void_p(s))
                if rc < 0:
                    raise N.CaptionerHipError(f"cap_load_weight({name}): {N.last_error()}")
                if rc == 0:
                    matched += 1
                else:
                    unknown.append(name)
            if len(sd) and not matched:
                raise N.CaptionerHipError(f"none of the {len(sd)} tensors is one this architecture stores "
                                          f"(first keys: {list(sd)[:3]}): wrong checkpoint or key prefix")
            missing = self.lib.cap_finalize_weights(self._h)
            if missing and strict:
                raise N.CaptionerHipError(f"checkpoint incomplete: {N.last_error()}")
        return {"matched": matched, "unknown": unknown}

    # ------------------------------------------------------------------------------------------ input checks
    def _pixels(self, pixels: torch.Tensor):
        """Frames, uint8 [B, S, S, 3] or float [B, 3, S, S] -> (contiguous on this device, the library's pixel format)."""
        if pixels.device != self.device:
            pixels = pixels.to(self.device, non_blocking=True)
        a = self.arch
        if pixels.dtype == torch.uint8:
            if pixels.dim() != 4 or pixels.shape[1:] != (a.image_size, a.image_size, 3):
                raise ValueError(f"uint8 frames must be [B,{a.image_size},{a.image_size},3], got {tuple(pixels.shape)}")
            fmt = N.CAP_PIX_U8_NHWC
        else:
            if pixels.dim() != 4 or pixels.shape[1:] != (3, a.image_size, a.image_size):
                raise ValueError(f"float frames must be [B,3,{a.image_size},{a.image_size}], got {tuple(pixels.shape)}")
            pixels = pixels.float()
            fmt = N.CAP_PIX_F32_NCHW
        return pixels.contiguous(), fmt

    def _ids_lens(self, ids: torch.Tensor, lens: torch.Tensor):
        """ids int [B, L], lens int [B] -> (ids, lens as int32 on this device, B, L).  Host tensors are validated here for free; device
        tensors are clamped by the kernels (no host synchronisation per call)."""
        B, L = _ids_shape(ids, lens)
        if not ids.is_cuda and not lens.is_cuda and B and L:
            if int(lens.max()) > L or int(lens.min()) < 1:
                raise ValueError("lens must be within 1..L")
            if int(ids.max()) >= self.arch.vocab or int(ids.min()) < 0:
                raise ValueError("token id outside the vocabulary")
        return ids.to(self.device, torch.int32).contiguous(), lens.to(self.device, torch.int32).contiguous(), B, L

    # ------------------------------------------------------------------------------------------ profiling
    def profile(self, on: bool) -> None:
        N.check(self.lib.cap_profile_enable(self._h, int(on)), "cap_profile_enable")

    def profile_report(self) -> dict:
        buf = C.create_string_buffer(1 << 16)
        N.check(self.lib.cap_profile_report(self._h, buf, len(buf)), "cap_profile_report")
        return json.loads(buf.value.decode())

    # ------------------------------------------------------------------------------------------ arena state (tests only)
    def _fill_arena(self, pattern: int) -> int:
        """Write the 32-bit pattern over every scratch buffer of this handle's arena on the current stream (index and kept buffers
        and the weights are left alone); returns the bytes filled.  For tests/test_arena_state_gpu.py: no product code calls it."""
        with torch.cuda.device(self.device):
            n = int(self.lib.cap_debug_fill_arena(self._h, C.c_uint32(pattern & 0xFFFFFFFF), C.c_void_p(_stream_ptr(self.device))))
        if n < 0:
            raise N.CaptionerHipError(f"cap_debug_fill_arena: {N.last_error()}")
        return n

    def _arena_kinds(self) -> dict:
        """{"arena_bytes", "scratch_bytes", "index_bytes", "kept_bytes", "index": [names], "kept": [names]} of this handle's arena."""
        buf = C.create_string_buffer(1 << 12)
        N.check(self.lib.cap_debug_arena_kinds(self._h, buf, len(buf)), "cap_debug_arena_kinds")
        return json.loads(buf.value.decode())


class CaptionerEngine(_Engine):
    """One handle = one model replica on one GPU, bound to torch's current stream of `device` at each call."""

    _NO_GPU = "needs a GPU (torch.cuda.is_available() is False)"
    _skip_kv16_guard = False     # tests/probe_kv16_outliers.py sets it on an instance to load a checkpoint the guard refuses

    def __init__(self, arch: BlipArch, dtype: str = "bf16", max_batch: int = 8, max_beams: int = 1,
                 max_len: int = 20, device: str | torch.device = "cuda:0", share_weights_with: "CaptionerEngine | None" = None,
                 cross_cache: str = "auto", weight_int8: bool = False, max_prompt: int = 0, max_score_rows: int = 0):
        """max_score_rows (BLIP): scoring capacity in decoder rows (`score`): N captions of L tokens run as ONE pass with one vocabulary
        GEMM when N * (L - 1) <= max_score_rows; 0 reserves nothing (the arena is what it always was) and `score` works in passes of
        as many captions as the decode rows hold, the head over max_batch * max_beams rows at a time - same bits.
        max_prompt (BLIP): prompt capacity - with max_prompt >= P the P - 1 prompt positions of a FULL batch run through the decoder
        as one prefill pass (`generate(prompt_ids=)`); 0 reserves nothing (the arena is what it always was) and a prompted batch
        is prefilled in chunks of as many captions as the decode rows hold (`prompt_limit` = the longest prompt taken).
        weight_int8 (BLIP-2, dtype "bf16" only): the reference's `load_in_8bit=True` (blip2.py:19-22) - the OPT decoder layers' Linear
        weights are kept as row-quantised int8 + fp32 row scales (bitsandbytes' storage) and streamed as bytes by the decode GEMMs,
        the vision tower's Linears and language_projection pass through the same quantiser at load; activations stay bf16.
        cross_cache: "auto" = the mode's own cross-attention K/V cache ("f32s": KV16 - int16 + one scale per 64-wide head row,
        the decode side's HBM stream at half the bytes; "bf16": bf16 rows; "f32": fp32 rows); "fp32" = fp32 rows in "f32s" too
        (`cross_cache_kind` tells what the handle uses).
        share_weights_with: an engine of the same model / dtype / GPU whose (read-only) weights this one uses instead of
        holding a copy - it gets its own arena only (cap_create_shared); load_state_dict through either is seen by both."""
        super().__init__(arch, dtype, max_batch, max_len, device)
        self.max_beams = max_beams
        self.max_prompt = int(max_prompt)
        if self.max_prompt and (_arch_family(arch) != "blip" or not 2 <= self.max_prompt <= N.CAP_MAX_PROMPT):
            raise ValueError(f"max_prompt = {max_prompt}: prompt capacity is BLIP's, 0 or 2..{N.CAP_MAX_PROMPT} tokens (BOS included)")
        self.prompt_limit = prompt_token_limit(max_batch, max_beams, self.max_prompt)
        self.max_score_rows = int(max_score_rows)
        if self.max_score_rows and (_arch_family(arch) != "blip" or self.max_score_rows < 0):
            raise ValueError(f"max_score_rows = {max_score_rows}: scoring capacity is BLIP's, 0 or a row count")
        self.is_coca = isinstance(arch, CocaArch)
        self.is_blip2 = isinstance(arch, Blip2Arch)
        if cross_cache not in ("auto", "fp32"):
            raise ValueError(f"cross_cache must be 'auto' or 'fp32', got {cross_cache!r}")
        self.cross_cache = cross_cache
        self.weight_int8 = bool(weight_int8)
        if self.weight_int8 and not (self.is_blip2 and dtype == "bf16"):
            raise ValueError("weight_int8 (load_in_8bit) is built for BLIP-2 with dtype 'bf16'")
        cfg = self._config(3 if self.is_blip2 else 1 if self.is_coca else 0, max_beams)
        if self.is_coca:
            self._vision_tower(cfg, arch.eps)
            self._text_tower(cfg, arch.context_length + 1, arch.eps, (arch.sot, arch.eos, arch.pad))
            cfg.embed_dim, cfg.pool_queries, cfg.pool_heads = arch.embed_dim, arch.pool_queries, arch.pool_heads
            cfg.mm_layers, cfg.min_len = arch.mm_layers, arch.min_seq_len
        else:
            self._vision_tower(cfg, arch.v_eps)
            self._text_tower(cfg, arch.max_pos, arch.t_eps, (arch.bos, arch.eos, arch.pad))
        if self.is_blip2:
            self._qformer(cfg)
        cfg.max_prompt, cfg.max_score_rows = self.max_prompt, self.max_score_rows
        cfg.cross_kv_fp32, cfg.weight_int8 = int(cross_cache == "fp32"), int(self.weight_int8)
        self._create(cfg, share_weights_with)

    def set_early_exit(self, poll_steps: int) -> None:
        """Leave the decode loop once every caption is finished, as HF generate does; the device state is looked at every
        `poll_steps` steps (one stream synchronisation each).  0 = never (default): no host sync inside generate."""
        N.check(self.lib.cap_set_early_exit(self._h, int(poll_steps)), "cap_set_early_exit")

    def set_bad_words(self, seqs) -> None:
        """HF `generate(bad_words_ids=seqs)` for every generating call that follows (BLIP and BLIP-2, greedy and beams, every
        decode path; `score` ignores it): a list of token-id lists - one token = banned at every step, n > 1 tokens = the last is
        banned whenever the caption's last n - 1 context tokens are the first n - 1.  None or [] clears the set.  Validated on the
        host (`validate_bad_words_ids`) before anything is uploaded; the upload is complete when this returns.  With a set in
        force `generate` refuses output_logprobs / output_vocab_maxprob and beam groups (the library's rules, by name)."""
        seqs = validate_bad_words_ids(seqs, self.arch)
        flat = [t for q in seqs for t in q]
        offs = [0]
        for q in seqs:
            offs.append(offs[-1] + len(q))
        ids_a = (C.c_int32 * max(len(flat), 1))(*flat)
        offs_a = (C.c_int32 * len(offs))(*offs)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device)
            N.check(self.lib.cap_set_bad_words(self._h, ids_a, offs_a, len(seqs), C.c_void_p(stream.cuda_stream)), "cap_set_bad_words")
            stream.synchronize()             # the engine may next be used on another stream (EnginePool)
        self._bad_words = seqs

    @property
    def bad_words(self) -> List[List[int]]:
        """The set in force as `set_bad_words` took it (validated; `[eos]` alone dropped); [] = none."""
        return [list(q) for q in getattr(self, "_bad_words", [])]

    @property
    def bad_words_counts(self) -> tuple:
        """(distinct single tokens, multi-token sequences) as the library holds them (cap_bad_words)."""
        a, b = C.c_int(0), C.c_int(0)
        N.check(self.lib.cap_bad_words(self._h, C.byref(a), C.byref(b)), "cap_bad_words")
        return int(a.value), int(b.value)

    def set_repeat_controls(self, repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0) -> None:
        """HF `generate(repetition_penalty=, no_repeat_ngram_size=)` for every generating call that follows (BLIP and BLIP-2, greedy
        and beams, every decode path; `score` ignores them): the penalty divides the positive and multiplies the negative scores of
        every token of the caption's context, once per distinct token; the n-gram size bans every token that would repeat an n-gram
        of the context.  HF's order (penalty, n-grams, bad words) and HF's context: BLIP's BOS, prompt and generated tokens; BLIP-2's
        image placeholders, BOS and generated tokens.  The defaults (1.0, 0) switch both off.  Validated on the host
        (`validate_repeat_controls`) first.  With a control on, `generate` refuses output_logprobs / output_vocab_maxprob, beam
        groups and a CoCa engine (the library's rules, by name)."""
        p, n = validate_repeat_controls(repetition_penalty, no_repeat_ngram_size, self.arch, self.max_len)
        if self.is_blip2 and (p != 1.0 or n > 0):      # the placeholders HF's processors see in front of BOS
            N.check(self.lib.cap_set_image_token(self._h, int(self.arch.image_token)), "cap_set_image_token")
        N.check(self.lib.cap_set_repeat_controls(self._h, C.c_float(p), int(n)), "cap_set_repeat_controls")
        self._repeat_controls = (float(C.c_float(p).value), n)

    @property
    def repetition_penalty(self) -> float:
        """The penalty in force (`set_repeat_controls`), as the fp32 number the kernels use; 1.0 = off."""
        return getattr(self, "_repeat_controls", (1.0, 0))[0]

    @property
    def no_repeat_ngram_size(self) -> int:
        """The n-gram size in force (`set_repeat_controls`); 0 = off."""
        return getattr(self, "_repeat_controls", (1.0, 0))[1]

    @property
    def repeat_controls(self) -> tuple:
        """(penalty, n-gram size) as the library holds them (cap_repeat_controls)."""
        a, b = C.c_float(0), C.c_int(0)
        N.check(self.lib.cap_repeat_controls(self._h, C.byref(a), C.byref(b)), "cap_repeat_controls")
        return float(a.value), int(b.value)

    def set_sampling(self, do_sample: bool = False, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, seed: int = 0) -> None:
        """HF `generate(do_sample=True, temperature=, top_k=, top_p=)` for every greedy generating call that follows (BLIP and
        BLIP-2, num_beams = 1, every decode path; `score` ignores it): the token of a step is drawn inside the selection kernel from
        the processed row (repetition controls and bad words in force) divided by the temperature, cut to the top_k best values
        (0 = off; ties stay) and to the nucleus of mass top_p (1.0 = off), by an inverse CDF over 40-bit fixed-point weights with a
        Philox4x32-10 uniform of (seed, the caption's key, the step) - INTEGRATION.md section 6g.  A caption's tokens depend on its
        logits, these numbers, its key and the step alone.  The defaults switch sampling off.  Validated on the host
        (`validate_sampling`) first.  Setting resets the engine's call counter, which numbers the default keys.  With sampling on,
        `generate` refuses beams, beam groups, output_logprobs / output_vocab_maxprob and a CoCa engine (by name)."""
        on, t, k, p, sd = validate_sampling(do_sample, temperature, top_k, top_p, seed, self.arch)
        N.check(self.lib.cap_set_sampling(self._h, int(on), C.c_float(t), int(k), C.c_float(p), C.c_uint64(sd)), "cap_set_sampling")
        self._sampling = (on, t, k, p, sd)
        self._sample_call_no = 0

    _NO_SAMPLING = (False, 1.0, 0, 1.0, 0)

    @property
    def do_sample(self) -> bool:
        """Whether the greedy loop draws its tokens (`set_sampling`)."""
        return getattr(self, "_sampling", self._NO_SAMPLING)[0]

    @property
    def temperature(self) -> float:
        """The temperature in force (`set_sampling`), as the fp32 number the kernel divides by."""
        return getattr(self, "_sampling", self._NO_SAMPLING)[1]

    @property
    def top_k(self) -> int:
        """The top-k count in force (`set_sampling`); 0 = off."""
        return getattr(self, "_sampling", self._NO_SAMPLING)[2]

    @property
    def top_p(self) -> float:
        """The nucleus mass in force (`set_sampling`), as the fp32 number the kernel reads; 1.0 = off."""
        return getattr(self, "_sampling", self._NO_SAMPLING)[3]

    @property
    def sample_seed(self) -> int:
        """The Philox key in force (`set_sampling`)."""
        return getattr(self, "_sampling", self._NO_SAMPLING)[4]

    @property
    def sampling(self) -> tuple:
        """(on, temperature, top_k, top_p, seed) as the library holds them (cap_sampling)."""
        on, t, k, p, sd = C.c_int(0), C.c_float(0), C.c_int(0), C.c_float(0), C.c_uint64(0)
        N.check(self.lib.cap_sampling(self._h, C.byref(on), C.byref(t), C.byref(k), C.byref(p), C.byref(sd)), "cap_sampling")
        return bool(on.value), float(t.value), int(k.value), float(p.value), int(sd.value)

    def next_sample_call(self) -> int:
        """The number of the next call that takes default sample keys, and advance the counter (`set_sampling` resets it)."""
        n = getattr(self, "_sample_call_no", 0)
        self._sample_call_no = n + 1
        return n

    @property
    def last_decode_steps(self) -> int:
        return int(self.lib.cap_last_decode_steps(self._h))

    @property
    def cross_cache_kind(self) -> str:
        """Layout of this handle's cross-attention K/V cache: "fp32", "bf16" or "kv16"."""
        return {0: "fp32", 1: "bf16", 2: "kv16"}[int(self.lib.cap_cross_cache_kind(self._h))]

    DECODE_PATHS = {"auto": 0, "batch": 1, "small": 2}

    def set_decode_path(self, path: str) -> None:
        """Kernels of the decode steps (BLIP, "f32s" / "bf16"): "auto" = the fused small-batch kernels for images x beams <= 16
        rows (6 launches per layer-step instead of 11; same bits), the batch kernels above; "batch" / "small" force one
        (forcing "small" makes generate fail for calls those kernels do not take)."""
        N.check(self.lib.cap_set_decode_path(self._h, self.DECODE_PATHS[path]), "cap_set_decode_path")

    def set_row_compaction(self, on: bool) -> None:
        """Greedy BLIP decode on the batch kernels: work on the rows of the captions still open only (default on; same tokens
        and lengths either way - off is for A/B runs and the equality tests)."""
        N.check(self.lib.cap_set_row_compaction(self._h, int(bool(on))), "cap_set_row_compaction")

    @property
    def last_row_compaction(self) -> bool:
        return int(self.lib.cap_last_row_compaction(self._h)) == 1

    @property
    def last_prefill_passes(self) -> int:
        """Prefill passes of the last prompted generate: 1 = the whole batch at once (0 after an unprompted call)."""
        return int(self.lib.cap_last_prefill_passes(self._h))

    @property
    def last_decode_path(self) -> str:
        return {0: "none", 1: "batch", 2: "small"}[int(self.lib.cap_last_decode_path(self._h))]

    # ------------------------------------------------------------------------------------------ weights
    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True) -> Dict[str, object]:
        """HF BLIP key names or an open_clip CoCa state dict (derived tensors are added here).
        Tensors the architecture does not store (tied heads, buffers) are skipped and reported; with strict=True missing
        ones raise.  A dict in which NOTHING matches always raises - it is a wrong checkpoint or wrong key prefixes, never a
        successful load.  Returns {"matched": n, "unknown": [names]}."""
        with _deriving_tensors():
            if self.is_coca and "derived.pool_q" not in sd:
                from .coca_weights import coca_library_state_dict
                sd = coca_library_state_dict(sd, self.arch)
            if self.is_blip2:
                sd = _with_qformer_x0(sd, self.arch.q_eps)
            if self.weight_int8:
                from .weights import blip2_int8_host_names, int8_roundtrip
                sd = dict(sd)
                for k in blip2_int8_host_names(sd):
                    sd[k] = int8_roundtrip(sd[k])
        # the KV16 cross-attention cache has ONE scale per 64-wide head row: a checkpoint whose key / value heads carry outlier
        # dimensions is refused here (measured bound: weights.KV16_MAX_HEAD_SPREAD), never served with coarser logits
        if not self._skip_kv16_guard and self.cross_cache_kind == "kv16":
            from .weights import KV16_MAX_HEAD_SPREAD, cross_kv_head_spread
            spread = cross_kv_head_spread(sd)
            if spread > KV16_MAX_HEAD_SPREAD:
                raise N.CaptionerHipError(
                    f"the cross-attention key / value heads of this checkpoint have dimensions {spread:.1f}x their head's median "
                    f"magnitude; the split mode's KV16 cache (one scale per 64-wide head row) holds the 1e-3 logit bar up to "
                    f"{KV16_MAX_HEAD_SPREAD:.0f}x - create the engine with cross_cache='fp32' (captioner.cross_cache: fp32; the "
                    f"wrappers choose it themselves), or use dtype 'f32' / 'bf16'")
        return self._stream_weights(sd, strict)

    # ------------------------------------------------------------------------------------------ forward
    @property
    def image_state_bytes(self) -> int:
        """Bytes of one image's state on this engine (cap_image_state_bytes)."""
        n = int(self.lib.cap_image_state_bytes(self._h))
        if n <= 0:
            raise N.CaptionerHipError(f"cap_image_state_bytes: {N.last_error()}")
        return n

    def image_state(self, pixels: torch.Tensor) -> torch.Tensor:
        """The image side alone: frames as `generate` takes them -> a plain uint8 [B, image_state_bytes] device tensor, one row per
        image, holding what the decode side reads from the image side (BLIP / CoCa: the image's cross-attention K/V rows in this
        engine's cache kind; BLIP-2: its language-projection rows).  `generate` and `score` take such a tensor where they take
        pixels and then skip the image side; the results are the bits of the calls from the pixels.  It is a tensor and nothing
        more: subsets, reorderings and repeats of images are indexing (`state[[4, 0, 0, 2]]`), batches are `torch.cat`, and a state
        made on one engine decodes on any engine of the same architecture, compute type and cross-cache kind that has the same
        weights (a pool's engines do).  Only the row size is checked on the way back in: a state made with OTHER WEIGHTS, or by
        an engine of another image size whose records happen to have this size, is the caller's to keep apart - it decodes without
        an error to captions of that other model's image.  More than max_batch frames go in calls of max_batch."""
        pixels, fmt = self._pixels(pixels)
        if fmt == N.CAP_PIX_IMAGE_STATE:
            raise ValueError("image_state takes frames, got an image state")
        B, nbytes = int(pixels.shape[0]), self.image_state_bytes
        out = torch.empty((B, nbytes), dtype=torch.uint8, device=self.device)
        for b0 in range(0, B, self.max_batch):
            nb = min(self.max_batch, B - b0)
            self._call("cap_encode_image_state", pixels[b0:b0 + nb], fmt, nb, out[b0:b0 + nb])
        return out

    def _pixels(self, pixels: torch.Tensor):
        """Frames as every engine takes them, or an image state: two dimensions, not uint8 [B, S, S, 3] frames."""
        if not is_image_state(pixels):
            return super()._pixels(pixels)
        validate_image_state(pixels, self.image_state_bytes)
        return pixels.to(self.device, non_blocking=True).contiguous(), N.CAP_PIX_IMAGE_STATE

    def encode(self, pixels: torch.Tensor) -> torch.Tensor:
        pixels, fmt = self._pixels(pixels)
        B = pixels.shape[0]
        shape = (B, self.arch.pool_queries, self.arch.embed_dim) if self.is_coca else (B, self.arch.n_tokens, self.arch.v_hidden)   # BLIP / BLIP-2: ViT image_embeds
        out = torch.empty(shape, dtype=torch.float32, device=self.device)
        self._call("cap_encode", pixels, fmt, B, out)
        return out

    def _decode_steps(self, max_length: int) -> int:
        """Steps the decode loop runs for a max_length: BLIP-2's counts new tokens, BLIP's and CoCa's count BOS too."""
        return max_length if self.is_blip2 else max_length - 1

    def generate(self, pixels: torch.Tensor, num_beams: int = 1, max_length: Optional[int] = None,
                 length_penalty: float = 1.0, output_logits: bool = False, num_beam_groups: Optional[int] = None,
                 output_logprobs: bool = False, output_vocab_maxprob: bool = False, prompt_ids=None, bad_words_ids=None,
                 repetition_penalty=None, no_repeat_ngram_size=None, sample_keys=None, num_return_sequences=None,
                 **sampling_options) -> Dict[str, torch.Tensor]:
        """prompt_ids (BLIP, greedy): a host list / tensor [P], [1, P] (one prompt for every caption) or [B, P] (one per caption), column
        0 = BOS - HF `BlipForConditionalGeneration.generate(pixel_values, input_ids=...)`, whose decoder receives input_ids[:, :-1].
        Validated on the host (`validate_prompt_ids`).  max_length counts the prompt; `sequences` start with it and `lengths`
        include it; `logits` ([max_length - P, B, vocab]), `token_logprobs`, `scored_steps` and `vocab_maxprob` cover the GENERATED
        steps only (entry j = the j-th generated token; the tail of a token_logprobs row stays zero).
        Returns device tensors: sequences int32 [B, max_length] (incl. BOS), lengths int32 [B],
        sequences_scores fp32 [B] (beams only), logits fp32 [max_length-1, B*num_beams, vocab] (optional).
        BLIP-2: max_length counts NEW tokens (HF max_new_tokens); sequences are those new tokens only (no image
        placeholders / BOS), logits [max_length, B*num_beams, vocab]; num_beams > 1 as for BLIP (HF's search behind a prompt pass
        that runs once per image: step 0's rows of an image are copies).
        output_logprobs (greedy): token_logprobs fp32 [B, steps] = log max softmax of every step's logits row as the selection saw
        it (steps as for logits), zero from the caption's end on, and scored_steps int32 [B] = valid entries per row - taken by the
        selection kernel itself (cap_generate_scored): any batch size, no logits buffer, same kernels otherwise;
        `perplexity_from_logprobs` turns them into the reference's per-caption perplexity.
        output_vocab_maxprob (greedy): vocab_maxprob fp32 [B, vocab] = every vocabulary entry's maximal softmax probability over the
        steps at which the caption was open (`scored_steps` of them; 0 where nothing ran) - what the reference's probability fusion
        takes from per-step logits, kept by the selection kernel instead (cap_generate_vocab).  A view without the row padding of
        the [B, acc_ld] buffer behind it; token_logprobs / scored_steps come with it; `fuse_vocab_groups` is its consumer.
        num_beam_groups (CoCa): the reference's `_generate_beamsearch` with that many beam groups (coca_model.py:335-482;
        its `generate()` defaults are 6 beams in 3 groups) - cap_generate_groups; no per-step logits in that mode.
        bad_words_ids: accepted when it equals the set in force (`set_bad_words`, `.bad_words`; None = not given), refused by name
        otherwise - the set is engine state, not a per-call option.
        repetition_penalty / no_repeat_ngram_size: likewise accepted when they equal the values in force (`set_repeat_controls`; None =
        not given), refused by name otherwise; they never reach `reject_unsupported_generation_options`.
        do_sample / temperature / top_k / top_p: with sampling in force (`set_sampling`) they are taken out of sampling_options and
        accepted when they equal the values in force, refused by name otherwise - the sampling state is engine state too.  Without
        it they go the way of every other sampling option below, as they always did.
        sample_keys (sampling only): an int64 tensor [B], caption b's 64-bit key; the default is (call_no << 32) | b, call_no = the
        number of default-keyed calls since `set_sampling` - repeated calls differ and are reproducible.  A call with given keys
        does not advance the counter.
        num_return_sequences = n (sampling only): `image_state` once, every record n times, keys (call_no << 32) | (b * n + r);
        sequences [B * n, L], image-major (HF's order).  Refused by name when B * n exceeds max_batch.
        sampling_options: anything else a caller of the reference's / HF's `generate` may pass (top_p, top_k, temperature,
        repetition_penalty, do_sample, ...): accepted at their neutral values, rejected BY NAME otherwise - never ignored."""
        if output_vocab_maxprob and (num_beam_groups is not None or num_beams != 1):      # before anything is allocated or run
            raise N.CaptionerHipError("output_vocab_maxprob is the greedy loop's (num_beams = 1): beam search "
                                      f"(num_beams = {num_beams}, num_beam_groups = {num_beam_groups}) keeps no per-step distribution")
        if bad_words_ids is not None and validate_bad_words_ids(bad_words_ids, self.arch) != self.bad_words:
            raise ValueError(f"generate: bad_words_ids differs from the set in force on this engine ({len(self.bad_words)} sequences): "
                             "the banned set is engine state - call set_bad_words(bad_words_ids) first")
        for name, given, held in (("repetition_penalty", repetition_penalty, self.repetition_penalty),
                                  ("no_repeat_ngram_size", no_repeat_ngram_size, self.no_repeat_ngram_size)):
            if given is None:
                continue
            p, n = validate_repeat_controls(given if name == "repetition_penalty" else None,
                                            given if name == "no_repeat_ngram_size" else None, self.arch, self.max_len)
            want = float(C.c_float(p).value) if name == "repetition_penalty" else n
            if want != held:
                raise ValueError(f"generate: {name} = {given!r} differs from the value in force on this engine ({held!r}): the repetition "
                                 f"controls are engine state - call set_repeat_controls first")
        if self.do_sample:          # the four keys are engine state: taken out before the judgement of the unbuilt options
            held = {"do_sample": True, "temperature": self.temperature, "top_k": self.top_k, "top_p": self.top_p}
            for name in list(held):
                if name not in sampling_options:
                    continue
                given = sampling_options.pop(name)
                if given is None:
                    continue
                _, t_, k_, p_, _ = validate_sampling(True, given if name == "temperature" else None, given if name == "top_k" else None,
                                                     given if name == "top_p" else None, None, self.arch)
                want = {"do_sample": bool(given), "temperature": t_, "top_k": k_, "top_p": p_}[name]
                if want != held[name]:
                    raise ValueError(f"generate: {name} = {given!r} differs from the value in force on this engine ({held[name]!r}): the "
                                     f"sampling state is engine state - call set_sampling first")
        elif sample_keys is not None or num_return_sequences not in (None, 1):
            raise ValueError("generate: " + ("sample_keys" if sample_keys is not None else f"num_return_sequences = {num_return_sequences!r}") +
                             " needs sampling in force on this engine (set_sampling(do_sample=True, ...)): the arg-max loop takes no keys "
                             "and returns one caption per image")
        if num_return_sequences not in (None, 1):
            n = num_return_sequences
            if isinstance(n, bool) or not hasattr(n, "__index__") or int(n) < 1:
                raise ValueError(f"generate: num_return_sequences must be an integer >= 1, got {n!r}")
            n, B0 = int(n), int(pixels.shape[0])
            if B0 * n > self.max_batch:
                raise ValueError(f"generate: num_return_sequences = {n} for {B0} images is {B0 * n} decode rows, more than this engine's "
                                 f"max_batch = {self.max_batch}")
            if prompt_ids is not None:
                prompt_ids = validate_prompt_ids(prompt_ids, self.arch, B0, max_length or self.max_len, num_beams, num_beam_groups,
                                                 self.prompt_limit)
                if prompt_ids.shape[0] == B0 and B0 > 1:
                    prompt_ids = prompt_ids.repeat_interleave(n, dim=0)
            state = pixels if is_image_state(pixels) else self.image_state(pixels)
            if sample_keys is None:
                sample_keys = torch.from_numpy(return_sequence_keys(self.next_sample_call(), B0, n).view(np.int64))
            return self.generate(state.repeat_interleave(n, dim=0), num_beams=num_beams, max_length=max_length, length_penalty=length_penalty,
                                 output_logits=output_logits, num_beam_groups=num_beam_groups, output_logprobs=output_logprobs,
                                 output_vocab_maxprob=output_vocab_maxprob, prompt_ids=prompt_ids, sample_keys=sample_keys,
                                 **sampling_options)
        if sampling_options:
            from .captioner.generation_options import reject_unsupported_generation_options, _NEUTRAL
            known = set(_NEUTRAL) | {"generation_type", "top_k", "top_p"}
            unknown = sorted(set(sampling_options) - known)
            if unknown:
                raise TypeError(f"generate() got unexpected keyword argument(s) {unknown}")
            reject_unsupported_generation_options(sampling_options, "CaptionerEngine.generate")
        L = max_length or self.max_len
        prompt = None
        if prompt_ids is not None:               # host check first: nothing unvalidated is uploaded or gathered from
            prompt = validate_prompt_ids(prompt_ids, self.arch, int(pixels.shape[0]), L, num_beams, num_beam_groups, self.prompt_limit)
        pixels, fmt = self._pixels(pixels)
        B = pixels.shape[0]
        ids = torch.empty((B, L), dtype=torch.int32, device=self.device)
        lens = torch.empty((B,), dtype=torch.int32, device=self.device)
        scores = torch.zeros((B,), dtype=torch.float32, device=self.device)
        steps = self._decode_steps(L)
        logits = lps = scored = vmax = prompt_d = keys_d = None
        if self.do_sample:           # one key per caption: given, or numbered by the engine's call counter
            keys_h = (keys_tensor(sample_keys, B) if sample_keys is not None else
                      torch.from_numpy(default_sample_keys(self.next_sample_call(), B).view(np.int64)))
        if output_logits:
            # zeros, not empty: with early exit the steps after the last executed one are never written (callers see 0, not
            # stale memory); `last_decode_steps` tells how many steps ran
            logits = torch.zeros((steps if prompt is None else L - int(prompt.shape[1]), B * num_beams, self.arch.vocab),
                                 dtype=torch.float32, device=self.device)
        if output_vocab_maxprob:
            output_logprobs = True
            acc_ld = (self.arch.vocab + 3) // 4 * 4
            vmax = torch.empty((B, acc_ld), dtype=torch.float32, device=self.device)      # zero-filled by the library
        if output_logprobs:
            if num_beam_groups is not None:
                raise N.CaptionerHipError("output_logprobs is the greedy loop's (num_beams = 1): the group beam search "
                                          f"(num_beams = {num_beams}, num_beam_groups = {num_beam_groups}) returns sequences_scores")
            # the library zero-fills both on this stream (entries after a caption's end and steps an early exit skipped stay 0)
            lps = torch.empty((B, steps), dtype=torch.float32, device=self.device)
            scored = torch.empty((B,), dtype=torch.int32, device=self.device)
        if num_beam_groups is not None and output_logits:
            raise ValueError("per-step logits are not recorded by the group beam search")
        ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731 - an absent buffer is NULL
        req = N.CapGenerateArgs(pixels=ptr(pixels), pixel_fmt=fmt, B=B, num_beams=num_beams, max_len=L, length_penalty=length_penalty,
                                out_ids=ptr(ids), out_len=ptr(lens), out_scores=ptr(scores), out_step_logits=ptr(logits),
                                out_logprobs=ptr(lps), out_scored=ptr(scored), out_vocab=ptr(vmax),
                                acc_ld=0 if vmax is None else vmax.shape[1])
        if num_beam_groups is not None:          # 0 is the library's "no groups": a count below 1 goes in as one it refuses
            req.num_beam_groups = max(int(num_beam_groups), -1) or -1
        with torch.cuda.device(self.device):
            if prompt is not None:
                prompt_d = prompt.to(self.device, non_blocking=False)
                req.prompt_ids, req.prompt_rows, req.prompt_len = prompt_d.data_ptr(), int(prompt.shape[0]), int(prompt.shape[1])
            if self.do_sample:
                keys_d = keys_h.to(self.device, non_blocking=False)
                N.check(self.lib.cap_generate_sampled(self._h, C.byref(req), C.c_void_p(keys_d.data_ptr()),
                                                      C.c_void_p(_stream_ptr(self.device))), "cap_generate_sampled")
            else:
                N.check(self.lib.cap_generate_request(self._h, C.byref(req), C.c_void_p(_stream_ptr(self.device))), "cap_generate_request")
            for t_ in (prompt_d, keys_d):
                if t_ is not None:
                    t_.record_stream(torch.cuda.current_stream(self.device))
        if num_beam_groups is not None:
            return {"sequences": ids, "lengths": lens, "sequences_scores": scores}
        out = {"sequences": ids, "lengths": lens}
        if lps is not None:
            out["token_logprobs"], out["scored_steps"] = lps, scored
        if vmax is not None:
            out["vocab_maxprob"] = vmax[:, :self.arch.vocab]
        if num_beams > 1:
            out["sequences_scores"] = scores
        if logits is not None:
            out["logits"] = logits
        return out

    @property
    def score_limit(self) -> int:
        """Longest caption (tokens, BOS included) `score` takes on this engine: BLIP's max_len counts BOS and one prefill pass covers 31
        positions; BLIP-2's max_len counts the tokens behind BOS, within the OPT decoder's positions."""
        if self.is_blip2:
            return min(self.max_len, self.arch.max_pos - self.arch.num_query_tokens - 1) + 1
        return min(self.max_len, SCORE_MAX_TOKENS)

    @property
    def last_score_passes(self) -> int:
        """Decoder passes of the last cap_score_captions call (`score` makes one call per max_batch images)."""
        return int(self.lib.cap_last_score_passes(self._h))

    def score(self, pixels: torch.Tensor, ids, lens, captions_per_image: int = 1, sort_by_length: bool = True) -> Dict[str, torch.Tensor]:
        """Teacher-forced log-probs of GIVEN captions under the captioner (BLIP, BLIP-2) - HF `model(pixel_values, input_ids=...)` reduced on
        the device.  ids [N, L] (column 0 = BOS) and lens [N] (tokens incl. BOS, and EOS / [SEP] if the end is to be scored; 0 = an
        absent slot when captions_per_image > 1) are host lists / tensors, N = B * captions_per_image, caption n belongs to image
        n // captions_per_image; columns from lens[n] on are padding.  Validated on the host first (`validate_score_ids`).
        Returns device tensors: token_logprobs fp32 [N, L - 1] (entry j = log_softmax(logits at position j)[ids[n, j + 1]] for j <
        lens[n] - 1, 0 behind), top_logprobs fp32 / top_ids int32 [N, L - 1] (log max softmax and arg-max of the same rows), scored
        int32 [N] = lens - 1.  Plain logits: no EOS mask, no MinLength, no label smoothing.
        The image side runs once per image.  More than max_batch images go in calls of max_batch; each call is trimmed to its own
        longest caption, and with captions_per_image == 1 and sort_by_length the pairs are sorted by length first (and un-sorted
        on return) so that a call's rows are its own maximum.  None of this changes a caption's bits."""
        Cn = int(captions_per_image)
        B = int(pixels.shape[0])
        ids_h, lens_h = validate_score_ids(ids, lens, self.arch, B, Cn, self.score_limit)
        need = max(int(lens_h.max()), 2) - 1
        if int(self.lib.cap_score_pass_captions(self._h, need + 1)) == 0:        # the handle's own capacity: nothing is uploaded
            raise ValueError(f"score: a caption of {need + 1} tokens is {need} decoder rows, more than this engine's workspace holds: "
                             f"no chunking fits it - create the engine with " +
                             ("a larger max_batch" if self.is_blip2 else f"max_score_rows >= {need}"))
        pixels, fmt = self._pixels(pixels)
        N_, L = int(ids_h.shape[0]), int(ids_h.shape[1])
        dev = self.device
        out = {"token_logprobs": torch.zeros((N_, L - 1), dtype=torch.float32, device=dev),
               "top_logprobs": torch.zeros((N_, L - 1), dtype=torch.float32, device=dev),
               "top_ids": torch.zeros((N_, L - 1), dtype=torch.int32, device=dev),
               "scored": torch.zeros((N_,), dtype=torch.int32, device=dev)}
        order = None
        if Cn == 1 and sort_by_length and B > self.max_batch:
            order = torch.argsort(lens_h, stable=True, descending=True)
            ids_h, lens_h = ids_h[order], lens_h[order]
            pixels = pixels[order.to(dev)]
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            for b0 in range(0, B, self.max_batch):
                nb = min(self.max_batch, B - b0)
                rows = slice(b0 * Cn, (b0 + nb) * Cn)
                Lc = max(int(lens_h[rows].max()), 2)
                ids_d = ids_h[rows, :Lc].contiguous().to(dev)
                lens_d = lens_h[rows].contiguous().to(dev)
                px = pixels[b0:b0 + nb]
                n = nb * Cn
                tlp = torch.empty((n, Lc - 1), dtype=torch.float32, device=dev)        # zero-filled by the library
                top = torch.empty((n, Lc - 1), dtype=torch.float32, device=dev)
                tid = torch.empty((n, Lc - 1), dtype=torch.int32, device=dev)
                sc = torch.empty((n,), dtype=torch.int32, device=dev)
                self._call("cap_score_captions", px, fmt, nb, ids_d, lens_d, Cn, Lc, tlp, top, tid, sc)
                for t in (ids_d, lens_d):
                    t.record_stream(stream)
                dst = rows if order is None else order[rows].to(dev)
                for key, val in (("token_logprobs", tlp), ("top_logprobs", top), ("top_ids", tid)):
                    out[key][dst, :Lc - 1] = val
                out["scored"][dst] = sc
        return out

    def fuse_vocab_groups(self, vocab_maxprob: torch.Tensor, groups: Sequence[Sequence[int]], th: float,
                          max_tokens: Optional[int] = None):
        """The group half of the probability fusion, on the device: per group of rows of `vocab_maxprob` (fp32 [N, vocab] from
        `generate(output_vocab_maxprob=True)`, any row stride), the fp32 mean over the members in listed order and the tokens whose
        mean exceeds `th` (strict), in ascending id order.  -> (ids int32 [G, K], probs fp32 [G, K], counts int32 [G]); row g holds
        counts[g] entries, the rest is -1 / 0.
        Default K = ceil(steps / th), steps = this engine's decode steps.  It cannot overflow: a step's softmax sums to 1, so for one
        caption sum_i max_t p_t(i) <= sum_t sum_i p_t(i) = steps, a mean over captions keeps that bound, and k tokens above th need
        k * th < steps: fewer than steps / th of them.  With a caller's smaller max_tokens a group that keeps more raises."""
        v = vocab_maxprob
        if v.dim() != 2 or v.dtype != torch.float32 or not v.is_cuda or v.stride(1) != 1 or v.shape[0] < 1 or v.shape[1] < 1:
            raise ValueError(f"vocab_maxprob must be a device fp32 [N, vocab] tensor with unit column stride, got {tuple(v.shape)} {v.dtype}")
        th = float(th)
        if not math.isfinite(th):
            raise ValueError(f"th must be finite, got {th}")
        Nr, V = int(v.shape[0]), int(v.shape[1])
        G = len(groups)
        K = fusion_max_tokens(self._decode_steps(self.max_len), th, V) if max_tokens is None else int(max_tokens)
        if K < 1:
            raise ValueError(f"max_tokens must be at least 1, got {K}")
        ids = torch.full((G, K), -1, dtype=torch.int32, device=v.device)
        probs = torch.zeros((G, K), dtype=torch.float32, device=v.device)
        counts = torch.zeros((G,), dtype=torch.int32, device=v.device)
        if G == 0:
            return ids, probs, counts
        rows, off = vocab_group_csr(groups, Nr)
        rows_d, off_d = rows.to(v.device), off.to(v.device)
        acc_ld = int(v.stride(0)) if Nr > 1 else max(int(v.stride(0)), V)
        _launch(self.lib, v.device, "cap_op_vocab_group_threshold", v, acc_ld, V, Nr, rows_d, int(rows.numel()), off_d, G,
                C.c_float(th), K, ids, probs, counts)
        if max_tokens is not None:
            over = (counts > K).nonzero().flatten().tolist()
            if over:
                raise N.CaptionerHipError(f"fuse_vocab_groups: group(s) {over[:8]} keep {counts[over[0]].item()} tokens above th = {th}, "
                                          f"more than max_tokens = {K}")
        return ids, probs, counts


class EnginePool:
    """Several CaptionerEngines on their own streams: consecutive batches overlap.  Every engine has its own arena (activations,
    K/V caches); the weights exist ONCE - engines 1.. are created on engine 0's weight store (cap_create_shared).

    One `cap_generate` is a chain of ~2 800 dependent kernels; between two dependent kernels of one HIP queue the GPU
    idles for the dispatch hand-over, and the decode kernels' small grids leave CUs free.  Independent batches do not depend
    on each other, so kernels of another queue run in those gaps AND next to them: in the pooled rocprofv3 trace kernels of
    different streams do co-run ("Overlapping whole batches"), and a pooled step is SHORTER than the sum
    of one batch's kernel durations.  What bounds the pool is the MFMA-bound image side, which two batches cannot run faster
    than one after the other.  Every batch is computed by exactly the kernels of a single engine: results are the same bits.

        pool = EnginePool(arch, n=3, dtype="bf16", max_batch=256)
        pool.load_state_dict(sd)
        outs = pool.generate_many(batches)            # or: out = pool.submit(px) ... pool.join()
    """

    def __init__(self, arch, n: int = 2, device: str | torch.device = "cuda:0", engine_cls=None, weights_of=None, **engine_kw):
        """weights_of: an existing engine whose weight store ALL n engines of the pool attach to (nothing to load then)."""
        if n < 1:
            raise ValueError("EnginePool needs at least one engine")
        self.device = torch.device(device)
        engine_cls = engine_cls or CaptionerEngine           # TextEncoderEngine: submit(ids, lens, method="embed")
        first = engine_cls(arch, device=device, share_weights_with=weights_of, **engine_kw)
        self.engines = [first] + [engine_cls(arch, device=device, share_weights_with=first, **engine_kw) for _ in range(n - 1)]
        with torch.cuda.device(self.device):
            self.streams = [torch.cuda.Stream(self.device) for _ in range(n)]
        self.arch, self._next = arch, 0
        self.last_coalesce = None

    def __len__(self) -> int:
        return len(self.engines)

    def load_state_dict(self, sd, strict: bool = True):
        return self.engines[0].load_state_dict(sd, strict=strict)      # one weight store behind every engine of the pool

    def set_early_exit(self, poll_steps: int) -> None:
        for e in self.engines:
            e.set_early_exit(poll_steps)

    def set_decode_path(self, path: str) -> None:
        for e in self.engines:
            e.set_decode_path(path)

    def set_bad_words(self, seqs) -> None:
        for e in self.engines:
            e.set_bad_words(seqs)

    @property
    def bad_words(self):
        return self.engines[0].bad_words

    def set_repeat_controls(self, repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0) -> None:
        for e in self.engines:
            e.set_repeat_controls(repetition_penalty, no_repeat_ngram_size)

    @property
    def repetition_penalty(self) -> float:
        return self.engines[0].repetition_penalty

    @property
    def no_repeat_ngram_size(self) -> int:
        return self.engines[0].no_repeat_ngram_size

    def set_sampling(self, do_sample: bool = False, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, seed: int = 0) -> None:
        """`CaptionerEngine.set_sampling` on every engine; resets the POOL's call counter, which numbers the batches of
        `generate_many` (batch j of a call takes call number counter + j, whichever engine or merged pass runs it)."""
        for e in self.engines:
            e.set_sampling(do_sample, temperature, top_k, top_p, seed)
        self._sample_call_no = 0

    @property
    def do_sample(self) -> bool:
        return self.engines[0].do_sample

    def batch_sample_keys(self, rows: Sequence[int]) -> List[torch.Tensor]:
        """The default keys of consecutive batches with these row counts, numbered from the pool's counter (which advances by their
        number): batch j's caption r has key ((counter + j) << 32) | r - what `engine.generate` gives a lone call of that number."""
        c0 = getattr(self, "_sample_call_no", 0)
        self._sample_call_no = c0 + len(rows)
        return [torch.from_numpy(default_sample_keys(c0 + j, int(r)).view(np.int64)) for j, r in enumerate(rows)]

    def set_row_compaction(self, on: bool) -> None:
        for e in self.engines:
            e.set_row_compaction(on)

    def close(self) -> None:
        for e in self.engines:
            e.close()

    @property
    def device_bytes(self) -> int:
        return sum(e.device_bytes for e in self.engines)

    def run(self, n: int, *inputs: torch.Tensor, **kw):
        """The same batch n times, rotating over the engines (benchmarks); returns the last output after join()."""
        out = None
        for _ in range(n):
            out = self.submit(*inputs, **kw)
        self.join()
        return out

    def submit(self, *inputs: torch.Tensor, then=None, method: str = "generate", **kw):
        """Start one batch on the next engine / stream - `engine.<method>(*inputs, **kw)` - and return its output (or
        `then(out)`, run on that stream) at once; the tensors are valid for the caller's stream after `join()`.  The inputs
        may come from the caller's stream."""
        i, self._next = self._next, (self._next + 1) % len(self.engines)
        s = self.streams[i]
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):
            out = getattr(self.engines[i], method)(*inputs, **kw)
            for t in inputs:
                if isinstance(t, torch.Tensor) and t.is_cuda:
                    t.record_stream(s)
            return then(out) if then is not None else out

    def join(self) -> None:
        """Make the caller's stream wait for everything submitted so far (device-side dependency, no host sync)."""
        cur = torch.cuda.current_stream(self.device)
        for s in self.streams:
            cur.wait_stream(s)

    # outputs of `generate` whose leading dimension is the batch's rows (what a merged pass is split back by)
    _PER_ROW_OUTPUTS = ("sequences", "lengths", "sequences_scores", "token_logprobs", "scored_steps", "vocab_maxprob")

    @staticmethod
    def coalesce_plan(rows: Sequence[int], n_engines: int, max_rows: int) -> List[List[int]]:
        """Dynamic batching plan: consecutive batches (their row counts in `rows`) merged into passes of at most `max_rows` rows -
        as few passes as the rows allow, but never fewer than engines (concurrency comes first) and rounded up to a multiple of
        the engine count (every engine runs the same number of passes); the rows spread over the passes as evenly as the order
        permits.  -> lists of batch indices, in order.  A batch larger than `max_rows` is a pass of its own."""
        nb = len(rows)
        if nb == 0:
            return []
        if max_rows <= 0:
            return [[i] for i in range(nb)]
        total = sum(rows)
        passes = max(-(-total // max_rows), min(nb, n_engines))
        if passes % n_engines:
            passes = min(nb, (passes // n_engines + 1) * n_engines)
        plan: List[List[int]] = []
        cur: List[int] = []
        cur_rows, left = 0, total
        for i, r in enumerate(rows):
            groups_left = max(1, passes - len(plan))
            # close the open pass when the next batch would overflow it, or when it already holds its share of what is left
            if cur and (cur_rows + r > max_rows or cur_rows >= (left + cur_rows) / groups_left):
                plan.append(cur)
                cur, cur_rows = [], 0
            cur.append(i)
            cur_rows += r
            left -= r
        plan.append(cur)
        return plan

    @classmethod
    def coalesce_plan_prompted(cls, rows: Sequence[int], n_engines: int, max_rows: int, prompt_lens: Sequence[int]) -> List[List[int]]:
        """`coalesce_plan` for prompted batches: every row of a pass has the same prompt length, so only consecutive batches whose
        prompt lengths agree are ever merged - each run of equal lengths is planned on its own."""
        if len(prompt_lens) != len(rows):
            raise ValueError(f"{len(prompt_lens)} prompt lengths for {len(rows)} batches")
        plan: List[List[int]] = []
        i = 0
        while i < len(rows):
            j = i
            while j < len(rows) and prompt_lens[j] == prompt_lens[i]:
                j += 1
            plan += [[i + k for k in g] for g in cls.coalesce_plan(list(rows[i:j]), n_engines, max_rows)]
            i = j
        return plan

    @staticmethod
    def merge_prompts(plan: Sequence[Sequence[int]], rows: Sequence[int], prompts: Sequence[torch.Tensor]) -> List[torch.Tensor]:
        """The prompt of every merged pass of `plan`: prompts[j] is batch j's validated [1, P] or [rows[j], P] tensor.  A pass whose
        batches all carry the same single row keeps that one row; otherwise every batch's prompt is expanded to its rows and the rows
        are concatenated in plan order - the order the frames are concatenated in."""
        out = []
        for g in plan:
            ps = [prompts[j] for j in g]
            if len({int(p.shape[1]) for p in ps}) != 1:
                raise ValueError(f"batches {list(g)} of one pass have prompts of different lengths {[int(p.shape[1]) for p in ps]}")
            if all(p.shape[0] == 1 and torch.equal(p, ps[0]) for p in ps):
                out.append(ps[0])
            else:
                out.append(torch.cat([p.expand(rows[j], p.shape[1]) if p.shape[0] == 1 else p for j, p in zip(g, ps)], dim=0).contiguous())
        return out

    @staticmethod
    def _per_batch_prompts(prompt_ids, n_batches: int) -> list:
        """One shared prompt - a TENSOR / array ([P] or [1, P]) or a FLAT list of ints - -> the same object for every batch.  A list /
        tuple whose elements are not ints is ALWAYS read as one prompt per batch (each [P], [1, P] or that batch's [rows, P]) and its
        length must be the number of batches: a shared prompt is never written as a nested list, and rows of one [B, P] prompt
        cannot span batches (every batch brings its own rows)."""
        if isinstance(prompt_ids, (list, tuple)) and len(prompt_ids) and not isinstance(prompt_ids[0], numbers.Integral):
            if len(prompt_ids) != n_batches:
                raise ValueError(f"prompt_ids is a list of {len(prompt_ids)} prompts for {n_batches} batches: a list of prompts is read "
                                 f"as one prompt per batch; give one shared prompt as a flat list of ints or a tensor, or one prompt "
                                 f"per batch")
            return list(prompt_ids)
        return [prompt_ids] * n_batches

    @classmethod
    def split_merged_outputs(cls, plan: Sequence[Sequence[int]], rows: Sequence[int], outs_m: Sequence[dict]) -> list:
        """The outputs of the merged passes of `plan` (one dict per pass, every value with the pass's rows leading) cut back into one
        dict per original batch; rows[j] = rows of batch j."""
        outs: list = [None] * len(rows)
        for g, om in zip(plan, outs_m):
            unknown = sorted(set(om) - set(cls._PER_ROW_OUTPUTS))
            if unknown:              # a new output key must say here whether it is per row - never guessed from its shape
                raise N.CaptionerHipError(f"generate_many(coalesce_rows=): output(s) {unknown} are not in the list of per-row "
                                          f"outputs {cls._PER_ROW_OUTPUTS}; cannot split a merged pass")
            r0 = 0
            for j in g:
                outs[j] = {k: v[r0:r0 + rows[j]] for k, v in om.items()}
                r0 += rows[j]
        return outs

    def generate_many(self, batches, threads: bool = False, coalesce_rows: int = 0, **generate_kw):
        """prompt_ids= (BLIP): one shared prompt as a flat list of ints or a tensor, or a list with one prompt per batch
        (`_per_batch_prompts`); batches merge into a pass only when their prompt lengths agree.
        All batches, in order.  threads=True: one host thread per engine (batch j goes to engine j % n) - needed when
        the engines poll for early exit (cap_set_early_exit synchronises its stream: from a single host thread that would
        stall the launches of the other streams; ctypes releases the GIL during cap_generate, so the threads do overlap).
        coalesce_rows > 0: dynamic batching - consecutive batches of the same frame shape are concatenated into passes of at most
        that many rows (`coalesce_plan`; the engines must have been built with max_batch >= coalesce_rows) and the outputs split
        back per batch.  A frame decodes to the same bits alone, in its own batch and in a merged pass (batch invariance,
        DESIGN.md section 2), so the results are those of the uncoalesced call; what changes is that the decode chain's fixed
        costs are paid once per pass: 256-frame batches on 3 engines 6 010 captions/s, merged to 1024 rows 6 600 (round 6)."""
        batches = list(batches)
        self.last_coalesce = None            # what the last call did with coalesce_rows: the plan, or why it was not applied
        prompts = None
        if generate_kw.get("prompt_ids") is not None:
            # one shared prompt or one prompt per batch; validated here on the host, once, against the batch it belongs to
            e0 = self.engines[0]
            L = generate_kw.get("max_length") or e0.max_len
            given = self._per_batch_prompts(generate_kw.pop("prompt_ids"), len(batches))
            prompts = [validate_prompt_ids(p, e0.arch, int(b.shape[0]), L, generate_kw.get("num_beams", 1),
                                           generate_kw.get("num_beam_groups"), min(e.prompt_limit for e in self.engines))
                       for p, b in zip(given, batches)]
        else:
            generate_kw.pop("prompt_ids", None)
        # sampling: every batch's keys are fixed HERE, before any plan - from the pool's own counter, or the caller's list with one
        # tensor per batch - and travel with the batch, so the pooled and the merged results are a lone call's bits
        keys = None
        nret = int(generate_kw.get("num_return_sequences") or 1)
        if getattr(self.engines[0], "do_sample", False):
            given = generate_kw.pop("sample_keys", None)
            if given is None:
                keys = self.batch_sample_keys([int(b.shape[0]) * nret for b in batches])
            else:
                if not isinstance(given, (list, tuple)) or len(given) != len(batches):
                    raise ValueError(f"sample_keys must be a list with one key tensor per batch ({len(batches)} batches)")
                keys = [keys_tensor(k, int(b.shape[0]) * nret) for k, b in zip(given, batches)]
        if coalesce_rows and len(batches) > 1:
            same = all(b.shape[1:] == batches[0].shape[1:] and b.dtype == batches[0].dtype and b.device == batches[0].device for b in batches)
            cap_rows = min(coalesce_rows, min(e.max_batch for e in self.engines))
            if generate_kw.get("output_logits"):
                self.last_coalesce = "not applied: per-step logits are recorded per pass"
            elif not same:
                self.last_coalesce = "not applied: the batches differ in frame shape, dtype or device"
            else:
                rows = [int(b.shape[0]) for b in batches]
                if nret > 1:
                    raise ValueError("generate_many: coalesce_rows with num_return_sequences > 1 is not built (an image's captions are "
                                     "rows of its own batch); expand the image state and pass sample_keys instead")
                plan = (self.coalesce_plan(rows, len(self.engines), cap_rows) if prompts is None else
                        self.coalesce_plan_prompted(rows, len(self.engines), cap_rows, [int(p.shape[1]) for p in prompts]))
                if any(len(g) > 1 for g in plan):
                    merged = [batches[g[0]] if len(g) == 1 else torch.cat([batches[j] for j in g], dim=0) for g in plan]
                    if prompts is not None:
                        generate_kw = dict(generate_kw, prompt_ids=self.merge_prompts(plan, rows, prompts))
                    if keys is not None:     # concatenated in plan order, as the frames are
                        generate_kw = dict(generate_kw, sample_keys=[torch.cat([keys[j] for j in g]) for g in plan])
                    outs_m = self.generate_many(merged, threads=threads, **generate_kw)
                    self.last_coalesce = plan            # (the inner call cleared it)
                    return self.split_merged_outputs(plan, [int(b.shape[0]) for b in batches], outs_m)
                self.last_coalesce = f"not applied: {len(batches)} batches on {len(self.engines)} engines leave nothing to merge within {cap_rows} rows"
            logger.debug("generate_many(coalesce_rows=%d) %s", coalesce_rows, self.last_coalesce)
        def kw_of(j):
            kw = generate_kw if prompts is None else dict(generate_kw, prompt_ids=prompts[j])
            return kw if keys is None else dict(kw, sample_keys=keys[j])
        if not threads or len(self.engines) == 1 or len(batches) <= 1:
            outs = [self.submit(b, **kw_of(j)) for j, b in enumerate(batches)]
            self.join()
            return outs
        import threading
        n = len(self.engines)
        outs: list = [None] * len(batches)
        errors: list = []
        cur = torch.cuda.current_stream(self.device)
        for s in self.streams:
            s.wait_stream(cur)

        def work(i):
            try:
                with torch.cuda.device(self.device), torch.cuda.stream(self.streams[i]):
                    for j in range(i, len(batches), n):
                        outs[j] = self.engines[i].generate(batches[j], **kw_of(j))
                        if batches[j].is_cuda:
                            batches[j].record_stream(self.streams[i])
            except Exception as e:  # noqa: BLE001 - re-raised on the caller's thread
                errors.append(e)

        ts = [threading.Thread(target=work, args=(i,)) for i in range(min(n, len(batches)))]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        if errors:
            raise errors[0]
        self.join()
        self._next = len(batches) % n
        return outs


class TextEncoderEngine(_Engine):
    """Sentence encoder replica (CAP_ARCH_MINILM handle): WordPiece ids + lengths -> L2-normalised mean-pooled embeddings.
    Replaces `SentenceTransformer("all-MiniLM-L6-v2").encode(...)` (reference goal_exploration.py:57,102;
    pseudolabeler.py:568,677); tokenisation stays on the host (captioner/sentence_encoder.py)."""

    def __init__(self, arch: MiniLMArch, dtype: str = "bf16", max_batch: int = 64, max_len: int = 32,
                 device: str | torch.device = "cuda:0", share_weights_with: "TextEncoderEngine | None" = None):
        super().__init__(arch, dtype, max_batch, max_len, device)
        cfg = self._config(2)
        # a lone encoder: its arch names the dimensions without the t_ of `_text_tower`
        cfg.t_hidden, cfg.t_layers, cfg.t_heads, cfg.t_ffn = arch.hidden, arch.layers, arch.heads, arch.ffn
        cfg.vocab, cfg.max_pos, cfg.t_eps = arch.vocab, arch.max_pos, arch.eps
        self._create(cfg, share_weights_with)

    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True) -> Dict[str, object]:
        """HF BertModel names; a leading `0.auto_model.` / `bert.` prefix (sentence-transformers / BertFor* saves) is dropped."""
        clean = {}
        for k, v in sd.items():
            for pre in ("0.auto_model.", "auto_model.", "bert."):
                if k.startswith(pre):
                    k = k[len(pre):]
            clean[k] = v
        return self._stream_weights(clean, strict)

    def embed(self, ids: torch.Tensor, lens: torch.Tensor) -> torch.Tensor:
        """ids int [B, L] (pad anywhere after `lens[b]` tokens), lens int [B] -> fp32 [B, hidden] on the device."""
        ids, lens, B, L = self._ids_lens(ids, lens)
        out = torch.empty((B, self.arch.hidden), dtype=torch.float32, device=self.device)
        self._call("cap_embed_text", ids, lens, B, L, out)
        return out


class ClipEngine(_Engine):
    """CLIP scorer replica (CAP_ARCH_CLIP handle): both towers and the image-caption logits of HF `CLIPModel`, as the
    reference's `--method clip` uses it (experimenting_env/captioner/pseudocaptioner.py:39-46, :352-357).  Embeddings come
    back L2-normalised, fp32 [B, projection_dim]; tokenisation stays on the host (captioner/clip_scorer.py)."""

    def __init__(self, arch: ClipArch, dtype: str = "f32s", max_batch: int = 256, max_len: Optional[int] = None,
                 device: str | torch.device = "cuda:0", share_weights_with: "ClipEngine | None" = None):
        super().__init__(arch, dtype, max_batch, max_len or arch.max_pos, device)
        cfg = self._config(N.CAP_ARCH_CLIP)
        self._vision_tower(cfg, arch.eps)
        self._text_tower(cfg, arch.max_pos, arch.eps, (arch.bos_token_id, arch.eos_token_id, arch.pad_token_id))
        cfg.embed_dim = arch.projection_dim
        cfg.hidden_act = N.CAP_ACT_GELU if arch.hidden_act == "gelu" else N.CAP_ACT_QUICK_GELU
        self.logit_scale = share_weights_with.logit_scale if share_weights_with is not None else None
        self._create(cfg, share_weights_with)

    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True) -> Dict[str, object]:
        """HF `CLIPModel` names (wrapper prefixes dropped, `*.position_ids` buffers and the absent patch bias ignored)."""
        from .weights import strip_wrapper_prefixes
        sd = {k: v for k, v in strip_wrapper_prefixes(sd).items()
              if not k.endswith("position_ids") and k != "vision_model.embeddings.patch_embedding.bias"}
        rep = self._stream_weights(sd, strict)
        v = C.c_float()
        with torch.cuda.device(self.device):
            if self.lib.cap_clip_logit_scale(self._h, C.byref(v)) == 0:
                self.logit_scale = float(v.value)
        return rep

    def embed_images(self, pixels: torch.Tensor) -> torch.Tensor:
        """uint8 [B, S, S, 3] RGB or normalised fp32 [B, 3, S, S] -> fp32 [B, projection_dim] (device), L2-normalised."""
        pixels, fmt = self._pixels(pixels)
        B = pixels.shape[0]
        if not 1 <= B <= self.max_batch:
            raise ValueError(f"batch of {B} images outside 1..{self.max_batch} (the engine's max_batch)")
        out = torch.empty((B, self.arch.projection_dim), dtype=torch.float32, device=self.device)
        self._call("cap_clip_embed_images", pixels, fmt, B, out)
        return out

    def embed_text(self, ids: torch.Tensor, lens: torch.Tensor) -> torch.Tensor:
        """ids int [B, L] (right padded; anything after the caption), lens int [B] = tokens up to and including the pooled EOT
        -> fp32 [B, projection_dim] (device), L2-normalised."""
        B, L = _ids_shape(ids, lens)
        if not 1 <= L <= self.max_len:
            raise ValueError(f"{L} tokens per caption outside 1..{self.max_len} (the engine's max_len)")
        if not 1 <= B <= self.max_batch:
            raise ValueError(f"batch of {B} captions outside 1..{self.max_batch} (the engine's max_batch)")
        ids, lens, B, L = self._ids_lens(ids, lens)
        out = torch.empty((B, self.arch.projection_dim), dtype=torch.float32, device=self.device)
        self._call("cap_clip_embed_text", ids, lens, B, L, out)
        return out

    def logits(self, img: torch.Tensor, txt: torch.Tensor, paired: bool = True) -> torch.Tensor:
        """exp(logit_scale) * img . txt^T of normalised embeddings: paired -> [n] (image i against caption i), else
        [Ni, Nt] (HF's logits_per_image)."""
        if self.logit_scale is None:
            raise N.CaptionerHipError("no weights loaded: logit_scale unknown")
        P = self.arch.projection_dim
        if img.dim() != 2 or txt.dim() != 2 or img.shape[1] != P or txt.shape[1] != P:
            raise ValueError(f"embeddings must be [n, {P}], got {tuple(img.shape)} / {tuple(txt.shape)}")
        if paired and img.shape[0] != txt.shape[0]:
            raise ValueError(f"paired logits need as many images as captions ({img.shape[0]} / {txt.shape[0]})")
        img = img.to(self.device, torch.float32).contiguous()
        txt = txt.to(self.device, torch.float32).contiguous()
        Ni, Nt = img.shape[0], txt.shape[0]
        out = torch.empty((Ni,) if paired else (Ni, Nt), dtype=torch.float32, device=self.device)
        _launch(self.lib, self.device, "cap_clip_logits", img, txt, Ni, Nt, int(bool(paired)), C.c_float(self.logit_scale), out, P)
        return out


class Blip2ItmEngine(_Engine):
    """BLIP-2 image-text scorer replica (CAP_ARCH_BLIP2_ITM handle): HF `Blip2ForImageTextRetrieval`'s two scores for batches of
    (image, caption) pairs, as the reference's `--method blip2_itm | blip2_itc` computes them one pair per call
    (experimenting_env/captioner/pseudocaptioner.py:193-308).  `encode_images` leaves an image batch's tokens and cross-attention
    K/V resident in the handle; `itc_image_features` and `itm` then read them without running the ViT-g again.  Tokenisation stays
    on the host (captioner/blip2_itm_scorer.py)."""

    def __init__(self, arch: Blip2ItmArch, dtype: str = "f32s", max_batch: int = 256, max_len: Optional[int] = None,
                 device: str | torch.device = "cuda:0", share_weights_with: "Blip2ItmEngine | None" = None):
        super().__init__(arch, dtype, max_batch, max_len or arch.max_text_len, device)
        cfg = self._config(N.CAP_ARCH_BLIP2_ITM)
        self._vision_tower(cfg, arch.v_eps)
        self._qformer(cfg)
        cfg.vocab, cfg.max_pos, cfg.pad = arch.vocab, arch.max_pos, arch.pad         # the text side is the Q-Former's: no tower of its own
        cfg.embed_dim = arch.projection_dim
        self.resident = 0            # images of the last encode_images
        self._create(cfg, share_weights_with)

    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True) -> Dict[str, object]:
        """HF `Blip2ForImageTextRetrieval` names (wrapper prefixes dropped, `*.position_ids` buffers ignored);
        `derived.qformer_x0` = qformer.layernorm(query_tokens) is computed here."""
        from .weights import strip_wrapper_prefixes
        sd = {k: v for k, v in strip_wrapper_prefixes(sd).items() if not k.endswith("position_ids")}
        with _deriving_tensors():
            sd = _with_qformer_x0(sd, self.arch.q_eps)
        return self._stream_weights(sd, strict)

    def encode_images(self, pixels: torch.Tensor) -> int:
        """uint8 [B, S, S, 3] RGB or normalised fp32 [B, 3, S, S]: runs the ViT-g and the cross K/V projections; the batch stays
        resident for `itc_image_features` / `itm`.  Returns B."""
        pixels, fmt = self._pixels(pixels)
        B = pixels.shape[0]
        self.resident = 0
        self._call("cap_blip2_itm_encode_images", pixels, fmt, B)
        self.resident = B
        return B

    def itc_image_features(self) -> torch.Tensor:
        """The resident images -> fp32 [B, num_query_tokens, projection_dim] (device), each query row L2-normalised."""
        B = self.resident
        out = torch.empty((B, self.arch.num_query_tokens, self.arch.projection_dim), dtype=torch.float32, device=self.device)
        self._call("cap_blip2_itc_image_features", B, out)
        return out

    def itc_text_features(self, ids: torch.Tensor, lens: torch.Tensor) -> torch.Tensor:
        """ids int [B, L] (right padded; anything after the caption), lens int [B] -> fp32 [B, projection_dim] (device), L2-normalised."""
        ids, lens, B, L = self._ids_lens(ids, lens)
        out = torch.empty((B, self.arch.projection_dim), dtype=torch.float32, device=self.device)
        self._call("cap_blip2_itc_text_features", ids, lens, B, L, out)
        return out

    def itc_scores(self, img: torch.Tensor, txt: torch.Tensor, paired: bool = True) -> torch.Tensor:
        """max over the queries of img [Ni, nq, P] . txt [Nt, P]: paired -> [n] (image i against caption i), else [Ni, Nt]."""
        nq, P = self.arch.num_query_tokens, self.arch.projection_dim
        if img.dim() != 3 or txt.dim() != 2 or tuple(img.shape[1:]) != (nq, P) or txt.shape[1] != P:
            raise ValueError(f"features must be [n, {nq}, {P}] and [n, {P}], got {tuple(img.shape)} / {tuple(txt.shape)}")
        if paired and img.shape[0] != txt.shape[0]:
            raise ValueError(f"paired scores need as many images as captions ({img.shape[0]} / {txt.shape[0]})")
        img = img.to(self.device, torch.float32).contiguous()
        txt = txt.to(self.device, torch.float32).contiguous()
        Ni, Nt = img.shape[0], txt.shape[0]
        out = torch.empty((Ni,) if paired else (Ni, Nt), dtype=torch.float32, device=self.device)
        _launch(self.lib, self.device, "cap_blip2_itc_scores", img, txt, Ni, Nt, int(bool(paired)), out, nq, P)
        return out

    def itm(self, ids: torch.Tensor, lens: torch.Tensor):
        """Resident image b against caption b -> (logits fp32 [B, 2], probability of a match fp32 [B]) on the device."""
        ids, lens, B, L = self._ids_lens(ids, lens)
        logits = torch.empty((B, 2), dtype=torch.float32, device=self.device)
        prob = torch.empty((B,), dtype=torch.float32, device=self.device)
        self._call("cap_blip2_itm_logits", ids, lens, B, L, logits, prob)
        return logits, prob
