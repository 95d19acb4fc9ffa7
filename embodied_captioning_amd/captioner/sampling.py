"""Sampling in the greedy decode loop: HF ``generate(do_sample=True, temperature=, top_k=, top_p=)`` on the device
(``cap_set_sampling``).  This module is the host side and needs no GPU.

* ``validate_sampling(do_sample, temperature, top_k, top_p, seed, arch)`` - the host check, naming what is wrong; returns
  ``(bool, float, int, float, int)`` with the two floats as the fp32 numbers the kernels use.  ``None`` stands for the neutral value.
* ``resolve_sampling(cfg, arch, max_batch)`` - the wrappers' configuration keys (``captioner.do_sample``, ``temperature``, ``top_k``,
  ``top_p``, ``sample_seed``, ``num_return_sequences``), validated before an engine exists.
* ``default_sample_keys`` / ``return_sequence_keys`` - the per-caption keys of a call: ``(call_no << 32) | row``.

The distribution, step by step, is stated in ``include/captioner_hip.h`` (cap_set_sampling) and INTEGRATION.md section 6g.
"""
from __future__ import annotations

import ctypes
import math
import numbers
from typing import Optional, Tuple

import numpy as np


def _family(arch) -> str:
    from ..config import Blip2Arch, CocaArch
    return "coca" if isinstance(arch, CocaArch) else "blip2" if isinstance(arch, Blip2Arch) else "blip"


def _f32(v: float) -> float:
    return float(ctypes.c_float(v).value)


def validate_sampling(do_sample=None, temperature=None, top_k=None, top_p=None, seed=None, arch=None) -> Tuple[bool, float, int, float, int]:
    """The host check of the sampling state -> (do_sample, temperature, top_k, top_p, seed) as the library is given them.  Raises
    ValueError naming the fault: a temperature that is not a finite number above 0, a top_k that is not an integer >= 0, a top_p
    outside (0, 1], a seed outside [0, 2^64), and - with do_sample - a CoCa architecture."""
    on = bool(do_sample) if do_sample is not None else False
    t = 1.0 if temperature is None else temperature
    k = 0 if top_k is None else top_k
    p = 1.0 if top_p is None else top_p
    s = 0 if seed is None else seed
    if isinstance(t, bool) or not isinstance(t, numbers.Real) or not math.isfinite(t) or not t > 0 or not _f32(t) > 0 or not math.isfinite(_f32(t)):
        raise ValueError(f"temperature must be a finite number above 0 (1.0 = neutral), got {temperature!r}")
    if isinstance(k, bool) or not hasattr(k, "__index__") or int(k) < 0 or int(k) >= 2 ** 31:
        raise ValueError(f"top_k must be an integer >= 0 (0 = off), got {top_k!r}")
    if isinstance(p, bool) or not isinstance(p, numbers.Real) or not (p > 0 and p <= 1) or not _f32(p) > 0:
        raise ValueError(f"top_p must be a number in (0, 1] (1.0 = off), got {top_p!r}")
    if isinstance(s, bool) or not hasattr(s, "__index__") or not 0 <= int(s) < 2 ** 64:
        raise ValueError(f"seed must be an integer in [0, 2^64), got {seed!r}")
    if on and arch is not None and _family(arch) == "coca":
        raise ValueError("do_sample: sampling is not built for CoCa (the reference's CoCa sampling loop - generation_type 'top_p' / 'top_k', "
                         "coca_model.py:266-275 - is out of scope); BLIP and BLIP-2 only")
    return on, _f32(t), int(k), _f32(p), int(s)


def reject_sampling_keys(cfg, who: str) -> None:
    """`captioner.do_sample` / `sample_seed` / `num_return_sequences` are BLIP's and BLIP-2's: a CoCa wrapper that finds one raises,
    naming it (its temperature / top_k / top_p keys are judged by `reject_unsupported_generation_options`, as they always were)."""
    given = [k for k, neutral in (("do_sample", (None, False)), ("sample_seed", (None,)), ("num_return_sequences", (None, 1)))
             if getattr(cfg, k, None) not in neutral]
    if given:
        raise ValueError(f"{who}: captioner.{' / captioner.'.join(given)} - sampling is implemented for arch_name 'blip' and 'blip2' only "
                         f"(CoCa's own sampling loop, coca_model.py:266-275, is not built)")


def resolve_sampling(cfg, arch, max_batch: Optional[int] = None, num_beams: int = 1, who: str = "captioner") -> Tuple[bool, float, int, float, int, int]:
    """captioner.do_sample / temperature / top_k / top_p / sample_seed / num_return_sequences -> (do_sample, temperature, top_k, top_p,
    seed, num_return_sequences), validated.  With do_sample false (or absent) temperature / top_k / top_p are accepted at their
    neutral values and refused by name otherwise (`reject_unsupported_generation_options`' judgement), never ignored."""
    n = getattr(cfg, "num_return_sequences", None)
    n = 1 if n is None else n
    if isinstance(n, bool) or not hasattr(n, "__index__") or int(n) < 1:
        raise ValueError(f"captioner.num_return_sequences must be an integer >= 1, got {n!r}")
    n = int(n)
    if not getattr(cfg, "do_sample", None):
        if n != 1:
            raise ValueError(f"captioner.num_return_sequences = {n} needs captioner.do_sample: the arg-max loop returns one caption per image")
        if getattr(cfg, "sample_seed", None) not in (None, 0):
            raise ValueError("captioner.sample_seed is given without captioner.do_sample")
        from .generation_options import reject_unsupported_generation_options
        reject_unsupported_generation_options({k: getattr(cfg, k) for k in ("temperature", "top_k", "top_p")
                                               if getattr(cfg, k, None) is not None}, who)
        return False, 1.0, 0, 1.0, 0, 1
    if int(num_beams or 1) > 1:
        raise ValueError(f"{who}: captioner.do_sample with captioner.num_beams = {num_beams}: beam sampling is not built (num_beams = 1 only)")
    try:
        on, t, k, p, s = validate_sampling(True, getattr(cfg, "temperature", None), getattr(cfg, "top_k", None), getattr(cfg, "top_p", None),
                                           getattr(cfg, "sample_seed", None), arch)
    except ValueError as e:
        raise ValueError(f"captioner.{e}") from None
    if max_batch is not None and n > int(max_batch):
        raise ValueError(f"captioner.num_return_sequences = {n} exceeds batch_size = {int(max_batch)}: one image's captions are rows of one call")
    return on, t, k, p, s, n


def default_sample_keys(call_no: int, n_rows: int, first: int = 0) -> np.ndarray:
    """The keys of a call's captions: (call_no << 32) | (first + row), uint64 [n_rows].  The low word is the caption's place in the
    CALL, the high word the call's number since `set_sampling`: repeated calls differ and are reproducible."""
    if not 0 <= int(call_no) < 2 ** 32 or first < 0 or first + n_rows > 2 ** 32:
        raise ValueError(f"sample keys: call number {call_no} or rows {first}..{first + n_rows} do not fit 32 bits each")
    return (np.uint64(int(call_no)) << np.uint64(32)) | np.arange(first, first + n_rows, dtype=np.uint64)


def return_sequence_keys(call_no: int, n_images: int, n: int) -> np.ndarray:
    """num_return_sequences = n: caption r of image b has key (call_no << 32) | (b * n + r); image-major, HF's order."""
    return default_sample_keys(call_no, n_images * n)


def keys_tensor(sample_keys, n_rows: int):
    """sample_keys as given (an int64 / uint64 tensor, array or list [n_rows]) -> a host int64 tensor holding the 64 bits."""
    import torch
    if isinstance(sample_keys, torch.Tensor):
        k = sample_keys.detach().cpu()
        if k.dtype not in (torch.int64, torch.uint64):
            raise ValueError(f"sample_keys must be an int64 tensor [{n_rows}], got {k.dtype}")
        k = k.view(torch.int64) if k.dtype != torch.int64 else k
    else:
        a = np.asarray(sample_keys)
        if a.dtype.kind not in "iu":
            raise ValueError(f"sample_keys must hold integers, got {a.dtype}")
        k = torch.from_numpy(np.ascontiguousarray(a.astype(np.uint64) if a.dtype.kind == "u" else a.astype(np.int64)).view(np.int64))
    if k.dim() != 1 or int(k.shape[0]) != int(n_rows):
        raise ValueError(f"sample_keys must have one key per caption: shape [{n_rows}], got {tuple(k.shape)}")
    return k.contiguous()
