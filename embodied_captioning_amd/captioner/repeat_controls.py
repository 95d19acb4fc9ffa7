"""Repetition controls of the decode loops: HF ``generate(repetition_penalty=, no_repeat_ngram_size=)`` on the device
(``cap_set_repeat_controls``).  This module is the host side and needs no GPU.

* ``validate_repeat_controls(repetition_penalty, no_repeat_ngram_size, arch, max_len)`` - the host check of the two numbers, naming
  what is wrong; returns them as ``(float, int)``.  ``None`` stands for the neutral value (1.0 / 0).
* ``resolve_repeat_controls(cfg, arch, max_len)`` - the wrappers' configuration keys, validated before an engine exists.
* ``reject_ngram_key(cfg, who)`` - CoCa's refusal of ``captioner.no_repeat_ngram_size`` (its ``repetition_penalty`` key is judged by
  ``reject_unsupported_generation_options``, as it always was).

The context the two processors see is HF's: BLIP's BOS, prompt and generated tokens; BLIP-2's image placeholders, BOS and generated
tokens (so a penalty lowers BLIP-2's BOS and placeholder scores from the first step on; where BOS and EOS are one id, EOS too).
"""
from __future__ import annotations

import math
import numbers
from typing import Optional, Tuple


def _family(arch) -> str:
    from ..config import Blip2Arch, CocaArch
    return "coca" if isinstance(arch, CocaArch) else "blip2" if isinstance(arch, Blip2Arch) else "blip"


def context_prefix(arch) -> int:
    """Tokens HF's processors see in front of a caption's first column: BLIP-2's image placeholders and BOS; none for BLIP (its BOS
    is the caption's first column)."""
    return arch.num_query_tokens + 1 if _family(arch) == "blip2" else 0


def validate_repeat_controls(repetition_penalty, no_repeat_ngram_size, arch, max_len: Optional[int] = None) -> Tuple[float, int]:
    """The host check of the two controls -> (penalty, size) as the library is given them.  Raises ValueError naming the fault: a
    penalty that is not a finite number above 0, a size that is not an integer >= 0 or that exceeds max_len plus the context prefix,
    and - for either control away from its neutral value - a CoCa architecture."""
    p = 1.0 if repetition_penalty is None else repetition_penalty
    n = 0 if no_repeat_ngram_size is None else no_repeat_ngram_size
    if isinstance(p, bool) or not isinstance(p, numbers.Real) or not math.isfinite(p) or not p > 0:
        raise ValueError(f"repetition_penalty must be a finite number above 0 (1.0 = off), got {repetition_penalty!r}")
    if isinstance(n, bool) or not hasattr(n, "__index__") or int(n) < 0:
        raise ValueError(f"no_repeat_ngram_size must be an integer >= 0 (0 = off), got {no_repeat_ngram_size!r}")
    p, n = float(p), int(n)
    if max_len is not None and n > int(max_len) + context_prefix(arch):
        raise ValueError(f"no_repeat_ngram_size = {n} is beyond the {int(max_len) + context_prefix(arch)} tokens a caption can hold "
                         f"(max_len {int(max_len)} + a prefix of {context_prefix(arch)})")
    if (p != 1.0 or n > 0) and _family(arch) == "coca":
        raise ValueError("repetition_penalty / no_repeat_ngram_size: not built for CoCa (its decode loop - MinLength, forced EOS, a pad "
                         "that ends the row - does not apply them); BLIP and BLIP-2 only")
    return p, n


def resolve_repeat_controls(cfg, arch, max_len: Optional[int] = None) -> Tuple[float, int]:
    """captioner.repetition_penalty / captioner.no_repeat_ngram_size -> (penalty, size), validated; absent keys are neutral."""
    try:
        return validate_repeat_controls(getattr(cfg, "repetition_penalty", None), getattr(cfg, "no_repeat_ngram_size", None), arch, max_len)
    except ValueError as e:
        raise ValueError(f"captioner.{e}") from None


def reject_ngram_key(cfg, who: str) -> None:
    """`captioner.no_repeat_ngram_size` is BLIP's and BLIP-2's: a CoCa wrapper that finds it raises, naming it."""
    n = getattr(cfg, "no_repeat_ngram_size", None)
    if n is not None and n != 0:
        raise ValueError(f"{who}: captioner.no_repeat_ngram_size = {n!r} - the n-gram control is implemented for arch_name 'blip' and "
                         f"'blip2' only (the reference's CoCa.generate has no such option)")
