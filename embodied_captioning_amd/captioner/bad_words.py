"""Banned words for the decode loops: HF ``generate(bad_words_ids=...)`` on the device (``cap_set_bad_words``).

The reference throws away every caption that contains one of its banned words (``pseudocaptioner.py:96-123``, mirrored here as
``distributed.BANNED_WORDS`` / ``filter_caption``).  Constrained decoding keeps the caption instead: the captioner never emits the
banned token sequences and writes its next-best caption.  This module is the host side, and needs no GPU and no tokenizer package:

* ``validate_bad_words_ids(seqs, arch)`` - the host check of a list of token-id sequences, naming what is wrong;
* ``bad_word_sequences(words, vocab, encode, mode)`` - banned WORDS to token-id sequences, given a vocabulary and an encoder.

Neither mode of ``bad_word_sequences`` can promise that ``filter_caption`` passes: the reference's rule is a substring test on the
decoded caption, and sub-word pieces can combine across a boundary into a banned word that no single banned sequence spells
("pic" + "ture" when only the whole-word piece is banned; a word split differently behind another prefix).  ``BatchedBoxCaptioner``
therefore still filters, and reports how many captions of a call fail.
"""
from __future__ import annotations

from typing import Callable, Iterable, List, Mapping, Sequence

BAN_MAX_MULTI = 1024      # multi-token sequences a handle takes (single tokens are unbounded)
BAN_MAX_LEN = 8           # tokens of one sequence


def _family(arch) -> str:
    from ..config import Blip2Arch, CocaArch
    return "coca" if isinstance(arch, CocaArch) else "blip2" if isinstance(arch, Blip2Arch) else "blip"


def validate_bad_words_ids(seqs, arch) -> List[List[int]]:
    """The host check of ``bad_words_ids``: a list of token-id sequences -> the list of int lists the library is given (``[eos]``
    alone dropped silently, as HF drops it).  None or an empty list is the empty set.  Raises ValueError naming the fault: a CoCa
    architecture, something that is not a list of lists of ints, an empty sequence, an id outside [0, vocab), the BOS / pad id or
    (BLIP-2) the image placeholder id - context only, never generated - more than 1024 multi-token sequences, one longer than 8."""
    if seqs is None:
        return []
    if isinstance(seqs, (str, bytes)) or not isinstance(seqs, Iterable):
        raise ValueError(f"bad_words_ids must be a list of token-id lists, got {type(seqs).__name__}")
    seqs = list(seqs)
    if not seqs:
        return []
    if _family(arch) == "coca":
        raise ValueError("bad_words_ids: not built for CoCa (the reference's CoCa.generate has no such option); BLIP and BLIP-2 only")
    out: List[List[int]] = []
    n_multi = 0
    special = [("BOS", arch.bos), ("pad", arch.pad)]
    if _family(arch) == "blip2":
        special.append(("image placeholder", arch.image_token))
    for q, seq in enumerate(seqs):
        if isinstance(seq, (str, bytes)) or not isinstance(seq, Iterable):
            raise ValueError(f"bad_words_ids[{q}] must be a list of token ids, got {seq!r}")
        seq = list(seq)
        if not seq:
            raise ValueError(f"bad_words_ids[{q}] is an empty sequence")
        ids = []
        for t in seq:
            if isinstance(t, bool) or not hasattr(t, "__index__"):
                raise ValueError(f"bad_words_ids[{q}] holds {t!r}: token ids are integers")
            t = int(t)
            if t < 0 or t >= arch.vocab:
                raise ValueError(f"bad_words_ids[{q}] holds token id {t}, out of range [0, {arch.vocab}) of the vocabulary")
            for name, tid in special:
                if t == tid:
                    raise ValueError(f"bad_words_ids[{q}] holds the {name} token ({tid}): it is context only and is never generated")
            ids.append(t)
        if ids == [arch.eos]:
            continue
        if len(ids) > BAN_MAX_LEN:
            raise ValueError(f"bad_words_ids[{q}] has {len(ids)} tokens: a banned sequence has at most {BAN_MAX_LEN}")
        if len(ids) > 1:
            n_multi += 1
            if n_multi > BAN_MAX_MULTI:
                raise ValueError(f"bad_words_ids holds more than {BAN_MAX_MULTI} multi-token sequences (single tokens are unbounded)")
        out.append(ids)
    return out


def _surface(piece: str) -> str:
    """A vocabulary entry as it shows in a decoded caption: without WordPiece's `##` / byte-level BPE's `Ġ` marker, lower-cased."""
    if piece.startswith("##"):
        piece = piece[2:]
    return piece.replace("Ġ", "").lower()


def bad_word_sequences(words: Sequence[str], vocab: Mapping[str, int], encode: Callable[[str], List[int]], mode: str = "word") -> List[List[int]]:
    """Banned words -> token-id sequences for ``bad_words_ids``.

    vocab: piece -> id; encode: text -> ids WITHOUT special tokens (a tokenizer's `encode(text, add_special_tokens=False)`).
    mode "word": the tokenisation of each word, as one sequence.  A byte-level BPE vocabulary (one that has `Ġ` pieces) tokenises a
    word differently behind a space, so both forms - `" word"` and `"word"` - are included.
    mode "substring": that, plus as single tokens every vocabulary entry whose surface (no `##` / `Ġ`, lower-cased) contains a banned
    word - the reference's `word in caption.lower()` rule applied to the vocabulary.
    Sequences come out deduplicated, in a fixed order (words as given, then vocabulary ids ascending).  See the module docstring for
    what neither mode can promise."""
    if mode not in ("word", "substring"):
        raise ValueError(f"bad_word_sequences: mode must be 'word' or 'substring', got {mode!r}")
    byte_level = any(p.startswith("Ġ") for p in vocab)
    seen, out = set(), []

    def add(ids):
        ids = [int(i) for i in ids]
        if ids and tuple(ids) not in seen:
            seen.add(tuple(ids))
            out.append(ids)

    lowered = []
    for w in words:
        w = str(w).strip().lower()
        if not w:
            raise ValueError("bad_word_sequences: an empty word")
        lowered.append(w)
        if byte_level:
            add(encode(" " + w))
        add(encode(w))
    if mode == "substring":
        for piece, tid in sorted(vocab.items(), key=lambda kv: kv[1]):
            s = _surface(piece)
            if s and any(w in s for w in lowered):
                add([tid])
    return out


def resolve_bad_words(cfg, tokenizer, arch):
    """The wrappers' configuration keys -> the sequences for `CaptionerEngine.set_bad_words`, or None when neither key is given.
    captioner.bad_words_ids: a list of token-id lists, taken as they are.  captioner.bad_words: a list of words, or the string
    "reference" (= `distributed.BANNED_WORDS`), turned into sequences by `bad_word_sequences` with the checkpoint's tokenizer
    (captioner.bad_words_mode: "word", the default, or "substring"); a model without a tokenizer refuses it by name.  Both keys
    given: the union.  Everything is validated here (`validate_bad_words_ids`), before an engine exists."""
    ids, words = getattr(cfg, "bad_words_ids", None), getattr(cfg, "bad_words", None)
    if ids is None and words is None:
        return None
    seqs = [] if ids is None else [list(q) if isinstance(q, Iterable) and not isinstance(q, (str, bytes)) else q for q in ids]
    if words is not None:
        if isinstance(words, str):
            if words != "reference":
                raise ValueError(f"captioner.bad_words must be a list of words or the string 'reference', got {words!r}")
            words = reference_banned_words()
        if tokenizer is None:
            raise ValueError("captioner.bad_words is given as words but this model has no tokenizer (a procedural model, or a checkpoint "
                             "directory without tokenizer files): give captioner.bad_words_ids instead")
        mode = getattr(cfg, "bad_words_mode", None) or "word"
        seqs += bad_word_sequences(list(words), tokenizer.get_vocab(),
                                   lambda s: list(tokenizer(s, add_special_tokens=False)["input_ids"]), mode)
    return validate_bad_words_ids(seqs, arch)


def reject_bad_words_keys(cfg, who: str) -> None:
    """The banned-word keys are BLIP's and BLIP-2's: a wrapper of another family that finds one in its configuration raises, naming
    it - a yaml key is never dropped silently."""
    given = [k for k in ("bad_words_ids", "bad_words", "bad_words_mode") if getattr(cfg, k, None) is not None]
    if given:
        raise ValueError(f"{who}: captioner.{' / captioner.'.join(given)} - banned words are implemented for arch_name 'blip' and 'blip2' "
                         f"only (the reference's CoCa.generate has no such option)")


def reference_banned_words() -> List[str]:
    """The reference's list (`distributed.BANNED_WORDS`): what `captioner.bad_words: reference` means."""
    from ..distributed import BANNED_WORDS
    return list(BANNED_WORDS)
