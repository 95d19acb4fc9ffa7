"""CPU: what the four engines hand to cap_create.  The constructors run without a GPU against a stub library that keeps the
CapConfig bytes; the non-zero fields of every kind must be the ones recorded in tests/golden/engine_configs.json (a dict of fields,
not raw bytes, so that a field appended to the struct later does not invalidate it).  Also the constructors' refusals, and the class
surface: one base under the four engines, and nothing of the captioner's on a scorer."""
import contextlib
import ctypes as C
import json
import os
import re

import pytest
import torch

from embodied_captioning_amd import _native as N
from embodied_captioning_amd import engine as E
from embodied_captioning_amd.config import Blip2Arch, Blip2ItmArch, BlipArch, ClipArch, CocaArch, MiniLMArch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "engine_configs.json")

CASES = {
    "blip": (E.CaptionerEngine, BlipArch, dict(max_batch=4, max_beams=3, max_len=12, max_prompt=5, max_score_rows=64)),
    "coca": (E.CaptionerEngine, CocaArch, dict(max_batch=4, max_beams=6, max_len=12, cross_cache="fp32")),
    "blip2": (E.CaptionerEngine, Blip2Arch, dict(dtype="bf16", max_batch=2, max_len=8, weight_int8=True)),
    "minilm": (E.TextEncoderEngine, MiniLMArch, dict(max_batch=8, max_len=16)),
    "clip": (E.ClipEngine, ClipArch, dict(max_batch=8)),
    "blip2_itm": (E.Blip2ItmEngine, Blip2ItmArch, dict(max_batch=8)),
}


class StubLibrary:
    """cap_create / cap_create_shared keep (entry, config bytes, handle shared with) and hand out 1, 2, ... as handles."""

    def __init__(self):
        self.created = []

    def _create(self, entry, cfg, shared, out):
        self.created.append((entry, bytes(cfg._obj), None if shared is None else shared.value))
        out._obj.value = len(self.created)
        return 0

    def cap_create(self, cfg, out):
        return self._create("cap_create", cfg, None, out)

    def cap_create_shared(self, cfg, shared, out):
        return self._create("cap_create_shared", cfg, shared, out)

    def cap_destroy(self, h):
        return 0


@pytest.fixture
def stub(monkeypatch):
    lib = StubLibrary()
    monkeypatch.setattr(N, "load_library", lambda *a, **k: lib)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "device", lambda *a, **k: contextlib.nullcontext())
    return lib


def nonzero_fields(raw: bytes) -> dict:
    cfg = N.CapConfig.from_buffer_copy(raw)
    out = {}
    for name, _ in N.CapConfig._fields_:
        v = getattr(cfg, name)
        v = list(v) if isinstance(v, C.Array) else v
        if any(v) if isinstance(v, list) else v:
            out[name] = v
    return out


def build(stub, case, **more):
    cls, arch, kw = CASES[case]
    eng = cls(arch.tiny(), device="cpu", **kw, **more)
    entry, raw, shared = stub.created[-1]
    eng.close()                  # while torch.cuda.device is still the null context
    return eng, entry, nonzero_fields(raw), shared


@pytest.mark.parametrize("case", list(CASES))
def test_config_handed_to_cap_create_is_the_recorded_one(stub, case):
    golden = json.load(open(GOLDEN))
    eng, entry, fields, shared = build(stub, case)
    assert entry == "cap_create" and shared is None and not eng.shares_weights
    assert fields["struct_size"] == C.sizeof(N.CapConfig)
    assert fields == golden[case]


def test_share_weights_with_goes_through_cap_create_shared_with_the_first_handle(stub):
    cls, arch, kw = CASES["blip"]
    first = cls(arch.tiny(), device="cpu", **kw)
    handle = first._h.value
    assert handle == 1 and stub.created[-1][0] == "cap_create"
    second = cls(arch.tiny(), device="cpu", share_weights_with=first, **kw)
    entry, raw, shared = stub.created[-1]
    assert entry == "cap_create_shared" and shared == handle and second._h.value == 2
    assert second.shares_weights and not first.shares_weights
    assert nonzero_fields(raw) == json.load(open(GOLDEN))["blip"]
    first.close(), second.close()


@pytest.mark.parametrize("case, kw, message", [
    ("coca", dict(max_prompt=5), f"max_prompt = 5: prompt capacity is BLIP's, 0 or 2..{N.CAP_MAX_PROMPT} tokens (BOS included)"),
    ("blip2", dict(max_prompt=5), f"max_prompt = 5: prompt capacity is BLIP's, 0 or 2..{N.CAP_MAX_PROMPT} tokens (BOS included)"),
    ("blip", dict(max_prompt=1), f"max_prompt = 1: prompt capacity is BLIP's, 0 or 2..{N.CAP_MAX_PROMPT} tokens (BOS included)"),
    ("blip", dict(max_prompt=N.CAP_MAX_PROMPT + 1),
     f"max_prompt = {N.CAP_MAX_PROMPT + 1}: prompt capacity is BLIP's, 0 or 2..{N.CAP_MAX_PROMPT} tokens (BOS included)"),
    ("coca", dict(max_score_rows=64), "max_score_rows = 64: scoring capacity is BLIP's, 0 or a row count"),
    ("blip", dict(cross_cache="bf16"), "cross_cache must be 'auto' or 'fp32', got 'bf16'"),
    ("blip", dict(weight_int8=True), "weight_int8 (load_in_8bit) is built for BLIP-2 with dtype 'bf16'"),
    ("blip2", dict(dtype="f32s"), "weight_int8 (load_in_8bit) is built for BLIP-2 with dtype 'bf16'"),
])
def test_constructor_refusals_keep_type_and_text(stub, case, kw, message):
    cls, arch, base = CASES[case]
    with pytest.raises(ValueError, match="^" + re.escape(message) + "$"):
        cls(arch.tiny(), device="cpu", **{**base, **kw})
    assert stub.created == []            # refused before a handle exists


@pytest.mark.parametrize("case", list(CASES))
def test_without_a_gpu_the_refusal_names_the_concrete_class(monkeypatch, case):
    cls, arch, kw = CASES[case]
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(N.CaptionerHipError, match=rf"^{cls.__name__} needs a GPU.*there is no CPU fallback in the product path$"):
        cls(arch.tiny(), **kw)


COMMON = {"load_state_dict", "close", "device_bytes", "profile", "profile_report", "_fill_arena", "_arena_kinds"}
SURFACE = {
    E.TextEncoderEngine: COMMON | {"embed"},
    E.ClipEngine: COMMON | {"embed_images", "embed_text", "logits", "saturations"},
    E.Blip2ItmEngine: COMMON | {"encode_images", "itc_image_features", "itc_text_features", "itc_scores", "itm", "saturations"},
}
CAPTIONER_ONLY = ("generate", "score", "image_state", "encode", "set_bad_words", "set_decode_path", "set_row_compaction")


def test_four_engines_share_one_base_and_scorers_do_not_get_the_captioner_surface():
    classes = (E.CaptionerEngine, *SURFACE)
    bases = set.intersection(*({c for c in cls.__mro__ if c is not object} for cls in classes))
    assert len(bases) == 1, bases                                  # one common ancestor, and it is none of the four
    assert not bases & set(classes)
    for cls, names in SURFACE.items():
        assert not issubclass(cls, E.CaptionerEngine)
        missing = sorted(n for n in names if not hasattr(cls, n))
        assert not missing, (cls.__name__, missing)
        handed = [n for n in CAPTIONER_ONLY if hasattr(cls, n)]
        assert not handed, (cls.__name__, handed)
    for n in CAPTIONER_ONLY + tuple(COMMON) + ("saturations", "DECODE_PATHS"):
        assert hasattr(E.CaptionerEngine, n), n
