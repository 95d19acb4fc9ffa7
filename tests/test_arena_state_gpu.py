"""GPU: no result depends on what the handle's arena held before the call.

Every engine call X below is run four times on one handle and must write the same BYTES into every output buffer each time:

  (a) as the engine stands (created, loaded, whatever the earlier cases left);
  (b) after `_fill_arena(0xFFFFFFFF)`: every scratch buffer of the arena, rounded tails included, holds a word that is a NaN as
      fp32, as bf16 and as both fp16 halves of a split-fp16 word, and -1 with a NaN scale in a KV16 block;
  (c) after `_fill_arena(0x42F742F7)`: finite in all of those types (123.6 / 123.5 / 3.5) - the split mode's clamp and any fmaxf turn
      a NaN back into a number, so a NaN alone can be swallowed;
  (d) after a DIFFERENT call Y (largest batch, longest length, other inputs, other kinds of call) with no fill in between: what
      production leaves behind, and the one case that reaches the index buffers, which are never poisoned (a poisoned index is an
      address).

A kernel that reads a padding column, a key one past `past`, a split-K slab of a dead row, a row at or beyond `*n_live`, the ragged
last group of a KV16 block or a strip of a partial tile - and lets it reach an output - fails here and nowhere else in the suite.

Beam searches run (a), (c), (d) only: beam.hip's candidate ranking and beam_merge_kernel order candidates by comparisons that are all
false for a NaN, so a row of NaN scores leaves `src` / `tok` entries of the merge unwritten and they index the sequence and ancestry
tables.  That cannot be shown to stay in range by reading, so no NaN is put where a beam search could pick it up.  The greedy
selection never selects a NaN and always yields a token in [0, V) (ops.h), so greedy calls run all four.

Two calls of the table cannot be made as written and are placed where the library takes them: beam GROUPS are CoCa's (a BLIP handle
refuses them), and the small-batch path does not exist in the exact fp32 mode (forcing it is refused), so "small" runs in "f32s" and
"bf16".  Row compaction only engages above 16 rows, so besides the B = 5 calls with the switch on and off a 17-row engine runs
the compacted loop itself.

Tiny procedural architectures, max_batch 8, max_len 12 (40 for the BLIP case beyond the fused self-attention's 32 positions).  No
tolerances anywhere: `_util.same_bits`."""
import functools

import numpy as np
import pytest
import torch

from _util import same_bits

pytestmark = pytest.mark.gpu

NAN_WORD, FINITE_WORD = 0xFFFFFFFF, 0x42F742F7
ALL_FILLS, FINITE_ONLY = (NAN_WORD, FINITE_WORD), (FINITE_WORD,)
BM, L = 8, 12

KEPT = {"blip": ["patches"], "coca": ["patches"], "blip2": ["patches"], "clip": ["patches"], "itm": ["patches", "itm_ckv"], "minilm": []}
INDEX = {"blip": ["seq", "finished", "lens", "live", "n_live", "anc", "beam"], "coca": ["seq", "finished", "lens", "anc", "beam"],
         "blip2": ["seq", "finished", "lens", "anc", "beam"], "clip": [], "itm": [], "minilm": []}

_ENGINES = []


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _ENGINES:
        e.close()
    _ENGINES.clear()
    _engine.cache_clear()


# ------------------------------------------------------------------------------------------------ models, engines, inputs
@functools.lru_cache(maxsize=None)
def _model(family, variant=""):
    from embodied_captioning_amd import config as Cf
    from embodied_captioning_amd import weights as W
    if family == "blip":          # "open": no EOS boost, so captions stay open beyond 32 positions
        arch = Cf.BlipArch.tiny()
        if variant == "kv16":     # 6 x 6 patches = 37 image tokens: above 32 keys the split mode keeps the cross K/V as KV16, and the 2 x 37 head
            arch.image_size, arch.patch_size = 84, 14          # rows of an image end inside a block of 32; 14 px patches: 588 -> 640 padded columns
        return arch, W.procedural_blip_state_dict(arch, 3, eos_boost=0.0 if variant == "open" else 2.0)
    if family == "coca":
        arch = Cf.CocaArch.tiny()
        return arch, W.procedural_coca_state_dict(arch, 3, eos_boost=2.0)
    if family == "blip2":         # int8 weights need OPT widths that are multiples of 256
        arch = Cf.Blip2Arch.small() if variant == "int8" else Cf.Blip2Arch.tiny()
        return arch, W.procedural_blip2_state_dict(arch, 3, eos_boost=0.3)
    if family == "clip":
        arch = Cf.ClipArch.tiny()
        return arch, W.procedural_clip_state_dict(arch, 3)
    if family == "itm":
        arch = Cf.Blip2ItmArch.tiny()
        return arch, W.procedural_blip2_itm_state_dict(arch, 3)
    arch = Cf.MiniLMArch.tiny()
    return arch, W.procedural_minilm_state_dict(arch, 3)


@functools.lru_cache(maxsize=None)
def _engine(family, mode, variant=""):
    """One engine per (family, mode) - plus BLIP's three variants (KV16 geometry, 40 positions, 17 rows) - shared by the cases of the module."""
    from embodied_captioning_amd import engine as E
    dtype = "bf16" if mode == "int8" else mode
    if family == "blip":
        arch, sd = _model("blip", {"len40": "open", "kv16": "kv16"}.get(variant, ""))
        full = dict(max_batch=BM, max_beams=3, max_len=L, max_prompt=4, max_score_rows=6 * (L - 1))          # 12 captions: two passes
        kw = {"": full, "kv16": full,
              "len40": dict(max_batch=BM, max_beams=1, max_len=40),
              "rows17": dict(max_batch=17, max_beams=1, max_len=L)}[variant]
        eng = E.CaptionerEngine(arch, dtype=dtype, **kw)
    elif family == "coca":
        arch, sd = _model("coca")
        eng = E.CaptionerEngine(arch, dtype=dtype, max_batch=BM, max_beams=6, max_len=L)
    elif family == "blip2":
        arch, sd = _model("blip2", "int8" if mode == "int8" else "")
        eng = E.CaptionerEngine(arch, dtype=dtype, max_batch=BM, max_beams=3, max_len=L, weight_int8=mode == "int8")
    elif family == "clip":
        arch, sd = _model("clip")
        eng = E.ClipEngine(arch, dtype=dtype, max_batch=BM, max_len=L)
    elif family == "itm":
        arch, sd = _model("itm")
        eng = E.Blip2ItmEngine(arch, dtype=dtype, max_batch=BM, max_len=L)
    else:
        arch, sd = _model("minilm")
        eng = E.TextEncoderEngine(arch, dtype=dtype, max_batch=BM, max_len=L)
    eng.load_state_dict(sd)
    _ENGINES.append(eng)
    return eng


def _px(eng, B, seed=3):
    from embodied_captioning_amd.weights import synthetic_pixels
    return synthetic_pixels(B, eng.arch.image_size, seed=seed).cuda()


def _tokens(n, length, seed, lo=110, hi=290):
    """int32 [n, length] of ids that are no model's BOS / EOS / pad / image token (every tiny vocabulary has at least 300 entries)"""
    return torch.from_numpy(np.random.default_rng(seed).integers(lo, hi, size=(n, length)).astype(np.int32))


RAGGED = [7, L, 1, 4, L, 2, 9, 3]          # text lengths: the shortest, the longest, odd ones in between


def _text(n, seed, first, last, ragged=True):
    """Right-padded token rows for the text towers: `first` ... `last` at lens - 1, then padding ids; lens ragged or all L."""
    ids = _tokens(n, L, seed)
    lens = torch.tensor((RAGGED if ragged else [L] * BM)[:n], dtype=torch.int32)
    for r in range(n):
        ids[r, 0] = first
        ids[r, int(lens[r]) - 1] = last if int(lens[r]) > 1 else first
    return ids, lens


def _captions(eng, n_images, seed, length=L):
    """3 captions per image for `score`: BOS + tokens, lengths 2 .. length, absent slots (0), EOS as a scored last token"""
    ids = _tokens(n_images * 3, length, seed)
    ids[:, 0] = eng.arch.bos
    lens = np.array(([2, 6, length, 3, 0, length, 2, 9, length, length, 5, 0] * 2)[: n_images * 3], dtype=np.int32)
    for n in (2, 8):
        ids[n, length - 1] = eng.arch.eos
    return ids, torch.from_numpy(lens)


def _prompts(eng, B, shift=0):
    return torch.tensor([[eng.arch.bos, 111 + shift + r, 140 + shift + r] for r in range(B)], dtype=torch.int32)


# ------------------------------------------------------------------------------------------------ the property
def _flat(out):
    if isinstance(out, torch.Tensor):
        return {"out": out}
    if isinstance(out, dict):
        return dict(out)
    return {f"out{i}": t for i, t in enumerate(out)}


def _run(fn):
    """fn() with the stream drained.  Anything but a result ends the SESSION: after a device fault nothing more may run on the GPU."""
    try:
        out = _flat(fn())
        torch.cuda.synchronize()
        return {k: v.clone() for k, v in out.items()}
    except AssertionError:
        raise
    except Exception as e:  # noqa: BLE001
        pytest.exit(f"test_arena_state_gpu: a call raised ({type(e).__name__}: {e}); stopping before anything else runs on the GPU", returncode=3)


def _differences(ref, got):
    bad = []
    for k in ref:
        a, b = ref[k], got[k]
        if same_bits(a, b):
            continue
        it = {2: torch.int16, 4: torch.int32}[a.element_size()]
        ne = (a.contiguous().view(it) != b.contiguous().view(it)).nonzero()
        first = tuple(int(i) for i in ne[0])
        bad.append(f"{k}: {len(ne)} of {a.numel()} elements differ, first at {first}: {a[first].item()!r} -> {b[first].item()!r}")
    return bad


def check_arena_independence(eng, X, Y, fills=ALL_FILLS):
    """(a) - (d) of the module docstring for the call X on `eng`; every state is tried before the assertion, which names them all."""
    ref = _run(X)
    failures = []
    for pattern in fills:
        assert eng._fill_arena(pattern) == eng._arena_kinds()["scratch_bytes"]
        bad = _differences(ref, _run(X))
        if bad:
            failures.append(f"after fill 0x{pattern:08X}: " + "; ".join(bad))
    _run(Y)
    bad = _differences(ref, _run(X))
    if bad:
        failures.append("after the dirtying call: " + "; ".join(bad))
    print(f"arena-state: {len(failures)} of {len(fills) + 1} states changed the outputs")
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------ BLIP
def _blip_generate(eng, B, path="auto", compaction=True, seed=3, **kw):
    eng.set_decode_path(path)
    eng.set_row_compaction(compaction)
    try:
        return eng.generate(_px(eng, B, seed), max_length=eng.max_len, **kw)
    finally:
        eng.set_decode_path("auto")
        eng.set_row_compaction(True)


def _blip_dirty(eng):
    """Y for BLIP: a full batch of other images through 3 beams, a prompted call, a scoring call and a plain greedy batch"""
    def Y():
        px = _px(eng, BM, seed=11)
        outs = [eng.generate(px, num_beams=eng.max_beams, max_length=eng.max_len)["sequences"]] if eng.max_beams > 1 else []
        if eng.max_prompt:
            outs.append(eng.generate(px, max_length=eng.max_len, prompt_ids=_prompts(eng, BM, shift=20))["sequences"])
            ids, lens = _captions(eng, 4, seed=12)
            outs.append(eng.score(px[:4], ids, lens, captions_per_image=3)["token_logprobs"])
        outs.append(_blip_generate(eng, eng.max_batch, path="batch", seed=13, output_logits=True)["sequences"])
        return outs
    return Y


def _score_call(eng, B=4):
    ids, lens = _captions(eng, B, seed=5)
    px = _px(eng, B)

    def X():
        out = eng.score(px, ids, lens, captions_per_image=3)
        assert eng.last_score_passes >= 2          # the pass buffers are reused inside the call
        return out
    return X


BLIP_MODES = ["f32", "f32s", "bf16"]
# name: (call, fills) - calls take the engine
BLIP_CALLS = {
    "encode": (lambda e: e.encode(_px(e, 5)), ALL_FILLS),
    "greedy_batch_compaction_on": (lambda e: _blip_generate(e, 5, "batch", True), ALL_FILLS),
    "greedy_batch_compaction_off": (lambda e: _blip_generate(e, 5, "batch", False), ALL_FILLS),
    "greedy_small_1": (lambda e: _blip_generate(e, 1, "small"), ALL_FILLS),
    "greedy_small_2": (lambda e: _blip_generate(e, 2, "small"), ALL_FILLS),
    "beams_3": (lambda e: _blip_generate(e, 5, num_beams=3), FINITE_ONLY),
    "prompted": (lambda e: _blip_generate(e, 5, prompt_ids=_prompts(e, 5)), ALL_FILLS),
    "logprob_vocab_and_step_logits": (lambda e: _blip_generate(e, 5, output_logits=True, output_logprobs=True, output_vocab_maxprob=True),
                                      ALL_FILLS),
}


# the exact fp32 mode has no small-batch path (forcing it is refused: test_generate_request_gpu.py)
@pytest.mark.parametrize("mode,call", [(m, c) for m in BLIP_MODES for c in sorted(BLIP_CALLS) if not (m == "f32" and c.startswith("greedy_small"))])
def test_blip_outputs_do_not_depend_on_the_arena(mode, call):
    eng = _engine("blip", mode)
    fn, fills = BLIP_CALLS[call]
    check_arena_independence(eng, lambda: fn(eng), _blip_dirty(eng), fills)


@pytest.mark.parametrize("mode", BLIP_MODES)
def test_blip_score_in_two_passes_does_not_depend_on_the_arena(mode):
    eng = _engine("blip", mode)
    check_arena_independence(eng, _score_call(eng), _blip_dirty(eng))


@pytest.mark.parametrize("mode", BLIP_MODES)
def test_blip_compacted_greedy_loop_does_not_depend_on_the_arena(mode):
    """17 rows: the batch kernels over the open captions' rows only (RowMap), which B = 5 never reaches"""
    eng = _engine("blip", mode, "rows17")

    def X():
        out = _blip_generate(eng, 17)
        assert eng.last_row_compaction and eng.last_decode_path == "batch"
        return out
    check_arena_independence(eng, X, _blip_dirty(eng))


@pytest.mark.parametrize("mode", BLIP_MODES)
def test_blip_beyond_32_positions_does_not_depend_on_the_arena(mode):
    """max_len 40: from position 33 on the self-attention runs un-fused, on every path"""
    eng = _engine("blip", mode, "len40")

    def X():
        out = _blip_generate(eng, 5)
        assert int(out["lengths"].max()) > 34
        return out
    check_arena_independence(eng, X, _blip_dirty(eng))


@pytest.mark.parametrize("call", sorted(BLIP_CALLS) + ["score"])
def test_blip_split_mode_with_kv16_cross_cache_does_not_depend_on_the_arena(call):
    """The tiny geometry's 17 image tokens keep fp32 rows in "f32s" (the engines above) and its 8 px patches need no padding columns; 37
    tokens of 14 px patches make the cross K/V cache KV16 and the patch rows padded (`patches`, the kept buffer, as in the other families)"""
    eng = _engine("blip", "f32s", "kv16")
    assert eng.cross_cache_kind == "kv16" and _engine("blip", "f32s").cross_cache_kind == "fp32"
    if call == "score":
        return check_arena_independence(eng, _score_call(eng), _blip_dirty(eng))
    fn, fills = BLIP_CALLS[call]
    check_arena_independence(eng, lambda: fn(eng), _blip_dirty(eng), fills)


# ------------------------------------------------------------------------------------------------ CoCa
def _coca_dirty(eng):
    def Y():
        px = _px(eng, BM, seed=11)
        return [eng.generate(px, num_beams=3, max_length=L)["sequences"], eng.generate(px, max_length=L, output_logits=True)["sequences"]]
    return Y


COCA_CALLS = {
    "encode": (lambda e: e.encode(_px(e, 5)), ALL_FILLS),
    "greedy": (lambda e: _blip_generate(e, 5), ALL_FILLS),
    "greedy_batch": (lambda e: _blip_generate(e, 5, "batch"), ALL_FILLS),
    "legacy_beams_3": (lambda e: _blip_generate(e, 5, num_beams=3), FINITE_ONLY),
    "beam_groups_6_in_3": (lambda e: _blip_generate(e, 2, num_beams=6, num_beam_groups=3), FINITE_ONLY),
}


@pytest.mark.parametrize("call", sorted(COCA_CALLS))
@pytest.mark.parametrize("mode", ["f32", "f32s", "bf16"])
def test_coca_outputs_do_not_depend_on_the_arena(mode, call):
    eng = _engine("coca", mode)
    fn, fills = COCA_CALLS[call]
    check_arena_independence(eng, lambda: fn(eng), _coca_dirty(eng), fills)


# ------------------------------------------------------------------------------------------------ BLIP-2
def _blip2_dirty(eng):
    def Y():
        px = _px(eng, BM, seed=11)
        ids, lens = _captions(eng, 4, seed=12)
        return [eng.generate(px, num_beams=3, max_length=L)["sequences"], eng.score(px[:4], ids, lens, captions_per_image=3)["token_logprobs"],
                eng.generate(px, max_length=L, output_logits=True)["sequences"]]
    return Y


BLIP2_CALLS = {
    "greedy": (lambda e: e.generate(_px(e, 5), max_length=L), ALL_FILLS),
    "beams_3": (lambda e: e.generate(_px(e, 5), num_beams=3, max_length=L), FINITE_ONLY),
    "score": (lambda e: _score_call(e)(), ALL_FILLS),
}


@pytest.mark.parametrize("call", sorted(BLIP2_CALLS))
@pytest.mark.parametrize("mode", ["f32", "f32s", "bf16", "int8"])
def test_blip2_outputs_do_not_depend_on_the_arena(mode, call):
    eng = _engine("blip2", mode)
    fn, fills = BLIP2_CALLS[call]
    check_arena_independence(eng, lambda: fn(eng), _blip2_dirty(eng), fills)


# ------------------------------------------------------------------------------------------------ CLIP, MiniLM
def _clip_text(eng, n, seed, ragged=True):
    return _text(n, seed, eng.arch.bos_token_id, eng.arch.eos_token_id, ragged)


@pytest.mark.parametrize("call", ["embed_images", "embed_text"])
@pytest.mark.parametrize("mode", ["f32", "f32s", "bf16"])
def test_clip_outputs_do_not_depend_on_the_arena(mode, call):
    eng = _engine("clip", mode)
    ids, lens = _clip_text(eng, 5, seed=5)
    X = (lambda: eng.embed_images(_px(eng, 5))) if call == "embed_images" else (lambda: eng.embed_text(ids, lens))

    def Y():
        return [eng.embed_images(_px(eng, BM, seed=11)), eng.embed_text(*_clip_text(eng, BM, seed=12, ragged=False))]
    check_arena_independence(eng, X, Y)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_minilm_embed_does_not_depend_on_the_arena(mode):
    eng = _engine("minilm", mode)
    ids, lens = _text(5, 5, eng.arch.cls, eng.arch.sep)
    check_arena_independence(eng, lambda: eng.embed(ids, lens), lambda: eng.embed(*_text(BM, 12, eng.arch.cls, eng.arch.sep, ragged=False)))


# ------------------------------------------------------------------------------------------------ BLIP-2 image-text scorer
def _itm_text(n, seed, ragged=True):
    return _text(n, seed, 101, 102, ragged)


def _itm_text_side(eng, ids, lens):
    logits, prob = eng.itm(ids, lens)
    return {"itc_image": eng.itc_image_features(), "itc_text": eng.itc_text_features(ids, lens), "itm_logits": logits, "itm_prob": prob}


@pytest.mark.parametrize("mode", ["f32", "f32s", "bf16"])
def test_itm_image_and_text_calls_do_not_depend_on_the_arena(mode):
    """Fills before `encode_images`: nothing of the image side, and nothing of the text side behind it, reads the arena's past"""
    eng = _engine("itm", mode)
    ids, lens = _itm_text(5, seed=5)

    def X():
        eng.encode_images(_px(eng, 5))
        return _itm_text_side(eng, ids, lens)

    def Y():
        eng.encode_images(_px(eng, BM, seed=11))
        return _itm_text_side(eng, *_itm_text(BM, seed=12, ragged=False))
    check_arena_independence(eng, X, Y)


@pytest.mark.parametrize("mode", ["f32", "f32s", "bf16"])
def test_itm_text_calls_read_only_the_kept_buffers_of_encode_images(mode):
    """Fills BETWEEN `encode_images` and the text-side calls: what they take from the image call lives in kept buffers (`itm_ckv`), and
    nothing else of the arena carries over.  With `itm_ckv` as scratch the fill would destroy it; with a scratch buffer carrying state the
    text side would change."""
    eng = _engine("itm", mode)
    ids, lens = _itm_text(5, seed=5)
    eng.encode_images(_px(eng, 5))

    def Y():          # the resident batch stays: other captions, the widest text batch
        return [eng.itm(*_itm_text(5, seed=12, ragged=False))[0], eng.itc_text_features(*_itm_text(BM, seed=13, ragged=False))]
    check_arena_independence(eng, lambda: _itm_text_side(eng, ids, lens), Y)


# ------------------------------------------------------------------------------------------------ structure
STRUCTURE = ([("blip", m, v) for m in BLIP_MODES for v in ("", "len40", "rows17")] + [("blip", "f32s", "kv16")] +
             [(f, m, "") for f in ("coca", "clip", "itm") for m in ("f32", "f32s", "bf16")] +
             [("blip2", m, "") for m in ("f32", "f32s", "bf16", "int8")] + [("minilm", m, "") for m in ("f32", "bf16")])


@pytest.mark.parametrize("family,mode,variant", STRUCTURE)
def test_every_arena_allocation_is_classified(family, mode, variant):
    eng = _engine(family, mode, variant)
    k = eng._arena_kinds()
    print(f"arena {family} {mode} {variant}: scratch {k['scratch_bytes']} index {k['index_bytes']} kept {k['kept_bytes']}")
    assert k["scratch_bytes"] + k["index_bytes"] + k["kept_bytes"] == k["arena_bytes"]          # nothing unclassified
    assert 0 < k["arena_bytes"] < eng.device_bytes                                              # the weights are not arena
    assert k["kept"] == KEPT[family]          # a new kept buffer needs an owner in DESIGN.md and a line here
    index = [n for n in INDEX[family] if not (family == "blip2" and eng.max_beams == 1 and n in ("anc", "beam"))]
    assert k["index"] == index
    assert (k["kept_bytes"] > 0) == bool(k["kept"]) and (k["index_bytes"] > 0) == bool(k["index"])
    assert eng._fill_arena(FINITE_WORD) == k["scratch_bytes"]


def test_a_shared_handle_fills_its_own_arena_only():
    """`cap_create_shared`: the fill reaches neither the weight store nor the other handle's arena"""
    from embodied_captioning_amd.engine import Blip2ItmEngine
    owner = _engine("itm", "f32s")
    ids, lens = _itm_text(5, seed=5)
    owner.encode_images(_px(owner, 5))
    ref = _run(lambda: _itm_text_side(owner, ids, lens))
    other = Blip2ItmEngine(owner.arch, dtype="f32s", max_batch=BM, max_len=L, share_weights_with=owner)
    _ENGINES.append(other)
    k = other._arena_kinds()
    assert k["arena_bytes"] == other.device_bytes == k["scratch_bytes"] + k["index_bytes"] + k["kept_bytes"]
    assert k["kept"] == KEPT["itm"] and k["arena_bytes"] == owner._arena_kinds()["arena_bytes"]
    other.encode_images(_px(other, 5))
    for pattern in ALL_FILLS:
        assert other._fill_arena(pattern) == k["scratch_bytes"]
        assert not _differences(ref, _run(lambda: _itm_text_side(owner, ids, lens)))          # the owner's kept state and the weights stand
        assert not _differences(ref, _run(lambda: _itm_text_side(other, ids, lens)))
