"""GPU: encode once, then generate, prompt and score from the image state - every result the BITS of the call from pixels.

`image_state(pixels)` exports what the decode side reads from the image side into a plain uint8 tensor; `generate` / `score` given that
tensor import it into the arena for the call's batch instead of running the image side.  Both are re-layouts of bytes the decoder
reads anyway, so there are no tolerances here: `_util.same_bits` on every output, against the calls from pixels, which the rest of
the suite pins to HF and the restatements.  Tiny procedural architectures, max_batch 8, 5 images, max_len 12.

A call that raises where a result was expected ends the session (`_run`): after a device fault nothing more may run on the GPU."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

from _util import same_bits

pytestmark = pytest.mark.gpu

BM, L, NIMG = 8, 12, 5
NAN_WORD, FINITE_WORD = 0xFFFFFFFF, 0x42F742F7
SUBSETS = {"subset_4_0_0_2": [4, 0, 0, 2], "single": [3], "repeated_8": [0, 1, 2, 3, 4, 0, 1, 2]}
IMAGE_SIDE_TAGS = ("patchify", "gemm_qkv", "vit_attention", "gemm_crosskv")

_ENGINES = []


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _ENGINES:
        e.close()
    _ENGINES.clear()
    for f in (_engine, _reference, _state):
        f.cache_clear()


# ------------------------------------------------------------------------------------------------ models, engines, inputs
@functools.lru_cache(maxsize=None)
def _model(family, variant=""):
    from embodied_captioning_amd import config as Cf
    from embodied_captioning_amd import weights as W
    if family == "blip":
        arch = Cf.BlipArch.tiny()
        if variant == "kv16":          # the KV16 geometry of test_arena_state_gpu.py: 6 x 6 patches of 14 px = 37 image tokens, 74 head rows per image
            arch.image_size, arch.patch_size = 84, 14
        return arch, W.procedural_blip_state_dict(arch, 3, eos_boost=2.0)
    if family == "coca":
        arch = Cf.CocaArch.tiny()
        return arch, W.procedural_coca_state_dict(arch, 3, eos_boost=2.0)
    arch = Cf.Blip2Arch.small() if variant == "int8" else Cf.Blip2Arch.tiny()
    return arch, W.procedural_blip2_state_dict(arch, 3, eos_boost=0.3)


BLIP_CONFIGS = [("f32", ""), ("f32s", ""), ("bf16", ""), ("f32s", "kv16")]
BLIP_IDS = ["f32", "f32s", "bf16", "f32s_kv16"]


@functools.lru_cache(maxsize=None)
def _engine(family, mode, variant="", max_batch=BM, sharing=False):
    from embodied_captioning_amd import engine as E
    arch, sd = _model(family, variant)
    owner = _engine(family, mode, variant) if sharing else None
    if family == "blip":
        kw = dict(max_beams=3, max_len=L, max_prompt=4, max_score_rows=6 * (L - 1))
    elif family == "coca":
        kw = dict(max_beams=6, max_len=L)
    else:
        kw = dict(max_beams=3, max_len=L, weight_int8=variant == "int8")
    eng = E.CaptionerEngine(arch, dtype="bf16" if variant == "int8" else mode, max_batch=max_batch, share_weights_with=owner, **kw)
    if owner is None:
        eng.load_state_dict(sd)
    _ENGINES.append(eng)
    return eng


def _px(eng, B=NIMG, seed=3):
    from embodied_captioning_amd.weights import synthetic_pixels
    return synthetic_pixels(B, eng.arch.image_size, seed=seed).cuda()


def _captions(eng, n_images, per_image=2, seed=5):
    """`per_image` captions per image for `score`: BOS + tokens that are no model's BOS / EOS / pad, ragged lengths, one ending in EOS"""
    n = n_images * per_image
    ids = torch.from_numpy(np.random.default_rng(seed).integers(110, 290, size=(n, L)).astype(np.int32))
    ids[:, 0] = eng.arch.bos
    lens = torch.tensor(([L, 6, 2, 9, L, 3, 7, L, 4, 5] * 2)[:n], dtype=torch.int32)
    ids[1, 5] = eng.arch.eos
    return ids, lens


def _run(fn):
    try:
        out = fn()
        torch.cuda.synchronize()
        return {k: v.clone() for k, v in out.items()} if isinstance(out, dict) else out.clone()
    except AssertionError:
        raise
    except Exception as e:  # noqa: BLE001
        pytest.exit(f"test_image_state_gpu: a call raised ({type(e).__name__}: {e}); stopping before anything else runs on the GPU", returncode=3)


def _same(ref, got, what):
    assert set(ref) == set(got), what
    bad = [k for k in ref if not same_bits(ref[k], got[k])]
    assert not bad, f"{what}: {bad} differ from the call on pixels"


# name: call(engine, pixels or state, images the rows are: indices into the 5)
def _score(eng, x, rows):
    ids, lens = _captions(eng, NIMG)
    sel = torch.tensor([2 * r + c for r in rows for c in range(2)])
    return eng.score(x, ids[sel], lens[sel], captions_per_image=2)


CALLS = {
    "greedy_logits_logprobs": lambda e, x, rows: e.generate(x, max_length=L, output_logits=True, output_logprobs=True),
    "greedy_logprobs": lambda e, x, rows: e.generate(x, max_length=L, output_logprobs=True),
    "vocab_maxprob": lambda e, x, rows: e.generate(x, max_length=L, output_vocab_maxprob=True),
    "beams_3": lambda e, x, rows: e.generate(x, num_beams=3, max_length=L),
    "beams_5": lambda e, x, rows: e.generate(x, num_beams=5, max_length=L),
    "groups_6_in_3": lambda e, x, rows: e.generate(x, num_beams=6, num_beam_groups=3, max_length=L),
    "prompt_4": lambda e, x, rows: e.generate(x, max_length=L, prompt_ids=[e.arch.bos, 111, 140, 173]),
    "greedy": lambda e, x, rows: e.generate(x, max_length=L),
    "score_2": _score,
}
ALL = tuple(range(NIMG))


@functools.lru_cache(maxsize=None)
def _reference(family, mode, variant, call, rows=ALL):
    """The call from PIXELS on the module's engine of that configuration: computed once, shared, never changed"""
    eng = _engine(family, mode, variant)
    return _run(lambda: CALLS[call](eng, _px(eng)[list(rows)], rows))


@functools.lru_cache(maxsize=None)
def _state(family, mode, variant):
    eng = _engine(family, mode, variant)
    st = _run(lambda: eng.image_state(_px(eng)))
    assert st.dtype == torch.uint8 and tuple(st.shape) == (NIMG, eng.image_state_bytes) and st.is_cuda and type(st) is torch.Tensor
    return st


def _check(family, mode, variant, call, rows=ALL, eng=None):
    eng = eng or _engine(family, mode, variant)
    st = _state(family, mode, variant)
    x = st if rows == ALL else st[list(rows)]
    ref = _reference(family, mode, variant, call, rows)
    # the reference ran on this engine, or its images were the last through it: nothing of them may help the call from the state
    assert eng._fill_arena(FINITE_WORD) == eng._arena_kinds()["scratch_bytes"]
    _same(ref, _run(lambda: CALLS[call](eng, x, rows)), f"{family} {mode} {variant} {call} rows {rows}")


# ------------------------------------------------------------------------------------------------ BLIP
@pytest.mark.parametrize("call", ["greedy_logits_logprobs", "vocab_maxprob", "beams_3", "prompt_4", "score_2"])
@pytest.mark.parametrize("mode,variant", BLIP_CONFIGS, ids=BLIP_IDS)
def test_blip_calls_from_a_state_give_the_bits_of_the_calls_from_pixels(mode, variant, call):
    eng = _engine("blip", mode, variant)
    assert eng.cross_cache_kind == {"f32": "fp32", "bf16": "bf16", "f32s": "kv16" if variant else "fp32"}[mode]
    _check("blip", mode, variant, call)


@pytest.mark.parametrize("sel", sorted(SUBSETS))
@pytest.mark.parametrize("mode,variant", BLIP_CONFIGS, ids=BLIP_IDS)
def test_blip_subsets_reorderings_and_repeats_are_indexing(mode, variant, sel):
    _check("blip", mode, variant, "greedy_logprobs", tuple(SUBSETS[sel]))


@pytest.mark.parametrize("mode,variant", BLIP_CONFIGS, ids=BLIP_IDS)
def test_blip_state_of_one_engine_decodes_on_another_with_the_same_weights(mode, variant):
    other = _engine("blip", mode, variant, max_batch=6, sharing=True)
    assert other.image_state_bytes == _engine("blip", mode, variant).image_state_bytes
    for call in ("greedy_logprobs", "beams_3"):
        _check("blip", mode, variant, call, eng=other)
    # and the other way round: what the second engine exports is what the first did
    assert torch.equal(_run(lambda: other.image_state(_px(other))), _state("blip", mode, variant))


def test_the_state_is_the_layout_the_header_states():
    """BLIP tiny on the KV16 geometry: 2 layers x (k, v) sections of 2 heads x 37 tokens, and the record size of the reference"""
    import _image_state_ref as R
    eng = _engine("blip", "f32s", "kv16")
    a = eng.arch
    assert eng.image_state_bytes == R.record_bytes(2, a.t_layers, a.t_heads, a.n_tokens)
    st = _state("blip", "f32s", "kv16").cpu().numpy()
    used = 2 * a.t_layers * R.section_bytes(2, a.t_heads, a.n_tokens)
    assert not st[:, used:].any() and st[:, :used].any()
    for mode, kind in (("f32", 0), ("bf16", 1)):
        e = _engine("blip", mode)
        assert e.image_state_bytes == R.record_bytes(kind, e.arch.t_layers, e.arch.t_heads, e.arch.n_tokens)


# ------------------------------------------------------------------------------------------------ CoCa, BLIP-2
@pytest.mark.parametrize("call", ["greedy_logprobs", "beams_5", "groups_6_in_3"])
@pytest.mark.parametrize("mode", ["f32s", "bf16"])
def test_coca_calls_from_a_state_give_the_bits_of_the_calls_from_pixels(mode, call):
    _check("coca", mode, "", call)


@pytest.mark.parametrize("call", ["greedy", "beams_3", "score_2"])
@pytest.mark.parametrize("mode", ["f32s", "bf16"])
def test_blip2_calls_from_a_state_give_the_bits_of_the_calls_from_pixels(mode, call):
    eng = _engine("blip2", mode)
    assert eng.image_state_bytes == (eng.arch.num_query_tokens * eng.arch.t_hidden * 4 + 255) // 256 * 256
    _check("blip2", mode, "", call)


def test_blip2_int8_greedy_from_a_state_gives_the_bits_of_the_call_from_pixels():
    _check("blip2", "bf16", "int8", "greedy")
    _check("blip2", "bf16", "int8", "greedy", tuple(SUBSETS["subset_4_0_0_2"]))


# ------------------------------------------------------------------------------------------------ the image side does not run
@pytest.mark.parametrize("family,mode,variant", [("blip", "f32s", "kv16"), ("blip", "bf16", ""), ("coca", "f32s", ""), ("blip2", "bf16", "")])
def test_the_image_side_does_not_run_from_a_state(family, mode, variant):
    eng = _engine(family, mode, variant)
    st = _state(family, mode, variant)
    try:
        eng.profile(True)
        _run(lambda: eng.generate(st, max_length=L))
        rep = eng.profile_report()
        assert rep["state_import"]["launches"] == 1 and "state_export" not in rep
        assert not [t for t in IMAGE_SIDE_TAGS if t in rep], sorted(rep)
        eng.profile(True)
        _run(lambda: eng.image_state(_px(eng)))
        rep = eng.profile_report()
        assert rep["state_export"]["launches"] == 1 and "state_import" not in rep
        assert "patchify" in rep and "gemm_qkv" in rep          # and the export is the image side, nothing of the decoder
        assert not [t for t in rep if "select" in t or "vocab" in t], sorted(rep)
    finally:
        eng.profile(False)


# ------------------------------------------------------------------------------------------------ arena independence
@pytest.mark.parametrize("family,mode,variant,call,fills", [
    ("blip", "f32s", "kv16", "greedy_logprobs", (NAN_WORD, FINITE_WORD)), ("blip", "f32s", "kv16", "beams_3", (FINITE_WORD,)),
    ("blip", "bf16", "", "greedy_logprobs", (NAN_WORD, FINITE_WORD)), ("blip", "f32", "", "greedy_logprobs", (NAN_WORD, FINITE_WORD)),
    ("coca", "f32s", "", "greedy_logprobs", (NAN_WORD, FINITE_WORD)), ("blip2", "f32s", "", "greedy", (NAN_WORD, FINITE_WORD)),
    ("blip2", "f32s", "", "beams_3", (FINITE_WORD,))])
def test_a_call_from_a_state_does_not_depend_on_the_arena(family, mode, variant, call, fills):
    """The import writes every byte of the image side that the decoder reads: the same bytes after a NaN fill and a finite fill of the
    arena's scratch buffers.  Beam searches get the finite fill only (tests/test_arena_state_gpu.py's header says why)."""
    eng = _engine(family, mode, variant)
    st = _state(family, mode, variant)
    ref = _reference(family, mode, variant, call)
    for pattern in fills:
        assert eng._fill_arena(pattern) == eng._arena_kinds()["scratch_bytes"]
        _same(ref, _run(lambda: CALLS[call](eng, st, ALL)), f"after fill 0x{pattern:08X}")
    # a subset after the fill: the cache beyond the call's B' and the ragged tail of its last KV16 group hold the pattern
    rows = tuple(SUBSETS["subset_4_0_0_2"])
    assert eng._fill_arena(fills[0]) == eng._arena_kinds()["scratch_bytes"]
    _same(_reference(family, mode, variant, call, rows), _run(lambda: CALLS[call](eng, st[list(rows)], rows)), "subset after a fill")


# ------------------------------------------------------------------------------------------------ pool
def test_pool_merges_state_batches_as_it_merges_pixel_batches():
    from embodied_captioning_amd.engine import EnginePool
    eng = _engine("blip", "f32s", "kv16")
    st = _state("blip", "f32s", "kv16")
    pool = EnginePool(eng.arch, n=2, dtype="f32s", max_batch=BM, max_beams=1, max_len=L, weights_of=eng)
    _ENGINES.extend(pool.engines)
    groups = [(0, 1), (2, 3, 4), (4, 0)]
    outs = _run_list(lambda: pool.generate_many([st[list(g)] for g in groups], coalesce_rows=BM, max_length=L, output_logprobs=True))
    assert isinstance(pool.last_coalesce, list) and any(len(g) > 1 for g in pool.last_coalesce), pool.last_coalesce
    for g, out in zip(groups, outs):
        _same(_reference("blip", "f32s", "kv16", "greedy_logprobs", g), out, f"pool batch {g}")
    # submit / run with a state, and a state made by a pool engine
    out = _run(lambda: pool.run(2, st, max_length=L, output_logprobs=True))
    _same(_reference("blip", "f32s", "kv16", "greedy_logprobs"), out, "pool.run")
    made = _run(lambda: _joined(pool, pool.submit(_px(eng), method="image_state")))
    assert torch.equal(made, st)


def _joined(pool, out):
    pool.join()
    return out


def _run_list(fn):
    try:
        outs = fn()
        torch.cuda.synchronize()
        return [{k: v.clone() for k, v in o.items()} for o in outs]
    except Exception as e:  # noqa: BLE001
        pytest.exit(f"test_image_state_gpu: a call raised ({type(e).__name__}: {e}); stopping before anything else runs on the GPU", returncode=3)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_are_by_name_and_before_any_launch():
    from embodied_captioning_amd import _native as N
    from embodied_captioning_amd import config as Cf
    from embodied_captioning_amd import engine as E
    eng, other = _engine("blip", "f32s", "kv16"), _engine("blip", "bf16")
    st = _state("blip", "f32s", "kv16")
    lib, s = eng.lib, C.c_void_p(torch.cuda.current_stream().cuda_stream)
    # a state of another engine's row size: refused on the host, both sizes named
    assert other.image_state_bytes != eng.image_state_bytes
    for fn in (lambda: other.generate(st, max_length=L), lambda: other.score(st, *_captions(other, NIMG, 1), captions_per_image=1)):
        with pytest.raises(ValueError) as e:
            fn()
        assert str(eng.image_state_bytes) in str(e.value) and str(other.image_state_bytes) in str(e.value) and "cross-cache kind" in str(e.value)
    with pytest.raises(ValueError, match="frames"):
        eng.image_state(st)
    # everything below must leave the stream and the outputs alone: the outputs hold a pattern
    ids = torch.full((BM + 1, L), -7, dtype=torch.int32, device="cuda")
    lens = torch.full((BM + 1,), -7, dtype=torch.int32, device="cuda")
    emb = torch.full((NIMG, eng.arch.n_tokens, eng.arch.v_hidden), -7.0, device="cuda")
    eng.profile(True)
    try:
        def refused(rc, *words):
            assert rc != 0
            msg = lib.cap_last_error().decode()
            assert all(w in msg for w in words), msg
        gen = lambda p, B: lib.cap_generate(eng._h, C.c_void_p(p), N.CAP_PIX_IMAGE_STATE, B, 1, L, C.c_float(1.0), C.c_void_p(ids.data_ptr()),  # noqa: E731
                                            C.c_void_p(lens.data_ptr()), None, None, s)
        refused(lib.cap_encode(eng._h, C.c_void_p(st.data_ptr()), N.CAP_PIX_IMAGE_STATE, NIMG, C.c_void_p(emb.data_ptr()), s),
                "cap_encode", "CAP_PIX_IMAGE_STATE")
        refused(gen(None, NIMG), "cap_generate", "null")
        refused(gen(st.data_ptr() + 8, 1), "cap_generate", "16-byte aligned")
        big = st[[0] * (BM + 1)].contiguous()
        refused(gen(big.data_ptr(), BM + 1), "cap_generate", "capacity")
        refused(lib.cap_encode_image_state(eng._h, C.c_void_p(st.data_ptr()), N.CAP_PIX_IMAGE_STATE, NIMG, C.c_void_p(big.data_ptr()), s),
                "cap_encode_image_state", "CAP_PIX_IMAGE_STATE")
        px = _px(eng)
        refused(lib.cap_encode_image_state(eng._h, C.c_void_p(px.data_ptr()), N.CAP_PIX_F32_NCHW, NIMG, None, s), "cap_encode_image_state", "null")
        refused(lib.cap_encode_image_state(eng._h, C.c_void_p(px.data_ptr()), N.CAP_PIX_F32_NCHW, NIMG, C.c_void_p(big.data_ptr() + 4), s),
                "cap_encode_image_state", "16-byte aligned")
        refused(lib.cap_encode_image_state(eng._h, C.c_void_p(px.data_ptr()), N.CAP_PIX_F32_NCHW, BM + 1, C.c_void_p(big.data_ptr()), s),
                "cap_encode_image_state", "capacity")
        sc = torch.full((NIMG, L - 1), -7.0, device="cuda")
        refused(lib.cap_score_captions(eng._h, C.c_void_p(st.data_ptr() + 8), N.CAP_PIX_IMAGE_STATE, NIMG, C.c_void_p(ids.data_ptr()),
                                       C.c_void_p(lens.data_ptr()), 1, L, C.c_void_p(sc.data_ptr()), C.c_void_p(sc.data_ptr()),
                                       C.c_void_p(ids.data_ptr()), C.c_void_p(lens.data_ptr()), s), "cap_score_captions", "16-byte aligned")
        torch.cuda.synchronize()
        assert eng.profile_report() == {}          # nothing was launched
    finally:
        eng.profile(False)
    assert bool((ids == -7).all()) and bool((lens == -7).all()) and bool((emb == -7.0).all()) and bool((sc == -7.0).all())
    assert torch.equal(big, st[[0] * (BM + 1)])
    # a sentence encoder has no image state
    tarch = Cf.MiniLMArch.tiny()
    te = E.TextEncoderEngine(tarch, dtype="f32", max_batch=2, max_len=8)
    try:
        assert lib.cap_image_state_bytes(te._h) == 0
        msg = lib.cap_last_error().decode()
        assert "cap_image_state_bytes" in msg and "BLIP" in msg
        assert lib.cap_image_state_bytes(None) == 0 and "null handle" in lib.cap_last_error().decode()
    finally:
        te.close()


# ------------------------------------------------------------------------------------------------ wrappers
def test_blip_wrapper_generates_and_scores_from_its_image_state():
    from embodied_captioning_amd.captioner.likelihood_scorer import CaptionLikelihoodScorer
    from embodied_captioning_amd.utils.predictor_utils import Captioner
    cfg = types.SimpleNamespace(arch_name="blip", model_name="procedural-tiny:4:2.0", checkpoint_name=None, height=224, width=224,
                                batch_size=2, num_beams=1, max_length=L, max_score_rows=44, early_exit_poll=0)
    model = Captioner(types.SimpleNamespace(captioner=cfg)).eval().model
    try:
        crops = torch.from_numpy(np.random.default_rng(9).integers(0, 256, size=(3, 40, 52, 3), dtype=np.uint8))          # resized on the way in
        caps = [[model.arch.bos, 120, 131, 142, model.arch.eos], [model.arch.bos, 150, 161], [model.arch.bos, 170, 181, 192]]
        st = model.image_state(crops)
        assert st.dtype == torch.uint8 and tuple(st.shape) == (3, model.engine.image_state_bytes)
        a, b = model.generate_batch(crops, output_perplexity=True), model.generate_batch(image_state=st, output_perplexity=True)
        assert a["texts"] == b["texts"] and torch.equal(a["sequences"], b["sequences"]) and torch.equal(a["lengths"], b["lengths"])
        assert same_bits(a["token_logprobs"], b["token_logprobs"]) and torch.equal(a["perplexities"], b["perplexities"])
        sub = model.generate_batch(image_state=st[[2, 0]])
        assert sub["texts"] == [a["texts"][2], a["texts"][0]]
        sa, sb = model.score_captions(crops, caps), model.score_captions(image_state=st, captions=caps)
        assert same_bits(sa["token_logprobs"], sb["token_logprobs"]) and torch.equal(sa["top_ids"], sb["top_ids"])
        assert torch.equal(sa["logprob_mean"], sb["logprob_mean"])
        scorer = CaptionLikelihoodScorer(model=model)
        assert torch.equal(scorer.score_matrix(crops, caps), scorer.score_matrix(st, caps))
        with pytest.raises(ValueError, match="one of the two"):
            model.generate_batch(crops, image_state=st)
        with pytest.raises(ValueError, match="one of the two"):
            model.generate_batch()
    finally:
        model.engine.close()
