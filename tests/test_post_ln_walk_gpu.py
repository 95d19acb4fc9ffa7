"""GPU: the shape of the post-LN encoder walks - the sentence encoder, the BLIP-2 Q-Former, the image-text scorer's Q-Former with
text rows - read off the engine's own profile tags at the tiny architectures, and the same walks on a handle that shares another
handle's weights (cap_create_shared replays the build's buffer sequence).  The expected launch counts follow from the arch fields:
one chain per layer and row set, the cross-attention chain on every q_cross_freq-th layer."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B = 3


def _n_cross(a):
    return sum(1 for i in range(a.q_layers) if i % a.q_cross_freq == 0)


def _text(vocab, L, seed):
    """ids int32 [B, L], ragged lens (the first row full)"""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, vocab, (B, L), generator=g, dtype=torch.int32)
    lens = torch.tensor([L, 3, L - 2], dtype=torch.int32)
    return ids, lens


def _launches(eng, call, prefix):
    """the launches per tag (of the tags that start with `prefix`) `call` records, and what it returns"""
    eng.profile(True)
    out = call()
    rep = eng.profile_report()
    eng.profile(False)
    return {t: rep[t]["launches"] for t in rep if t.startswith(prefix)}, out


def _check_sharing(first, own, make_shared, run):
    """`run(engine)` -> tuple of tensors: the same bits on the handle that shares `first`'s weights; arena + weights add up"""
    shared = make_shared(first)
    other = make_shared(first)
    for x, y in zip(run(first), run(shared)):
        assert torch.equal(x, y)
    assert shared.device_bytes == other.device_bytes < first.device_bytes
    assert own.device_bytes == first.device_bytes
    for e in (shared, other, own, first):
        e.close()


def test_minilm_embed_is_one_chain_per_layer():
    from embodied_captioning_amd.config import MiniLMArch
    from embodied_captioning_amd.engine import TextEncoderEngine
    from embodied_captioning_amd.weights import procedural_minilm_state_dict
    a = MiniLMArch.tiny()
    L = 9
    ids, lens = _text(a.vocab, L, 1)
    sd = procedural_minilm_state_dict(a, 4)
    eng = TextEncoderEngine(a, dtype="f32", max_batch=B, max_len=L)
    eng.load_state_dict(sd)
    got, _ = _launches(eng, lambda: eng.embed(ids, lens), "te_")
    print(got)
    want = {t: a.layers for t in ("te_gemm_qkv", "te_attention", "te_gemm_o", "te_gemm_f1", "te_gemm_f2")}
    assert got == dict(want, te_layernorm=2 * a.layers, te_embed=1, te_pool=1)
    own = TextEncoderEngine(a, dtype="f32", max_batch=B, max_len=L)
    own.load_state_dict(sd)
    _check_sharing(eng, own, lambda f: TextEncoderEngine(a, dtype="f32", max_batch=B, max_len=L, share_weights_with=f),
                   lambda e: (e.embed(ids, lens),))


def test_blip2_generate_runs_the_qformer_once_per_layer():
    from embodied_captioning_amd.config import Blip2Arch
    from embodied_captioning_amd.engine import CaptionerEngine
    from embodied_captioning_amd.weights import procedural_blip2_state_dict, synthetic_pixels
    a = Blip2Arch.tiny()
    n = 4
    kw = dict(dtype="f32s", max_batch=B, max_beams=1, max_len=n)
    sd = procedural_blip2_state_dict(a, 5, eos_boost=0.3)
    px = synthetic_pixels(B, a.image_size, seed=5).cuda()
    eng = CaptionerEngine(a, **kw)
    eng.load_state_dict(sd)
    got, _ = _launches(eng, lambda: eng.generate(px, max_length=n), "qf_")
    print(got)
    want = {t: a.q_layers for t in ("qf_gemm_qkv", "qf_self_attn", "qf_gemm_so", "qf_gemm_f1", "qf_gemm_f2")}
    want.update({t: _n_cross(a) for t in ("qf_gemm_cq", "qf_gemm_ckv", "qf_cross_attn", "qf_gemm_co")})
    assert got == want
    own = CaptionerEngine(a, **kw)
    own.load_state_dict(sd)

    def run(e):
        out = e.generate(px, max_length=n, output_logits=True)
        return out["sequences"], out["lengths"], out["logits"]
    _check_sharing(eng, own, lambda f: CaptionerEngine(a, share_weights_with=f, **kw), run)


def test_itm_calls_walk_the_row_sets_they_have():
    from embodied_captioning_amd.config import Blip2ItmArch
    from embodied_captioning_amd.engine import Blip2ItmEngine
    from embodied_captioning_amd.weights import procedural_blip2_itm_state_dict, synthetic_frames_u8
    a = Blip2ItmArch.tiny()
    L = 11
    ids, lens = _text(a.vocab, L, 2)
    sd = procedural_blip2_itm_state_dict(a, 6)
    frames = synthetic_frames_u8(B, a.image_size, a.image_size, seed=6)
    kw = dict(dtype="f32s", max_batch=B, max_len=L)
    eng = Blip2ItmEngine(a, **kw)
    eng.load_state_dict(sd)
    nl, nc = a.q_layers, _n_cross(a)
    q_set = {t: nl for t in ("itm_gemm_qkv_q", "itm_gemm_so_q", "itm_gemm_f1_q", "itm_gemm_f2_q")}
    t_set = {t: nl for t in ("itm_gemm_qkv_t", "itm_gemm_so_t", "itm_gemm_f1_t", "itm_gemm_f2_t")}
    cross = {t: nc for t in ("itm_gemm_cq", "itm_cross_attn", "itm_gemm_co")}

    got, _ = _launches(eng, lambda: eng.encode_images(frames), "itm_")
    print("encode_images", got)
    assert got == {"itm_gemm_ckv": nc}
    got, _ = _launches(eng, eng.itc_image_features, "itm_")
    print("itc_image_features", got)
    assert got == dict(q_set, itm_self_attn=nl, **cross)
    got, _ = _launches(eng, lambda: eng.itc_text_features(ids, lens), "itm_")
    print("itc_text_features", got)
    assert got == dict(t_set, itm_self_attn=nl, itm_embed_text=1)
    got, _ = _launches(eng, lambda: eng.itm(ids, lens), "itm_")
    print("itm", got)
    assert got == dict(q_set, **t_set, **cross, itm_self_attn=nl, itm_embed_text=1, itm_head=1)

    own = Blip2ItmEngine(a, **kw)
    own.load_state_dict(sd)

    def run(e):
        e.encode_images(frames)
        img, txt = e.itc_image_features(), e.itc_text_features(ids, lens)
        return (img, txt, e.itc_scores(img, txt), e.itc_scores(img, txt, paired=False)) + tuple(e.itm(ids, lens))
    _check_sharing(eng, own, lambda f: Blip2ItmEngine(a, share_weights_with=f, **kw), run)
