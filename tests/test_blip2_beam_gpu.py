"""GPU: beam search for BLIP-2 OPT through the C ABI and the Python layers - against the HF golden (tests/golden/blip2_tiny_beam.npz),
against the fp64 beam search over the restatement (tests/_blip2_beam_ref.py), and against itself: a caption's bits depend neither on
the batch it is in nor on the handle's beam capacity."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from embodied_captioning_amd import _native as N
from test_blip2_beam_cpu import KEYS, case_inputs, load_beam_golden

pytestmark = pytest.mark.gpu

I_FILL, F_FILL = -7, 123.5          # what every output buffer of a refused request holds before the call


def _tiny():
    from embodied_captioning_amd.config import Blip2Arch
    return Blip2Arch.tiny()


@functools.lru_cache(maxsize=None)
def _weights(seed, eos_boost):
    from embodied_captioning_amd.weights import procedural_blip2_state_dict
    return procedural_blip2_state_dict(_tiny(), seed, eos_boost=eos_boost)


def _engine(arch, sd, dtype, batch, beams, int8=False):
    from embodied_captioning_amd.engine import CaptionerEngine
    eng = CaptionerEngine(arch, dtype=dtype, max_batch=batch, max_beams=beams, max_len=arch.max_new_tokens, weight_int8=int8)
    eng.load_state_dict(sd)
    return eng


def _host(out):
    return {k: v.cpu() for k, v in out.items()}


# ---------------------------------------------------------------------------------------------- HF golden
@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("dtype", ["f32", "f32s"])
def test_tiny_beams_match_the_hf_golden(dtype, key):
    """Tokens and lengths identical to HF on every image the file does not list as omitted (fp64 decision gap below 1e-3).
    sequences_scores within 2e-3 (the bar tests/test_configs_gpu.py holds BLIP's beam-3 golden to) on every image that returns HF's
    hypothesis: all the kept ones, and an omitted one unless its near-tie went the other way - it then returns ANOTHER hypothesis,
    whose score is not the quantity HF's number measures (it may lie anywhere below; nothing bounds the two scores' distance)."""
    g, meta = load_beam_golden()
    a, sd, px, K, lp = case_inputs(meta, key)
    eng = _engine(a, sd, dtype, meta["batch"], K)
    out = _host(eng.generate(px.cuda(), num_beams=K, length_penalty=lp, max_length=a.max_new_tokens))
    eng.close()
    keep = np.setdiff1d(np.arange(meta["batch"]), g[f"omit_{key}"])
    want = g[f"ids_{key}"]
    want_len = np.array([int(np.argmax(r == a.eos)) + 1 if (r == a.eos).any() else r.size for r in want])
    got, got_len, sc = out["sequences"].numpy(), out["lengths"].numpy(), out["sequences_scores"].numpy()
    print(key, dtype, "score error", np.abs(sc - g[f"scores_{key}"]), "gaps", g[f"gap_{key}"])
    assert np.array_equal(got[keep], want[keep]), (got, want)
    assert np.array_equal(got_len[keep], want_len[keep])
    scored = np.array([b for b in range(meta["batch"]) if np.array_equal(got[b], want[b])])
    assert set(keep) <= set(scored)
    assert np.abs(sc[scored] - g[f"scores_{key}"][scored]).max() < 2e-3


# ---------------------------------------------------------------------------------------------- invariances (exact)
@pytest.mark.parametrize("mode", ["f32s", "bf16", "bf16-int8"])
def test_a_caption_does_not_depend_on_its_batch_or_on_the_beam_capacity(mode):
    """int8 weights: the fixture whose OPT widths the int8 weight stream takes (tests/test_blip2_int8_gpu.py), 4 crops per call at the
    most - up to there the int8 prompt pass keeps one kernel."""
    from embodied_captioning_amd.weights import procedural_blip2_state_dict, synthetic_pixels
    dtype, int8 = mode.split("-")[0], mode.endswith("int8")
    if int8:
        from test_blip2_int8_gpu import _small_arch
        a = _small_arch()
        sd = procedural_blip2_state_dict(a, 5, eos_boost=0.3)
    else:
        a, sd = _tiny(), _weights(11, 0.5)
    px = synthetic_pixels(4, a.image_size, seed=11).cuda()
    n = a.max_new_tokens
    e3 = _engine(a, sd, dtype, 4, 3, int8)
    whole = _host(e3.generate(px, num_beams=3, max_length=n))
    same = lambda x, y, rows=slice(None): all(torch.equal(x[k][rows], y[k]) for k in ("sequences", "lengths", "sequences_scores"))  # noqa: E731
    # alone and inside the batch of 4
    for b in (0, 2):
        assert same(whole, _host(e3.generate(px[b:b + 1], num_beams=3, max_length=n)), slice(b, b + 1)), b
    # permuting the images permutes the results
    perm = [2, 0, 3, 1]
    assert same(whole, _host(e3.generate(px[perm], num_beams=3, max_length=n)), perm)
    # a handle with room for 5 beams serving 3
    e5 = _engine(a, sd, dtype, 4, 5, int8)
    assert same(whole, _host(e5.generate(px, num_beams=3, max_length=n)))
    e5.close()
    # the greedy loop of a beam handle is the greedy loop
    e1 = _engine(a, sd, dtype, 4, 1, int8)
    g1, g3 = _host(e1.generate(px, max_length=n)), _host(e3.generate(px, max_length=n))
    assert torch.equal(g1["sequences"], g3["sequences"]) and torch.equal(g1["lengths"], g3["lengths"])
    e1.close()
    e3.close()


# ---------------------------------------------------------------------------------------------- production head width
def test_heads_of_80_against_the_fp64_beam_search():
    """The arch of tests/test_blip2_gpu.py::test_blip2_real_head_dims_against_restatement (ViT heads 88, OPT heads 80 -> the HD8 = 10
    form of the attention), K = 3, B = 2, "f32".  Seed 6 was chosen on the CPU: fp64 decision gaps 8.2e-3 and 1.1e-2."""
    from embodied_captioning_amd.config import Blip2Arch
    from embodied_captioning_amd.weights import procedural_blip2_state_dict, synthetic_pixels
    import _blip2_beam_ref as BR
    a = Blip2Arch(image_size=42, patch_size=14, v_hidden=704, v_layers=2, v_heads=8, v_mlp=1408, q_hidden=128, q_layers=3, q_heads=2,
                  q_ffn=256, num_query_tokens=6, t_hidden=320, t_layers=2, t_heads=4, t_ffn=640, vocab=1000, max_pos=64, eos=3,
                  image_token=999, max_new_tokens=8)
    sd = procedural_blip2_state_dict(a, 6, eos_boost=0.4)
    px = synthetic_pixels(2, a.image_size, seed=6)
    ref = BR.beam_search(sd, a, px, 3, 1.0, dtype=np.float64)
    ok = ref["gap"] > 1e-3
    assert ok.all(), ref["gap"]
    assert ref["reorders"] >= 3
    eng = _engine(a, sd, "f32", 2, 3)
    out = _host(eng.generate(px.cuda(), num_beams=3, max_length=a.max_new_tokens))
    eng.close()
    print("score error", np.abs(out["sequences_scores"].numpy() - ref["scores"]), "gaps", ref["gap"])
    assert np.array_equal(out["sequences"].numpy()[ok], ref["ids"][ok])
    assert np.array_equal(out["lengths"].numpy()[ok], ref["lens"][ok])
    assert np.abs(out["sequences_scores"].numpy()[ok] - ref["scores"][ok]).max() < 2e-3


# ---------------------------------------------------------------------------------------------- early exit, per-step logits
def test_early_exit_leaves_the_beam_loop_with_the_same_results():
    from embodied_captioning_amd.weights import synthetic_pixels
    a, sd = _tiny(), _weights(2, 12.0)
    px = synthetic_pixels(4, a.image_size, seed=4).cuda()
    eng = _engine(a, sd, "f32", 4, 3)
    res = []
    for poll in (0, 1):
        eng.set_early_exit(poll)
        res.append((_host(eng.generate(px, num_beams=3, max_length=a.max_new_tokens)), eng.last_decode_steps))
    eng.close()
    (x, sx), (y, sy) = res
    assert sx == a.max_new_tokens and sy < a.max_new_tokens, (sx, sy)
    assert all(torch.equal(x[k], y[k]) for k in ("sequences", "lengths", "sequences_scores"))


def test_per_step_logits_of_a_beam_search():
    from embodied_captioning_amd.weights import synthetic_pixels
    a, sd = _tiny(), _weights(11, 0.5)
    B, K, n = 3, 3, a.max_new_tokens
    px = synthetic_pixels(B, a.image_size, seed=11).cuda()
    eng = _engine(a, sd, "f32s", B, K)
    beams = eng.generate(px, num_beams=K, max_length=n, output_logits=True)["logits"].cpu()
    greedy = eng.generate(px, max_length=n, output_logits=True)["logits"].cpu()
    eng.close()
    assert beams.shape == (n, B * K, a.vocab) and greedy.shape == (n, B, a.vocab)
    step0 = beams[0].view(B, K, a.vocab)
    for k in range(K):          # the prompt pass ran once per image: its K rows are copies, and they are the greedy call's bits
        assert torch.equal(step0[:, k], greedy[0])
    assert not torch.equal(beams[1].view(B, K, a.vocab)[:, 0], beams[1].view(B, K, a.vocab)[:, 1])      # later rows are beams of their own


# ---------------------------------------------------------------------------------------------- requests
def _buffers(eng, B, rows, steps, cols, max_len, acc_ld=516):
    i32 = lambda *s: torch.full(s, I_FILL, dtype=torch.int32, device="cuda")          # noqa: E731
    f32 = lambda *s: torch.full(s, F_FILL, dtype=torch.float32, device="cuda")        # noqa: E731
    return {"out_ids": i32(B, max_len), "out_len": i32(B), "out_scores": f32(B), "out_step_logits": f32(steps, rows, eng.arch.vocab),
            "out_logprobs": f32(B, cols), "out_scored": i32(B), "out_vocab": f32(B, acc_ld)}


BASE = ("out_ids", "out_len", "out_scores")
REFUSED = {
    "prompt": (BASE, {"prompt": True}, "text prompt"),
    "out_logprobs": (BASE + ("out_logprobs", "out_scored"), {}, "per-step log-probs are the greedy loop's"),
    "out_vocab": (BASE + ("out_logprobs", "out_scored", "out_vocab"), {}, "greedy loop's"),
    "num_beam_groups": (BASE, {"num_beam_groups": 3}, "beam groups are the CoCa loop's"),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_a_refused_beam_request_launches_nothing(case):
    from embodied_captioning_amd.weights import synthetic_pixels
    a, sd = _tiny(), _weights(11, 0.5)
    B, K, n = 2, 3, a.max_new_tokens
    use, fields, word = REFUSED[case]
    eng = _engine(a, sd, "f32s", B, K)
    px = synthetic_pixels(B, a.image_size, seed=11).cuda()
    bufs = _buffers(eng, B, B * K, 1, n, n)
    req = N.CapGenerateArgs(pixels=px.data_ptr(), pixel_fmt=N.CAP_PIX_F32_NCHW, B=B, num_beams=K, max_len=n, length_penalty=1.0)
    for name in use:
        setattr(req, name, bufs[name].data_ptr())
    if "out_vocab" in use:
        req.acc_ld = bufs["out_vocab"].shape[1]
    fields = dict(fields)
    if fields.pop("prompt", False):
        prompt = torch.tensor([[a.bos, 11, 12]], dtype=torch.int32, device="cuda")
        req.prompt_ids, req.prompt_rows, req.prompt_len = prompt.data_ptr(), 1, 3
    for k, v in fields.items():
        setattr(req, k, v)
    before = eng.last_decode_steps
    rc = eng.lib.cap_generate_request(eng._h, C.byref(req), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    msg = N.last_error()
    torch.cuda.synchronize()
    assert rc != 0 and "cap_generate_request:" in msg and word in msg, (rc, msg)
    assert eng.last_decode_steps == before
    for name, t in bufs.items():
        assert bool((t == (I_FILL if t.dtype == torch.int32 else F_FILL)).all()), name
    eng.close()


def test_a_handle_takes_one_to_eight_beams():
    from embodied_captioning_amd.engine import CaptionerEngine
    with pytest.raises(N.CaptionerHipError, match="max_beams"):
        CaptionerEngine(_tiny(), dtype="f32s", max_batch=2, max_beams=9, max_len=8)


# ---------------------------------------------------------------------------------------------- the plugin class
def test_wrapper_reads_num_beams_and_the_pool_returns_the_single_engine_ids():
    from PIL import Image
    from embodied_captioning_amd.captioner.utils.utils import Configuration
    from embodied_captioning_amd.captioner.utils.utils_captioner import select_captioner
    rng = np.random.default_rng(0)
    ims = [Image.fromarray(rng.integers(0, 256, size=(50, 41, 3), dtype=np.uint8), "RGB") for _ in range(6)]
    kw = dict(arch_name="blip2", model_name="procedural-blip2-tiny:11:0.5", height=224, width=224, dtype="f32s", num_beams=3, batch_size=2)
    one = select_captioner(Configuration(**kw).captioner).eval()
    assert one.num_beams == 3 and one.length_penalty == 1.0 and one.engine.max_beams == 3
    out = one(ims[0])
    assert isinstance(out["text"], str) and isinstance(out["sequences_scores"], float)
    assert 1 <= len(out["logits"]) <= one.arch.max_new_tokens and out["logits"][0].shape == (3, one.arch.vocab)
    single = one.generate_batch(ims)
    assert single["texts"][0] == out["text"] and single["scores"].shape == (6,)
    pooled = select_captioner(Configuration(streams=2, **kw).captioner).eval()
    assert pooled.pool is not None
    many = pooled.generate_batch(ims)
    assert torch.equal(many["sequences"], single["sequences"]) and torch.equal(many["lengths"], single["lengths"])
    assert torch.equal(many["scores"], single["scores"])
    # captioner.length_penalty through the configuration object: forward, generate_batch and the pool give what the engine gives
    # when it is handed the penalty, and not what it gives without
    lp2 = select_captioner(Configuration(streams=2, length_penalty=2.0, **kw).captioner).eval()
    assert lp2.length_penalty == 2.0 and lp2.pool is not None
    px = lp2.preprocess(ims).to(lp2.device)
    want = [_host(lp2.engine.generate(px[i:i + 2], num_beams=3, length_penalty=2.0, max_length=lp2.max_length)) for i in (0, 2, 4)]
    want = {k: torch.cat([w[k] for w in want]) for k in ("sequences", "lengths", "sequences_scores")}
    plain = torch.cat([_host(lp2.engine.generate(px[i:i + 2], num_beams=3, max_length=lp2.max_length))["sequences_scores"] for i in (0, 2, 4)])
    assert torch.equal(plain, single["scores"]) and not torch.equal(want["sequences_scores"], plain)
    many2 = lp2.generate_batch(ims)                          # six crops in micro-batches of two: the pool
    assert torch.equal(many2["sequences"], want["sequences"]) and torch.equal(many2["lengths"], want["lengths"])
    assert torch.equal(many2["scores"], want["sequences_scores"])
    two = lp2.generate_batch(ims[:2])                        # one micro-batch: the wrapper's own engine
    assert torch.equal(two["sequences"], want["sequences"][:2]) and torch.equal(two["scores"], want["sequences_scores"][:2])
    fwd = lp2(ims[0])
    alone = _host(lp2.engine.generate(px[:1], num_beams=3, length_penalty=2.0, max_length=lp2.max_length))
    assert fwd["sequences_scores"] == float(alone["sequences_scores"][0])
    assert fwd["text"] == lp2.decode(alone["sequences"][0, :int(alone["lengths"][0])].tolist())
    with pytest.raises(N.CaptionerHipError, match="greedy loop's"):
        one.generate_batch(ims[:2], output_perplexity=True)
    with pytest.raises(N.CaptionerHipError, match="output_vocab_maxprob is the greedy loop's"):
        one.generate_batch(ims[:2], output_vocab_maxprob=True)
