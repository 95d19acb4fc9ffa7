"""GPU: teacher-forced scoring of given captions under BLIP-2 (`CaptionerEngine.score` on a Blip2Arch engine: the prompt pass once per
image, the caption pass behind the cached prompt through opt_prefix_attention) on the procedural tiny / small fixtures, against the
float32 / float64 restatement (tests/_score_ref.py::blip2_score on oracle/blip2_ref.py).

* "f32" / "f32s": every live token log-prob within 2e-3, top_ids equal wherever the restatement's top-2 margin exceeds 2e-3;
* "bf16" and `load_in_8bit` (Blip2Arch.small(), against the restatement on the dequantised int8 weights, as tests/test_blip2_int8_gpu.py
  compares): no absolute bar - top_ids agree wherever the fp32 restatement's margin exceeds 0.05; the measured maximum is printed;
* own captions: `generate(output_logprobs=True)` then `score` of the returned tokens behind BOS;
* the same bits for a pair alone, in a batch, as a candidate slot, under every chunking of the passes; padding never leaks;
* refusals; generate / score / generate; the wrapper."""
import numpy as np
import pytest
import torch

from _score_ref import blip2_score, random_captions

pytestmark = pytest.mark.gpu

KEYS = ("token_logprobs", "top_logprobs", "top_ids", "scored")
B, C, L = 4, 3, 12


def _fixture(arch, seed, quantised=False):
    from oracle import blip2_ref as R2
    from embodied_captioning_amd.weights import procedural_blip2_state_dict, synthetic_pixels
    sd = procedural_blip2_state_dict(arch, seed, eos_boost=0.3)
    px = synthetic_pixels(B, arch.image_size, seed=seed)
    ids = random_captions(arch, B * C, L, None, seed=seed)
    lens = np.array([2, 6, L, 3, 0, L, 2, 9, L, L, 5, 0], dtype=np.int32)              # lengths 2, middle, L; two absent slots
    for n in (2, 8):
        ids[n, L - 1] = arch.eos                                                         # the generation EOS as a last token
    ref_sd = R2.int8_state_dict(sd) if quantised else sd
    return dict(arch=arch, sd=sd, px=px, ids=ids, lens=lens, ref32=blip2_score(ref_sd, arch, px, ids, lens, C, torch.float32),
                ref64=blip2_score(ref_sd, arch, px, ids, lens, C, torch.float64))


@pytest.fixture(scope="module")
def tiny():
    from embodied_captioning_amd.config import Blip2Arch
    return _fixture(Blip2Arch.tiny(), 3)


@pytest.fixture(scope="module")
def small_q8():
    from embodied_captioning_amd.config import Blip2Arch
    return _fixture(Blip2Arch.small(), 5, quantised=True)


def _engine(fx, dtype, batch=B, beams=1, **kw):
    from embodied_captioning_amd.engine import CaptionerEngine
    eng = CaptionerEngine(fx["arch"], dtype=dtype, max_batch=batch, max_beams=beams, max_len=L - 1, **kw)
    eng.load_state_dict(fx["sd"])
    return eng


def _cpu(out):
    return {k: out[k].cpu() for k in KEYS}


def _same(a, b, rows_a=slice(None), rows_b=slice(None)):
    return all(torch.equal(a[k][rows_a], b[k][rows_b]) for k in KEYS)


def _check_shape_and_zeros(fx, out):
    live = fx["ref64"]["live"]
    assert tuple(out["token_logprobs"].shape) == (B * C, L - 1)
    assert np.array_equal(out["scored"].numpy(), np.maximum(fx["lens"] - 1, 0))
    for k in KEYS[:3]:
        assert float(np.abs(out[k].numpy()[~live]).max()) == 0.0, k
    return live


@pytest.mark.parametrize("dtype", ["f32", "f32s"])
def test_blip2_token_logprobs_against_float64(tiny, dtype):
    eng = _engine(tiny, dtype)
    out = _cpu(eng.score(tiny["px"].cuda(), tiny["ids"], tiny["lens"], captions_per_image=C))
    eng.close()
    live = _check_shape_and_zeros(tiny, out)
    ref = tiny["ref64"]
    err = np.abs(out["token_logprobs"].double().numpy() - ref["token_logprobs"])[live].max()
    err_top = np.abs(out["top_logprobs"].double().numpy() - ref["top_logprobs"])[live].max()
    print(f"score blip2-tiny {dtype} against float64 restatement: max |d token log-prob| {err:.3e}, top {err_top:.3e}")
    assert err <= 2e-3 and err_top <= 2e-3
    sure = live & (ref["margin"] > 2e-3)
    assert sure.sum() >= 0.9 * live.sum()
    assert np.array_equal(out["top_ids"].numpy()[sure], ref["top_ids"][sure])
    assert bool((out["token_logprobs"] <= out["top_logprobs"]).all())


@pytest.mark.parametrize("mode", ["bf16", "load_in_8bit"])
def test_blip2_reduced_precision_top_ids_and_measured_error(tiny, small_q8, mode):
    fx = small_q8 if mode == "load_in_8bit" else tiny
    eng = _engine(fx, "bf16", weight_int8=mode == "load_in_8bit")
    out = _cpu(eng.score(fx["px"].cuda(), fx["ids"], fx["lens"], captions_per_image=C))
    eng.close()
    live = _check_shape_and_zeros(fx, out)
    sure = live & (fx["ref32"]["margin"] > 0.05)
    assert sure.sum() >= 0.7 * live.sum()                                            # known from the CPU restatement alone: 49 / 61 of 65
    assert np.array_equal(out["top_ids"].numpy()[sure], fx["ref32"]["top_ids"][sure])
    err = np.abs(out["token_logprobs"].double().numpy() - fx["ref64"]["token_logprobs"])[live]
    print(f"score blip2 {mode}: max |d token log-prob| against float64 {err.max():.3e} (mean {err.mean():.3e}), "
          f"{int(sure.sum())} of {int(live.sum())} positions above the 0.05 margin")


def test_blip2_scoring_a_generated_caption_reproduces_the_greedy_call(tiny):
    arch, px = tiny["arch"], tiny["px"].cuda()
    eng = _engine(tiny, "f32s")
    gen = eng.generate(px, max_length=L - 1, output_logprobs=True)
    new, glen, glp = gen["sequences"].cpu(), gen["lengths"].cpu(), gen["token_logprobs"].cpu()
    ids = torch.cat([torch.full((B, 1), arch.bos, dtype=torch.int32), new], 1)       # BOS + the new tokens
    lens = glen + 1
    out = _cpu(eng.score(px, ids, lens))
    eng.close()
    ref = blip2_score(tiny["sd"], arch, tiny["px"], ids.numpy(), lens.numpy(), 1, torch.float32)
    sure = ref["live"] & (ref["margin"] > 4e-3)
    assert sure.sum() >= 0.9 * ref["live"].sum()
    assert torch.equal(out["scored"], gen["scored_steps"].cpu())
    n = 0
    for r, j in zip(*np.nonzero(sure)):
        if int(ref["top_ids"][r, j]) != int(ids[r, j + 1]):
            break                                                                      # the device left the restatement's path at a near-tie
        assert int(out["top_ids"][r, j]) == int(ids[r, j + 1]), (r, j)
        assert float(out["token_logprobs"][r, j]) == float(out["top_logprobs"][r, j]), (r, j)
        assert abs(float(out["token_logprobs"][r, j]) - float(glp[r, j])) <= 4e-3, (r, j)
        n += 1
    d = (out["token_logprobs"] - glp).abs()[torch.from_numpy(ref["live"])].max()
    print(f"own captions blip2 f32s: {n} positions compared, max |score - generate| over all live positions {float(d):.3e}")
    assert n >= 0.8 * sure.sum()


@pytest.mark.parametrize("dtype", ["f32s", "bf16"])
def test_blip2_same_bits_alone_batched_as_a_slot_and_under_every_chunking(tiny, dtype):
    px, ids, lens = tiny["px"].cuda(), tiny["ids"], tiny["lens"]
    big = _engine(tiny, dtype, batch=16)                                               # 16 x 9 pass rows: 12 captions x 10 positions at once
    base = _cpu(big.score(px, ids, lens, captions_per_image=C))
    assert big.last_score_passes == 1
    small = _engine(tiny, dtype, batch=4)                                              # 36 pass rows: 3 captions (one image) per pass
    got = _cpu(small.score(px, ids, lens, captions_per_image=C))
    assert small.last_score_passes == 4 and _same(base, got)
    tight = _engine(tiny, dtype, batch=2)                                              # 18 rows: one caption per pass, two images per call
    got = _cpu(tight.score(px, ids, lens, captions_per_image=C))
    assert tight.last_score_passes == 6 and _same(base, got)
    pair_px = px.repeat_interleave(C, dim=0)
    keep = [n for n in range(B * C) if lens[n] > 0]
    for n in (1, 2, 10):
        alone = _cpu(small.score(pair_px[n:n + 1], ids[n:n + 1], lens[n:n + 1]))
        assert _same(base, alone, slice(n, n + 1)), (dtype, n)
    for sort in (True, False):
        pairs = _cpu(small.score(pair_px[keep], ids[keep], lens[keep], sort_by_length=sort))
        assert _same(base, pairs, keep), (dtype, sort)
    # padding and the contents of absent slots never leak
    other = random_captions(tiny["arch"], B * C, L, None, seed=77)
    ids2 = ids.copy()
    for n in range(B * C):
        ids2[n, lens[n]:] = other[n, lens[n]:]
    assert not np.array_equal(ids, ids2) and _same(base, _cpu(small.score(px, ids2, lens, captions_per_image=C)))
    for e in (big, small, tight):
        e.close()


def test_blip2_refusals_state_and_wrapper(tiny):
    import types
    arch, px, ids, lens = tiny["arch"], tiny["px"].cuda(), tiny["ids"], tiny["lens"]
    eng = _engine(tiny, "f32s")
    pair_ids, pair_lens = ids[[2, 5, 8, 9]], lens[[2, 5, 8, 9]]                          # the four full-length captions
    with pytest.raises(ValueError, match="too long"):
        eng.score(px, random_captions(arch, B, L + 1, None, seed=1), np.full(B, L + 1))
    with pytest.raises(ValueError, match="BOS"):
        eng.score(px, pair_ids[:, ::-1].copy(), pair_lens)
    a = {k: v.clone() for k, v in eng.generate(px, max_length=L - 1, output_logprobs=True).items()}
    eng.score(px, ids, lens, captions_per_image=C)
    b = eng.generate(px, max_length=L - 1, output_logprobs=True)
    assert all(torch.equal(a[k], b[k]) for k in a)
    eng.close()
    long_eng = _engine(tiny, "f32s", batch=1)                                          # 9 pass rows: a caption of 12 tokens needs 10
    with pytest.raises(ValueError, match="max_batch"):
        long_eng.score(px[:1], pair_ids[:1], pair_lens[:1])
    long_eng.close()
    # the wrapper: BOS put in front, candidates per image, agreement with engine.score
    from embodied_captioning_amd.utils.predictor_utils import Captioner
    cfg = types.SimpleNamespace(arch_name="blip2", model_name="procedural-blip2-tiny:1", checkpoint_name=None, height=224, width=224,
                                batch_size=2, max_new_tokens=8)
    cap = Captioner(types.SimpleNamespace(captioner=cfg)).eval()
    model = cap.model
    crops = torch.zeros((2, model.arch.image_size, model.arch.image_size, 3), dtype=torch.uint8)
    crops[1] += 90
    caps = [[model.arch.bos, 31, 47, 59, model.arch.eos], [31, 47]]
    out = cap.score_batch(crops, caps)
    assert out["n_tokens"].tolist() == [4, 2] and tuple(out["token_logprobs"].shape) == (2, 4)
    ids2 = np.full((2, 5), model.arch.pad, dtype=np.int32)
    ids2[0] = caps[0]
    ids2[1, :3] = [model.arch.bos] + caps[1]
    direct = model.engine.score(model.preprocess(crops).to(model.device), ids2, [5, 3])
    assert torch.equal(out["token_logprobs"], direct["token_logprobs"].cpu())
    cands = model.score_captions(crops, [[caps[0], caps[1]], [caps[1]]])
    assert cands["n_tokens"].tolist() == [4, 2, 2, 0] and torch.equal(cands["token_logprobs"][2], out["token_logprobs"][1])
    assert abs(float(out["perplexity"][0]) - float(torch.exp(-out["token_logprobs"][0, :4].double().mean()))) <= 1e-9
    model.engine.close()


@pytest.mark.parametrize("dtype", ["f32", "f32s"])
def test_blip2_token_logprobs_against_the_hf_golden(dtype):
    """tests/golden/blip2_tiny_score.npz: HF `Blip2ForConditionalGeneration(pixel_values, input_ids=...)` logits reduced in float64
    (tools/make_goldens_score.py); row 1 is HF's own greedy caption with its EOS."""
    import json
    import os
    from embodied_captioning_amd.config import Blip2Arch
    from embodied_captioning_amd.engine import CaptionerEngine
    from embodied_captioning_amd.weights import procedural_blip2_state_dict, synthetic_pixels
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "blip2_tiny_score.npz"))
    meta = json.loads(str(g["meta"]))
    arch = Blip2Arch(**meta["arch"])
    sd = procedural_blip2_state_dict(arch, meta["seed"], eos_boost=meta["eos_boost"])
    px = synthetic_pixels(meta["batch"], arch.image_size, seed=meta["seed"])
    ids, lens, Cn = g["ids"], g["lens"], meta["captions_per_image"]
    eng = CaptionerEngine(arch, dtype=dtype, max_batch=meta["batch"], max_beams=1, max_len=ids.shape[1] - 1)
    eng.load_state_dict(sd)
    out = _cpu(eng.score(px.cuda(), ids, lens, captions_per_image=Cn))
    eng.close()
    live = np.arange(ids.shape[1] - 1)[None, :] < (lens[:, None] - 1)
    assert np.array_equal(out["scored"].numpy(), lens - 1)
    err = np.abs(out["token_logprobs"].double().numpy() - g["token_logprobs"])[live].max()
    print(f"score blip2-tiny {dtype} against HF golden: max |d token log-prob| {err:.3e}")
    assert err <= 2e-3
    sure = live & (g["margin"] > 2e-3)
    assert sure.sum() >= 0.9 * live.sum() and np.array_equal(out["top_ids"].numpy()[sure], g["top_ids"][sure])
    own = meta["own_caption_row"]
    n = int(lens[own]) - 1
    assert np.array_equal(out["top_ids"][own, :n].numpy(), ids[own, 1:n + 1])
    assert torch.equal(out["token_logprobs"][own, :n], out["top_logprobs"][own, :n])
    for k in KEYS[:3]:
        assert float(np.abs(out[k].numpy()[~live]).max()) == 0.0
