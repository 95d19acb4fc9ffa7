"""GPU: teacher-forced scoring of given captions (`CaptionerEngine.score`, cap_score_captions) on the BLIP tiny fixture.

1. against tests/golden/blip_tiny_score.npz (HF `BlipForConditionalGeneration(pixel_values, input_ids=...)`, tools/
   make_goldens_score.py) and the float64 restatement (tests/_score_ref.py): in "f32" and "f32s" every live token log-prob within
   2e-3 - the project holds logits to 1e-3, and a log-softmax moves by at most the target's error plus the largest error in the
   row -, top_ids equal wherever the reference's top-2 margin exceeds 2e-3, scored == lens - 1, exact zeros behind a caption's end;
2. "bf16": no absolute bar - top_ids agree with the fp32 restatement wherever its margin exceeds 0.05 (the margin token_parity is
   given in tests/test_blip2_gpu.py); the measured maximum is printed (profiles/score_captions_tolerances.txt);
3. own-caption consistency: `generate(output_logprobs=True)`, then `score` of the returned sequences;
4. invariance in bits: a pair alone, in a batch, as a slot of a 3-candidate request, every chunking of the arena, length sort on / off;
5. padding and absent slots never leak;  6. refusals before anything is launched;  7. generate / score / generate;
8. the wrapper surface;  9. BLIP-base geometry (KV16 cross cache): HF's greedy captions scored as given captions."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from _score_ref import blip_score, random_captions

pytestmark = pytest.mark.gpu

KEYS = ("token_logprobs", "top_logprobs", "top_ids", "scored")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "blip_tiny_score.npz")


@pytest.fixture(scope="module")
def fx():
    """The golden's arch, weights, frames, captions - and the float32 / float64 restatements, computed once."""
    from embodied_captioning_amd.config import BlipArch
    from embodied_captioning_amd.weights import procedural_blip_state_dict, synthetic_pixels
    g = np.load(GOLDEN)
    meta = json.loads(str(g["meta"]))
    arch = BlipArch(**meta["arch"])
    sd = procedural_blip_state_dict(arch, meta["seed"], eos_boost=meta["eos_boost"])
    px = synthetic_pixels(meta["batch"], arch.image_size, seed=meta["seed"])
    ids, lens, Cn = g["ids"], g["lens"], meta["captions_per_image"]
    return dict(g=g, meta=meta, arch=arch, sd=sd, px=px, ids=ids, lens=lens, C=Cn, L=int(ids.shape[1]),
                ref64=blip_score(sd, arch, px, ids, lens, Cn, torch.float64), ref32=blip_score(sd, arch, px, ids, lens, Cn, torch.float32))


def _engine(fx, dtype, batch=4, beams=3, max_len=None, **kw):
    from embodied_captioning_amd.engine import CaptionerEngine
    eng = CaptionerEngine(fx["arch"], dtype=dtype, max_batch=batch, max_beams=beams, max_len=max_len or fx["L"], **kw)
    eng.load_state_dict(fx["sd"])
    return eng


def _cpu(out):
    return {k: out[k].cpu() for k in KEYS}


def _same(a, b, rows_a=slice(None), rows_b=slice(None)):
    return all(torch.equal(a[k][rows_a], b[k][rows_b]) for k in KEYS)


# ------------------------------------------------------------------------------------------------ 1. goldens and float64
@pytest.mark.parametrize("dtype", ["f32", "f32s"])
def test_token_logprobs_against_hf_golden_and_float64(fx, dtype):
    eng = _engine(fx, dtype)
    out = _cpu(eng.score(fx["px"].cuda(), fx["ids"], fx["lens"], captions_per_image=fx["C"]))
    eng.close()
    live = fx["ref64"]["live"]
    lens = fx["lens"]
    assert out["token_logprobs"].shape == (12, fx["L"] - 1) and out["top_ids"].dtype == torch.int32
    assert np.array_equal(out["scored"].numpy(), lens - 1)
    for k in KEYS[:3]:
        assert float(np.abs(out[k].numpy()[~live]).max()) == 0.0, k                # exact zeros behind every caption's end
    tlp, top = out["token_logprobs"].double().numpy(), out["top_logprobs"].double().numpy()
    for name, want_tlp, want_ids, margin in (("HF golden", fx["g"]["token_logprobs"], fx["g"]["top_ids"], fx["g"]["margin"]),
                                             ("float64 restatement", fx["ref64"]["token_logprobs"], fx["ref64"]["top_ids"],
                                              fx["ref64"]["margin"])):
        err = np.abs(tlp - want_tlp)[live].max()
        print(f"score blip-tiny {dtype} against {name}: max |d token log-prob| {err:.3e}")
        assert err <= 2e-3, (dtype, name, err)
        sure = live & (margin > 2e-3)
        assert sure.sum() >= 0.9 * live.sum()
        assert np.array_equal(out["top_ids"].numpy()[sure], want_ids[sure])
    err_top = np.abs(top - fx["ref64"]["top_logprobs"])[live].max()
    print(f"score blip-tiny {dtype}: max |d top log-prob| against float64 {err_top:.3e}")
    assert err_top <= 2e-3
    assert bool((out["token_logprobs"] <= out["top_logprobs"]).all())
    own = fx["meta"]["own_caption_row"]                                              # HF's own greedy caption is its own arg-max path
    n = int(lens[own]) - 1
    assert np.array_equal(out["top_ids"][own, :n].numpy(), fx["ids"][own, 1:n + 1])
    assert torch.equal(out["token_logprobs"][own, :n], out["top_logprobs"][own, :n])


# ------------------------------------------------------------------------------------------------ 2. bf16
def test_bf16_top_ids_at_clear_margins_and_measured_error(fx):
    eng = _engine(fx, "bf16")
    out = _cpu(eng.score(fx["px"].cuda(), fx["ids"], fx["lens"], captions_per_image=fx["C"]))
    eng.close()
    live, margin = fx["ref32"]["live"], fx["ref32"]["margin"]
    assert np.array_equal(out["scored"].numpy(), fx["lens"] - 1)
    sure = live & (margin > 0.05)
    assert sure.sum() >= 0.85 * live.sum()                                           # known from the CPU restatement alone: 61 of 70
    assert np.array_equal(out["top_ids"].numpy()[sure], fx["ref32"]["top_ids"][sure])
    err = np.abs(out["token_logprobs"].double().numpy() - fx["ref64"]["token_logprobs"])[live]
    print(f"score blip-tiny bf16: max |d token log-prob| against float64 {err.max():.3e} (mean {err.mean():.3e}), "
          f"{int(sure.sum())} of {int(live.sum())} positions above the 0.05 margin")
    for k in KEYS[:3]:
        assert float(np.abs(out[k].numpy()[~live]).max()) == 0.0


# ------------------------------------------------------------------------------------------------ 3. own captions
def _own_caption_fixture():
    """Seed of the procedural checkpoint chosen ON THE CPU: the first whose greedy captions (fp32 restatement) leave out at most 1
    position in 10 at a 4e-3 top-2 margin and do not all have the same length."""
    from oracle import blip_ref as R
    from embodied_captioning_amd.config import BlipArch
    from embodied_captioning_amd.weights import procedural_blip_state_dict, synthetic_pixels
    arch = BlipArch.tiny()
    px = synthetic_pixels(8, arch.image_size, seed=7)
    for seed in range(3, 12):
        sd = procedural_blip_state_dict(arch, seed, eos_boost=2.0)
        seq = R.greedy_generate(sd, arch, px, 12)["sequences"].numpy()
        lens = np.array([r.tolist().index(arch.eos) + 1 if arch.eos in r.tolist() else len(r) for r in seq])
        ids = np.full((8, 12), arch.pad, dtype=np.int32)
        ids[:, : seq.shape[1]] = seq
        ref = blip_score(sd, arch, px, ids, lens, 1, torch.float32)
        sure = ref["live"] & (ref["margin"] > 4e-3)
        if sure.sum() >= 0.9 * ref["live"].sum() and len(set(lens.tolist())) > 1:
            return arch, sd, px, ids, lens, ref, sure
    raise AssertionError("no seed keeps the margins")


def test_scoring_a_generated_caption_reproduces_the_greedy_call():
    from embodied_captioning_amd.engine import CaptionerEngine
    arch, sd, px, ids, lens, ref, sure = _own_caption_fixture()
    assert sure.sum() >= 0.9 * ref["live"].sum()                                     # the cap on what the margins leave out
    eng = CaptionerEngine(arch, dtype="f32s", max_batch=8, max_beams=1, max_len=12, max_score_rows=8 * 11)
    eng.load_state_dict(sd)
    gen = eng.generate(px.cuda(), max_length=12, output_logprobs=True)
    seq, glen, glp = gen["sequences"].cpu(), gen["lengths"].cpu(), gen["token_logprobs"].cpu()
    out = _cpu(eng.score(px.cuda(), seq, glen))
    eng.close()
    assert torch.equal(out["scored"], gen["scored_steps"].cpu())
    same_path = np.array([np.array_equal(seq[r, : int(glen[r])].numpy(), ids[r, : int(lens[r])]) and int(glen[r]) == int(lens[r])
                          for r in range(8)])
    assert same_path.sum() >= 6                                                      # the margins say the tokens are the restatement's
    n = 0
    for r in np.nonzero(same_path)[0]:
        for j in np.nonzero(sure[r])[0]:
            assert int(out["top_ids"][r, j]) == int(seq[r, j + 1]), (r, j)
            assert float(out["token_logprobs"][r, j]) == float(out["top_logprobs"][r, j]), (r, j)
            assert abs(float(out["token_logprobs"][r, j]) - float(glp[r, j])) <= 4e-3, (r, j)
            assert abs(float(out["token_logprobs"][r, j]) - ref["token_logprobs"][r, j]) <= 2e-3 + 1e-4, (r, j)
            n += 1
    d = (out["token_logprobs"] - glp).abs()[torch.from_numpy(ref["live"] & same_path[:, None])].max()
    print(f"own captions f32s: {n} positions compared, max |score - generate| over all live positions {float(d):.3e}")
    assert n >= 20


# ------------------------------------------------------------------------------------------------ 4. invariance in bits
@pytest.mark.parametrize("dtype", ["f32s", "bf16"])
def test_same_bits_alone_batched_as_a_slot_and_under_every_chunking(fx, dtype):
    px, ids, lens, Cn, L = fx["px"].cuda(), fx["ids"], fx["lens"], fx["C"], fx["L"]
    one_pass = _engine(fx, dtype, max_score_rows=12 * (L - 1))
    base = _cpu(one_pass.score(px, ids, lens, captions_per_image=Cn))
    assert one_pass.last_score_passes == 1
    # chunkings of the same request: 1 caption per pass; 2 of an image's 3 captions, then 1; whole images with the head in slices of 4 rows
    for kw, passes in ((dict(batch=4, beams=3), 12), (dict(batch=4, beams=8), 8), (dict(batch=4, beams=1, max_prompt=L), 4)):
        eng = _engine(fx, dtype, **kw)
        got = _cpu(eng.score(px, ids, lens, captions_per_image=Cn))
        assert eng.last_score_passes == passes, (kw, eng.last_score_passes)
        assert _same(base, got), (dtype, kw)
        eng.close()
    # every caption as a pair of its own image: alone, and inside a batch of pairs (one call of 4 images, three calls)
    pair_px = px.repeat_interleave(Cn, dim=0)
    for n in (2, 7, 11):
        alone = _cpu(one_pass.score(pair_px[n:n + 1], ids[n:n + 1], lens[n:n + 1]))
        assert _same(base, alone, slice(n, n + 1)), (dtype, n)
    for sort in (True, False):
        pairs = _cpu(one_pass.score(pair_px, ids, lens, sort_by_length=sort))       # 12 images on a 4-image engine: 3 calls
        assert _same(base, pairs), (dtype, sort)
    # a pair as slot c of a 3-candidate request whose other slots are absent or other captions
    for c in range(3):
        slot_ids = random_captions(fx["arch"], 3, L, None, seed=40 + c)
        slot_lens = np.array([0, 0, L], dtype=np.int32)[[(k - c) % 3 for k in range(3)]]     # slot c + 1 absent, c + 2 full
        slot_ids[c], slot_lens[c] = ids[5], lens[5]                                    # caption 5: image 1, 7 tokens
        got = _cpu(one_pass.score(px[1:2], slot_ids, slot_lens, captions_per_image=3))
        assert _same(base, got, slice(5, 6), slice(c, c + 1)), (dtype, c)
    one_pass.close()


# ------------------------------------------------------------------------------------------------ 5. padding never leaks
def test_ids_behind_a_captions_end_and_absent_slots_change_nothing(fx):
    px, L, Cn = fx["px"].cuda(), fx["L"], fx["C"]
    ids, lens = fx["ids"].copy(), fx["lens"].copy()
    lens[[4, 9]] = 0                                                                 # two absent slots
    eng = _engine(fx, "f32s")
    a = _cpu(eng.score(px, ids, lens, captions_per_image=Cn))
    other = random_captions(fx["arch"], 12, L, None, seed=99)
    ids2 = ids.copy()
    for n in range(12):
        ids2[n, lens[n]:] = other[n, lens[n]:]                                        # lens 0: the whole row
    ids2[4, 0] = 3                                                                    # an absent slot's column 0 is not looked at either
    b = _cpu(eng.score(px, ids2, lens, captions_per_image=Cn))
    eng.close()
    assert not np.array_equal(ids, ids2)
    assert _same(a, b)
    assert int(a["scored"][4]) == 0 and float(a["token_logprobs"][4].abs().max()) == 0.0 and int(a["top_ids"][9].abs().max()) == 0
    keep = [n for n in range(12) if n not in (4, 9)]
    assert np.abs(a["token_logprobs"].double().numpy()[keep] - fx["ref64"]["token_logprobs"][keep])[fx["ref64"]["live"][keep]].max() <= 2e-3


# ------------------------------------------------------------------------------------------------ 6. refusals
def _abi_score(eng, px, ids, lens, Cn, L):
    n = ids.shape[0]
    ids_d, lens_d = torch.as_tensor(ids, dtype=torch.int32).cuda(), torch.as_tensor(lens, dtype=torch.int32).cuda()
    f = torch.full((n, max(L - 1, 1)), -7.0, device="cuda")
    i = torch.full((n, max(L - 1, 1)), -7, dtype=torch.int32, device="cuda")
    sc = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
    rc = eng.lib.cap_score_captions(eng._h, p(px), 0, int(px.shape[0]), p(ids_d), p(lens_d), Cn, L, p(f), p(f.clone()), p(i), p(sc),
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert float(f.max()) == -7.0 and int(sc.max()) == -7                              # a refused call writes nothing
    return rc


def test_refusals_name_the_fault_before_anything_is_launched(fx):
    from embodied_captioning_amd import _native
    from embodied_captioning_amd.config import CocaArch
    from embodied_captioning_amd.engine import CaptionerEngine
    px, ids, lens, L = fx["px"].cuda(), fx["ids"], fx["lens"], fx["L"]
    eng = _engine(fx, "f32s", batch=4, beams=1, max_len=L)
    pair_ids, pair_lens = ids[2::3], lens[2::3]                                        # the 4 full-length captions
    with pytest.raises(ValueError, match="outside"):
        eng.score(px, pair_ids, np.array([L, L + 1, L, L]))
    with pytest.raises(ValueError, match="outside"):
        eng.score(px, pair_ids, np.array([L, 1, L, L]))
    with pytest.raises(ValueError, match="absent slot"):
        eng.score(px, pair_ids, np.array([L, 0, L, L]))
    bad = pair_ids.copy()
    bad[1, 0] = 7
    with pytest.raises(ValueError, match="BOS"):
        eng.score(px, bad, pair_lens)
    bad = pair_ids.copy()
    bad[3, 4] = fx["arch"].vocab
    with pytest.raises(ValueError, match="out of range"):
        eng.score(px, bad, pair_lens)
    long_ids = random_captions(fx["arch"], 4, L + 1, None, seed=1)
    with pytest.raises(ValueError, match="too long"):
        eng.score(px, long_ids, np.full(4, L + 1))
    with pytest.raises(ValueError, match="max_score_rows >= %d" % (L - 1)):           # 4 workspace rows, 11 needed
        eng.score(px, pair_ids, pair_lens)
    assert _abi_score(eng, px, long_ids, np.full(4, L + 1), 1, L + 1) != 0 and "capacity" in _native.last_error()
    assert _abi_score(eng, px, pair_ids, pair_lens, 1, L) != 0 and "max_score_rows >= %d" % (L - 1) in _native.last_error()
    assert _abi_score(eng, px, pair_ids, pair_lens, 0, L) != 0 and "captions_per_image" in _native.last_error()
    assert _abi_score(eng, px, pair_ids[:, :1], pair_lens, 1, 1) != 0
    eng.close()
    carch = CocaArch.tiny()
    coca = CaptionerEngine(carch, dtype="f32s", max_batch=2, max_beams=1, max_len=8)    # no weights needed: refused by the handle's kind
    cpx = torch.zeros((2, 3, carch.image_size, carch.image_size), device="cuda")
    cids = np.full((2, 4), 5, dtype=np.int32)
    assert _abi_score(coca, cpx, cids, np.full(2, 4), 1, 4) != 0 and "CoCa" in _native.last_error()
    with pytest.raises(ValueError, match="CoCa"):
        coca.score(cpx, cids, np.full(2, 4))
    coca.close()


# ------------------------------------------------------------------------------------------------ 7. state
def test_generate_score_generate_on_one_handle(fx):
    px, L = fx["px"].cuda(), fx["L"]
    eng = _engine(fx, "f32s", batch=4, beams=3)
    a = eng.generate(px, max_length=L, output_logprobs=True)
    a = {k: v.clone() for k, v in a.items()}
    eng.score(px, fx["ids"], fx["lens"], captions_per_image=fx["C"])
    b = eng.generate(px, max_length=L, output_logprobs=True)
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
    beams = eng.generate(px, num_beams=3, max_length=L)
    eng.score(px, fx["ids"], fx["lens"], captions_per_image=fx["C"])
    again = eng.generate(px, num_beams=3, max_length=L)
    assert all(torch.equal(beams[k], again[k]) for k in beams)
    eng.close()


# ------------------------------------------------------------------------------------------------ 8. surface
def _pil(seed, size=(48, 40)):
    from PIL import Image
    rng = np.random.default_rng(seed)
    return Image.fromarray(rng.integers(0, 256, size=(size[1], size[0], 3), dtype=np.uint8), "RGB")


def test_wrapper_plugin_scorer_and_pseudo_caption_surface():
    import types
    from embodied_captioning_amd.captioner.likelihood_scorer import CaptionLikelihoodScorer
    from embodied_captioning_amd.pseudocaptioner import likelihood_pseudo_captions
    from embodied_captioning_amd.utils.predictor_utils import Captioner
    cap_cfg = types.SimpleNamespace(arch_name="blip", model_name="procedural-tiny:4:2.0", checkpoint_name=None, height=224, width=224,
                                    batch_size=2, num_beams=3, max_length=12, max_score_rows=44)
    cap = Captioner(types.SimpleNamespace(captioner=cap_cfg)).eval()
    model, arch = cap.model, cap.model.arch
    crops = [_pil(1), _pil(2), _pil(3)]                                                  # 3 images on a 2-image engine: two calls
    pairs = [[arch.bos, 31, 47, 59, arch.eos], [31, 47], [arch.bos, 7, 8, 9, 10, 11, 12, 13]]      # BOS is put in front where missing
    out = model.score_captions(crops, pairs)
    assert out["captions_per_image"] == 1 and out["n_tokens"].tolist() == [4, 2, 7] and tuple(out["token_logprobs"].shape) == (3, 7)
    ids = np.full((3, 8), arch.pad, dtype=np.int32)
    rows = [pairs[0], [arch.bos] + pairs[1], pairs[2]]
    for r, p in enumerate(rows):
        ids[r, : len(p)] = p
    direct = model.engine.score(model.preprocess(crops).to(model.device), ids, [len(p) for p in rows])
    assert torch.equal(out["token_logprobs"], direct["token_logprobs"].cpu()) and torch.equal(out["top_ids"], direct["top_ids"].cpu())
    again = cap.score_batch(crops, pairs)
    assert all(torch.equal(out[k], again[k]) for k in ("token_logprobs", "logprob_mean", "perplexity", "top_perplexity"))
    # the summary numbers are float64 arithmetic on the returned log-probs (the step bar of the device values is tested above)
    for r in range(3):
        n = int(out["n_tokens"][r])
        lp = out["token_logprobs"][r, :n].double()
        assert float(out["token_logprobs"][r, n:].abs().sum()) == 0.0
        assert abs(float(out["logprob_sum"][r]) - float(lp.sum())) <= 1e-12 and abs(float(out["logprob_mean"][r]) - float(lp.mean())) <= 1e-12
        assert abs(float(out["perplexity"][r]) - float(torch.exp(-lp.mean()))) <= 1e-9
        top = out["top_logprobs"][r, :n].double()
        assert abs(float(out["top_perplexity"][r]) - float(torch.exp(-top.mean()))) <= 1e-9
        assert float(out["top_perplexity"][r]) <= float(out["perplexity"][r]) + 1e-12
    # candidates per image (ragged): caption-major rows with absent slots; a candidate's numbers are the pair's, bit for bit
    cands = model.score_captions(crops, [[pairs[0], pairs[2]], [pairs[1]], [pairs[2], pairs[0]]])
    assert cands["captions_per_image"] == 2 and cands["n_tokens"].tolist() == [4, 7, 2, 0, 7, 4]
    assert torch.equal(cands["token_logprobs"][0], out["token_logprobs"][0]) and torch.equal(cands["token_logprobs"][2], out["token_logprobs"][1])
    assert torch.equal(cands["token_logprobs"][4], out["token_logprobs"][2]) and bool(torch.isnan(cands["perplexity"][3]))
    with pytest.raises(ValueError, match="tokenizer"):
        model.score_captions(crops[:1], ["a chair"])
    # the scorer surface and the pseudo-caption selection on it
    scorer = CaptionLikelihoodScorer(model=model)
    assert scorer.arch is arch and scorer.device == model.device
    sp = scorer.score_pairs(crops, pairs)
    assert torch.equal(sp, out["logprob_mean"])
    sm = scorer.score_matrix(crops, [pairs[0], pairs[2], pairs[0]])                       # a duplicate caption: scored once, copied
    assert tuple(sm.shape) == (3, 3) and torch.equal(sm[:, 0], sm[:, 2])
    assert float(sm[0, 0]) == float(out["logprob_mean"][0]) and float(sm[2, 1]) == float(out["logprob_mean"][2])
    frame = np.random.default_rng(5).integers(0, 256, size=(96, 128, 3), dtype=np.uint8)
    mk = lambda box, c: {"image": frame, "pred_box": np.array(box, np.float32), "caption": c}      # noqa: E731
    grouped = {(0, 1): [mk([8, 8, 60, 60], "31 47 59"), mk([20, 10, 90, 70], "7 8 9"), mk([30, 30, 80, 90], "31 47 59")],
               (0, 2): [mk([5, 5, 50, 50], "12 13")]}

    class IdScorer(CaptionLikelihoodScorer):                                             # the procedural model has no tokenizer
        def score_matrix(self, images, captions):
            return super().score_matrix(images, [[int(t) for t in c.split()] for c in captions])

    res = likelihood_pseudo_captions(grouped, IdScorer(model=model))
    assert set(res) == {"(0, 1)", "(0, 2)"}
    lst = res["(0, 1)"]["captions_list"]
    assert sorted(c for _, c in lst) == ["31 47 59", "7 8 9"] and lst[0][0] >= lst[1][0] and res["(0, 1)"]["pseudocaption"] == lst[0]
    assert all(isinstance(s, float) and s < 0 for s, _ in lst) and res["(0, 2)"]["pseudocaption"][1] == "12 13"
    model.engine.close()


# ------------------------------------------------------------------------------------------------ 9. BLIP-base geometry (KV16 cross cache)
def test_base_geometry_scores_hf_greedy_captions_as_their_own_argmax_path():
    """tests/golden/blip_base256.npz holds HF's greedy captions of the procedural BLIP-base and the top-2 logit margin of every step:
    scored as GIVEN captions, each must be its own arg-max path wherever that margin exceeds 2e-3 - on the split mode's KV16 cross
    cache, which the tiny fixture (17 image tokens) never uses.  One pass with reserved capacity, one caption per pass without (on
    the same weights), and the captions as candidate slots give the same bits."""
    from _util import golden_inputs
    from embodied_captioning_amd.engine import CaptionerEngine
    g, meta, arch, sd, px = golden_inputs("blip_base256")
    n, L = 8, meta["max_length"]
    seq = np.asarray(g["greedy_sequences"])[:n].astype(np.int32)
    margin = np.asarray(g["greedy_margin"])[:, :n].T                                   # [n, L - 1]
    lens = np.array([r.tolist().index(arch.eos) + 1 if arch.eos in r.tolist() else L for r in seq], dtype=np.int32)
    live = np.arange(L - 1)[None, :] < (lens[:, None] - 1)
    pxd = px[:n].cuda()
    eng = CaptionerEngine(arch, dtype="f32s", max_batch=n, max_beams=3, max_len=L, max_score_rows=n * (L - 1))
    eng.load_state_dict(sd)
    assert eng.cross_cache_kind == "kv16"
    out = _cpu(eng.score(pxd, seq, lens))
    assert eng.last_score_passes == 1 and np.array_equal(out["scored"].numpy(), lens - 1)
    sure = live & (margin > 2e-3)
    assert sure.sum() >= 0.9 * live.sum()
    assert np.array_equal(out["top_ids"].numpy()[sure], seq[:, 1:][sure])
    assert torch.equal(out["token_logprobs"][torch.from_numpy(sure)], out["top_logprobs"][torch.from_numpy(sure)])
    assert bool((out["token_logprobs"].numpy()[live] < 0).all()) and float(np.abs(out["token_logprobs"].numpy()[~live]).max()) == 0.0
    small = CaptionerEngine(arch, dtype="f32s", max_batch=n, max_beams=3, max_len=L, share_weights_with=eng)
    chunked = _cpu(small.score(pxd, seq, lens))
    assert small.last_score_passes == n and _same(out, chunked)
    small.close()
    # image b of the first four with its own caption and caption b + 4 as candidates: slot 0 is the pair, bit for bit
    cand_ids = np.stack([seq[:4], seq[4:]], axis=1).reshape(8, L)
    cand_lens = np.stack([lens[:4], lens[4:]], axis=1).reshape(8)
    cands = _cpu(eng.score(pxd[:4], cand_ids, cand_lens, captions_per_image=2))
    assert eng.last_score_passes == 1
    assert _same(out, cands, slice(0, 4), slice(0, 8, 2))
    eng.close()
