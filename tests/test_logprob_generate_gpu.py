"""GPU: per-step log-probs of the greedy loop (`engine.generate(output_logprobs=True)`, cap_generate_scored) and the batched
per-caption perplexity built on them, on procedural tiny checkpoints: against float64 on the returned logits, bit-equal across the
small-batch path, the batch kernels with and without row compaction and a merged pool pass, and against the one-crop product path
(`forward` + `compute_perplexity()`) for BLIP, CoCa and BLIP-2.

The bar of a step value is the selection kernel's (tests/test_logprob_kernel_gpu.py): the larger of 8 x the error of torch float32
on the CPU against float64 on the same logits rows, and 4 fp32 spacings at the value's magnitude."""
import dataclasses
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

L = 12


def _pil(seed, size=(48, 40)):
    from PIL import Image
    rng = np.random.default_rng(seed)
    return Image.fromarray(rng.integers(0, 256, size=(size[1], size[0], 3), dtype=np.uint8), "RGB")


def _step_bar(rows32):
    """rows32 fp32 [n, V] (host) -> (float64 log max softmax [n], bar [n])."""
    x = rows32.double().numpy()
    m = x.max(axis=1, keepdims=True)
    want = -np.log(np.exp(x - m).sum(axis=1))
    ref32 = torch.log_softmax(rows32, dim=-1).max(dim=-1).values.double().numpy()
    ref_err = float(np.abs(ref32 - want).max())
    return want, np.maximum(8.0 * ref_err, 4.0 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64))


@pytest.fixture(scope="module")
def blip_tiny():
    from embodied_captioning_amd.config import BlipArch
    from embodied_captioning_amd.weights import procedural_blip_state_dict, synthetic_pixels
    arch = BlipArch.tiny()
    # seed 5 at eos_boost 2: the fp32 restatement ends these captions after 4, 7, 8 and 12 tokens (the first 8 rows: 4, 8, 12)
    return arch, procedural_blip_state_dict(arch, 5, eos_boost=2.0), synthetic_pixels(24, arch.image_size, seed=7)


@pytest.mark.parametrize("dtype", ["f32s", "bf16"])
def test_blip_token_logprobs_match_float64_of_the_returned_logits(blip_tiny, dtype):
    from embodied_captioning_amd.engine import CaptionerEngine
    arch, sd, px = blip_tiny
    eng = CaptionerEngine(arch, dtype=dtype, max_batch=8, max_beams=1, max_len=L)
    eng.load_state_dict(sd)
    pxd = px[:8].cuda()
    out = eng.generate(pxd, max_length=L, output_logprobs=True, output_logits=True)
    plain = eng.generate(pxd, max_length=L)
    assert torch.equal(out["sequences"], plain["sequences"]) and torch.equal(out["lengths"], plain["lengths"])
    assert set(plain) == {"sequences", "lengths"}
    lp, sc, lens, logits = out["token_logprobs"].cpu(), out["scored_steps"].cpu(), out["lengths"].cpu(), out["logits"].cpu()
    assert lp.shape == (8, L - 1) and lp.dtype == torch.float32 and sc.dtype == torch.int32
    assert torch.equal(sc, lens - 1)
    assert len(set(lens.tolist())) > 1                         # rows end at different steps
    worst = 0.0
    for r in range(8):
        n = int(sc[r])
        assert n >= 1 and float(lp[r, n:].abs().max() if n < L - 1 else 0.0) == 0.0
        want, bar = _step_bar(logits[:n, r])
        err = np.abs(lp[r, :n].double().numpy() - want)
        worst = max(worst, float((err / bar).max()))
        assert (err <= bar).all(), (dtype, r, lp[r, :n], want, bar)
        assert bool((lp[r, :n] < 0).all())
    print(f"token_logprob generate blip-tiny {dtype}: kernel_err_over_bar_max={worst:.3f}")
    eng.close()


def test_same_bits_alone_batched_uncompacted_merged_and_with_early_exit(blip_tiny):
    from embodied_captioning_amd.engine import CaptionerEngine, EnginePool
    arch, sd, px = blip_tiny
    eng = CaptionerEngine(arch, dtype="f32s", max_batch=24, max_beams=1, max_len=L)
    eng.load_state_dict(sd)
    pxd = px.cuda()
    kw = dict(max_length=L, output_logprobs=True)
    full = eng.generate(pxd, **kw)
    assert eng.last_row_compaction and eng.last_decode_path == "batch"          # asking for log-probs keeps the compacted loop
    lp, sc = full["token_logprobs"].clone(), full["scored_steps"].clone()
    assert torch.equal(sc, full["lengths"] - 1) and len(set(sc.tolist())) > 1
    plain = eng.generate(pxd, max_length=L)
    assert eng.last_row_compaction
    assert torch.equal(plain["sequences"], full["sequences"]) and torch.equal(plain["lengths"], full["lengths"])
    # every frame alone: the small-batch kernels
    for r in range(24):
        one = eng.generate(pxd[r:r + 1], **kw)
        assert eng.last_decode_path == "small" and not eng.last_row_compaction
        assert torch.equal(one["token_logprobs"], lp[r:r + 1]) and torch.equal(one["scored_steps"], sc[r:r + 1]), r
    # the batch kernels without compaction
    eng.set_row_compaction(False)
    off = eng.generate(pxd, **kw)
    assert not eng.last_row_compaction
    assert torch.equal(off["token_logprobs"], lp) and torch.equal(off["scored_steps"], sc)
    eng.set_row_compaction(True)
    # early exit: the steps that never run leave the zeros
    eng.set_early_exit(1)
    early = eng.generate(pxd, **kw)
    assert int(sc.max()) <= eng.last_decode_steps <= L - 1
    assert torch.equal(early["token_logprobs"], lp) and torch.equal(early["scored_steps"], sc)
    eng.set_early_exit(0)
    # three batches of 8 merged into one 24-row pass by the pool, split back per batch
    pool = EnginePool(arch, n=1, dtype="f32s", max_batch=24, max_beams=1, max_len=L, weights_of=eng)
    outs = pool.generate_many([pxd[0:8], pxd[8:16], pxd[16:24]], coalesce_rows=24, **kw)
    assert pool.last_coalesce == [[0, 1, 2]], pool.last_coalesce
    assert pool.engines[0].last_row_compaction
    for j, o in enumerate(outs):
        assert torch.equal(o["token_logprobs"], lp[8 * j:8 * j + 8]) and torch.equal(o["scored_steps"], sc[8 * j:8 * j + 8])
        assert torch.equal(o["sequences"], full["sequences"][8 * j:8 * j + 8])
    pool.close()
    eng.close()


def test_beams_with_logprobs_are_refused_by_name(blip_tiny):
    from embodied_captioning_amd._native import CaptionerHipError
    from embodied_captioning_amd.engine import CaptionerEngine
    arch, sd, px = blip_tiny
    eng = CaptionerEngine(arch, dtype="f32s", max_batch=4, max_beams=3, max_len=L)
    eng.load_state_dict(sd)
    with pytest.raises(CaptionerHipError, match="num_beams"):
        eng.generate(px[:4].cuda(), num_beams=3, max_length=L, output_logprobs=True)
    out = eng.generate(px[:4].cuda(), num_beams=3, max_length=L)          # the handle still works
    assert "sequences_scores" in out and "token_logprobs" not in out
    eng.close()


def _model(**kw):
    from embodied_captioning_amd.captioner.utils.utils import Configuration
    from embodied_captioning_amd.captioner.utils.utils_captioner import select_captioner
    return select_captioner(Configuration(height=224, width=224, dtype="f32s", batch_size=4, **kw).captioner).eval()


def _check_against_one_crop(model, crops, steps_of_len, tag):
    """generate_batch(output_perplexity=True) against forward + compute_perplexity per crop: |d ln ppl| <= max over the steps of the
    kernel bar + the measured error of compute_perplexity's own fp32 softmax on the same logits."""
    out = model.generate_batch(crops, output_perplexity=True)
    base = model.generate_batch(crops)
    assert out["texts"] == base["texts"] and torch.equal(out["sequences"], base["sequences"])
    assert "perplexities" not in base and "token_logprobs" not in base
    ppl = out["perplexities"]
    assert ppl.dtype == torch.float64 and ppl.shape == (len(crops),) and bool(torch.isfinite(ppl).all())
    worst = 0.0
    for i, crop in enumerate(crops):
        one = model(crop)
        assert one["text"] == out["texts"][i]
        want32 = float(model.compute_perplexity())
        rows = torch.cat([l.float().cpu() for l in one["logits"]])                    # [T, V]
        n = int(out["scored_steps"][i])
        assert n == rows.shape[0] == steps_of_len(int(out["lengths"][i])), (tag, i, n, rows.shape)
        lp64, bar = _step_bar(rows)
        own = abs(np.log(want32) + lp64.sum() / n)                                    # compute_perplexity's fp32 arithmetic
        diff = abs(np.log(float(ppl[i])) - np.log(want32))
        worst = max(worst, diff / (bar.max() + own))
        assert diff <= bar.max() + own, (tag, i, float(ppl[i]), want32, bar.max(), own)
        err = np.abs(out["token_logprobs"][i, :n].double().numpy() - lp64)
        assert (err <= bar).all(), (tag, i, err, bar)
    print(f"token_logprob perplexity {tag}: d_ln_ppl_over_bar_max={worst:.3f}")
    return out


def test_batched_perplexity_equals_the_one_crop_path_blip():
    model = _model(arch_name="blip", model_name="procedural-tiny:4:2.0", max_length=L)
    _check_against_one_crop(model, [_pil(i) for i in range(30, 34)], lambda n: n - 1, "blip-tiny")


def test_batched_perplexity_equals_the_one_crop_path_blip2():
    model = _model(arch_name="blip2", model_name="procedural-blip2-tiny:11:0.5", max_new_tokens=8)
    _check_against_one_crop(model, [_pil(i) for i in range(40, 44)], lambda n: n, "blip2-tiny")


def test_batched_perplexity_equals_the_one_crop_path_coca_with_eos_mask_and_forced_eos():
    model = _model(arch_name="coca", model_name="procedural-coca-tiny:1:4.0")
    crops = [_pil(i) for i in range(50, 54)]
    a = model.arch
    assert a.min_seq_len >= 3                                   # steps 0 and 1 run with EOS masked
    lens = model.generate_batch(crops)["lengths"]
    if int(lens.max()) < a.seq_len:                             # cut the longest caption short: its last step is the forced EOS
        model.arch = dataclasses.replace(a, seq_len=max(int(lens.max()) - 1, a.min_seq_len + 1))
    assert model.arch.seq_len > a.min_seq_len
    out = _check_against_one_crop(model, crops, lambda n: n - 1, "coca-tiny")
    seq, ln = out["sequences"], out["lengths"]
    assert int(ln.max()) == model.arch.seq_len                  # a row reached the forced-EOS last step
    r = int(ln.argmax())
    assert int(seq[r, model.arch.seq_len - 1]) == a.eos and int(out["scored_steps"][r]) == model.arch.seq_len - 1
    # no caption of this fixture ends on a sampled pad id (the one-crop path records one step fewer for such a row)
    assert all(int(seq[i, int(ln[i]) - 1]) == a.eos for i in range(len(crops)))


def test_box_captioner_with_perplexity(tmp_path):
    from embodied_captioning_amd.pseudolabeler import BatchedBoxCaptioner, save_record
    from embodied_captioning_amd.utils.predictor_utils import Captioner
    cap_cfg = types.SimpleNamespace(arch_name="blip", model_name="procedural-tiny:4:2.0", checkpoint_name=None,
                                    height=224, width=224, dtype="f32s", max_length=L, batch_size=4)
    cap = Captioner(types.SimpleNamespace(captioner=cap_cfg)).eval()
    rng = np.random.default_rng(0)
    frame = rng.integers(0, 256, size=(120, 160, 3), dtype=np.uint8)
    boxes = [(10, 20, 60, 90), (100, 5, 158, 60), (70, 30, 130, 110)]
    plain = BatchedBoxCaptioner(cap).predict_caption(boxes, frame)
    got = BatchedBoxCaptioner(cap, with_perplexity=True).predict_caption(boxes, frame)
    assert "perplexities" not in plain and got["captions"] == plain["captions"] and len(got["captions"]) == 3
    p = got["perplexities"]
    assert p.dtype == torch.float64 and p.shape == (3,) and bool(torch.isfinite(p).all()) and bool((p >= 1.0).all())
    texts, ppl = cap.caption_batch([_pil(1), _pil(2)], return_perplexity=True)
    assert texts == cap.caption_batch([_pil(1), _pil(2)]) and ppl.shape == (2,)
    path = save_record(str(tmp_path), "episode_0_step_0", got, frame)
    rec = np.load(path, allow_pickle=True)["arr_0"].item()
    assert set(rec) == {"instances", "image"} and set(rec["instances"]) == {"captions", "embeddings", "perplexities"}
    assert torch.equal(rec["instances"]["perplexities"], p) and rec["instances"]["captions"] == got["captions"]
    old = np.load(save_record(str(tmp_path), "episode_0_step_1", plain, frame), allow_pickle=True)["arr_0"].item()
    assert set(old["instances"]) == {"captions", "embeddings"}
