"""GPU: `engine.generate(output_vocab_maxprob=True)` (cap_generate_vocab), `engine.fuse_vocab_groups` and
`fused_pseudo_captions` on procedural tiny checkpoints: against float64 on the logits the same call returns, unchanged sequences,
the same bits on the small-batch path, the batch kernels with and without row compaction, a merged pool pass and with early exit,
and the fused pseudo-caption against the host functions fed the same call's logits - BLIP, CoCa (min-length mask, forced EOS) and
BLIP-2.

Bar of a probability: tests/_fusion_ref.py (8 x torch-fp32-CPU softmax's own error on the same rows, or 4 fp32 spacings).  The
threshold condition of the end-to-end checks: no float64 group mean within 4 fp32 spacings of th - asserted on the CPU, from the
same call's logits, before the device result is compared."""
import numpy as np
import pytest
import torch

from _fusion_ref import assert_no_mean_in_band, group_mean64, kept64, prob_bar, softmax64, spacing32, threshold_band

pytestmark = pytest.mark.gpu

L = 12
# th per fixture.  The procedural checkpoints are near-uniform over their 512 tokens (the reference's 0.25 would keep nothing), so
# th sits between well separated group means of the fp32 restatement (oracle/*_ref.py on the CPU, groups GROUPS3, float64 fusion;
# listed per group: its largest mean and the means next to th):
#   blip  (seed 5, boost 2):   top means .0305 .0219 | .0232 .0211 | .0235 .0220 .0219   -> th .0225, nearest mean 5e-4 away
#   coca  (seed 1, boost 4):   top means .0990 .0222 | .0299 .0236 | .7747 .0234         -> th .0250, nearest mean 1.4e-3 away
#   blip2 (seed 11, boost .5): top means .0092       | .0099 .0094 | .0097 .0086         -> th .0095, nearest mean 1e-4 away
# against a band of 4 fp32 spacings of th (7.5e-9 / 7.5e-9 / 3.7e-9); the tests assert the condition again on the call's own logits.
TH = {"blip": 0.0225, "coca": 0.025, "blip2": 0.0095}


@pytest.fixture(scope="module")
def blip_tiny():
    from embodied_captioning_amd.config import BlipArch
    from embodied_captioning_amd.weights import procedural_blip_state_dict, synthetic_pixels
    arch = BlipArch.tiny()
    # the fixture of tests/test_logprob_generate_gpu.py: captions of 4 to 12 tokens
    return arch, procedural_blip_state_dict(arch, 5, eos_boost=2.0), synthetic_pixels(24, arch.image_size, seed=7)


def _want_from_logits(logits, scored, eos=None, min_len=0):
    """logits fp32 [steps, B, V] (host) -> (float64 max_t softmax over each row's first scored steps [B, V], bar [B, V], ref_err);
    min_len: the selection saw EOS at -inf while t + 1 < min_len."""
    B, V = logits.shape[1], logits.shape[2]
    want, bar, ref = np.zeros((B, V)), np.zeros((B, V)), 0.0
    for r in range(B):
        n = int(scored[r])
        rows = logits[:n, r].clone()
        for t in range(n):
            if t + 1 < min_len:
                rows[t, eos] = float("-inf")
        want[r] = softmax64(rows).max(axis=0)
        bar[r], e = prob_bar(rows, want[r])
        ref = max(ref, e)
    return want, bar, ref


def _check_one_call(eng, pxd, tag, steps, eos=None, min_len=0, **kw):
    out = eng.generate(pxd, output_logits=True, output_vocab_maxprob=True, **kw)
    plain = eng.generate(pxd, **kw)
    assert torch.equal(out["sequences"], plain["sequences"]) and torch.equal(out["lengths"], plain["lengths"])
    assert set(plain) == {"sequences", "lengths"}
    assert set(out) == {"sequences", "lengths", "logits", "token_logprobs", "scored_steps", "vocab_maxprob"}
    scored_only = eng.generate(pxd, output_logprobs=True, **kw)
    assert torch.equal(out["token_logprobs"], scored_only["token_logprobs"]) and torch.equal(out["scored_steps"], scored_only["scored_steps"])
    B, V = pxd.shape[0], eng.arch.vocab
    vm = out["vocab_maxprob"]
    assert vm.shape == (B, V) and vm.dtype == torch.float32 and vm.is_cuda and vm.stride(0) % 4 == 0 and vm.stride(0) >= V
    assert out["logits"].shape[0] == steps
    sc = out["scored_steps"].cpu()
    want, bar, ref = _want_from_logits(out["logits"].cpu(), sc, eos, min_len)
    err = np.abs(vm.cpu().double().numpy() - want)
    print(f"vocab_maxprob generate {tag}: ref_err_fp32={ref:.3e} kernel_err_over_bar_max={float((err / bar).max()):.3f} "
          f"scored_steps={sc.tolist()}")
    assert (err <= bar).all(), (tag, float((err / bar).max()))
    return out, want, bar


@pytest.mark.parametrize("dtype", ["f32s", "bf16"])
def test_blip_one_call_with_logits_and_vocab_maxprob(blip_tiny, dtype):
    from embodied_captioning_amd.engine import CaptionerEngine
    arch, sd, px = blip_tiny
    eng = CaptionerEngine(arch, dtype=dtype, max_batch=8, max_beams=1, max_len=L)
    eng.load_state_dict(sd)
    out, _, _ = _check_one_call(eng, px[:8].cuda(), f"blip-tiny {dtype}", L - 1, max_length=L)
    assert torch.equal(out["scored_steps"], out["lengths"] - 1) and len(set(out["lengths"].tolist())) > 1
    eng.close()


def test_coca_one_call_with_min_length_mask_and_forced_eos():
    from embodied_captioning_amd.config import CocaArch
    from embodied_captioning_amd.engine import CaptionerEngine
    from embodied_captioning_amd.weights import procedural_coca_state_dict, synthetic_pixels
    arch = CocaArch.tiny()
    eng = CaptionerEngine(arch, dtype="f32s", max_batch=8, max_beams=1, max_len=arch.seq_len)
    eng.load_state_dict(procedural_coca_state_dict(arch, 1, eos_boost=4.0))
    pxd = synthetic_pixels(8, arch.image_size, seed=3).cuda()
    lens = eng.generate(pxd, max_length=arch.seq_len)["lengths"]
    Lc = arch.seq_len if int(lens.max()) == arch.seq_len else max(int(lens.max()) - 1, arch.min_seq_len + 1)     # a row reaches the forced EOS
    assert arch.min_seq_len >= 3 and Lc > arch.min_seq_len
    out, _, _ = _check_one_call(eng, pxd, "coca-tiny f32s", Lc - 1, eos=arch.eos, min_len=arch.min_seq_len, max_length=Lc)
    assert int(out["lengths"].max()) == Lc
    eng.close()


def test_blip2_one_call():
    from embodied_captioning_amd.config import Blip2Arch
    from embodied_captioning_amd.engine import CaptionerEngine
    from embodied_captioning_amd.weights import procedural_blip2_state_dict, synthetic_pixels
    arch = Blip2Arch.tiny()
    eng = CaptionerEngine(arch, dtype="f32s", max_batch=4, max_beams=1, max_len=8)
    eng.load_state_dict(procedural_blip2_state_dict(arch, 11, eos_boost=0.5))
    out, _, _ = _check_one_call(eng, synthetic_pixels(4, arch.image_size, seed=5).cuda(), "blip2-tiny f32s", 8, max_length=8)
    assert torch.equal(out["scored_steps"], out["lengths"])
    eng.close()


def test_same_bits_alone_batched_uncompacted_merged_and_with_early_exit(blip_tiny):
    from embodied_captioning_amd.engine import CaptionerEngine, EnginePool
    arch, sd, px = blip_tiny
    eng = CaptionerEngine(arch, dtype="f32s", max_batch=24, max_beams=1, max_len=L)
    eng.load_state_dict(sd)
    pxd = px.cuda()
    kw = dict(max_length=L, output_vocab_maxprob=True)
    full = eng.generate(pxd, **kw)
    assert eng.last_row_compaction and eng.last_decode_path == "batch"          # asking for the vector keeps the compacted loop
    vm = full["vocab_maxprob"].clone()
    assert len(set(full["scored_steps"].tolist())) > 1
    for r in range(24):                                                          # every frame alone: the small-batch kernels
        one = eng.generate(pxd[r:r + 1], **kw)
        assert eng.last_decode_path == "small" and not eng.last_row_compaction
        assert torch.equal(one["vocab_maxprob"], vm[r:r + 1]), r
    eng.set_row_compaction(False)
    off = eng.generate(pxd, **kw)
    assert not eng.last_row_compaction and torch.equal(off["vocab_maxprob"], vm)
    eng.set_row_compaction(True)
    eng.set_early_exit(1)
    early = eng.generate(pxd, **kw)
    assert eng.last_decode_steps <= L - 1 and torch.equal(early["vocab_maxprob"], vm)
    assert torch.equal(early["sequences"], full["sequences"])
    eng.set_early_exit(0)
    pool = EnginePool(arch, n=1, dtype="f32s", max_batch=24, max_beams=1, max_len=L, weights_of=eng)
    outs = pool.generate_many([pxd[0:8], pxd[8:16], pxd[16:24]], coalesce_rows=24, **kw)
    assert pool.last_coalesce == [[0, 1, 2]], pool.last_coalesce
    assert pool.engines[0].last_row_compaction
    for j, o in enumerate(outs):
        assert torch.equal(o["vocab_maxprob"], vm[8 * j:8 * j + 8]) and torch.equal(o["sequences"], full["sequences"][8 * j:8 * j + 8])
        assert torch.equal(o["scored_steps"], full["scored_steps"][8 * j:8 * j + 8])
    pool.close()
    eng.close()


def test_beams_are_refused_by_name_and_the_handle_still_works(blip_tiny):
    from embodied_captioning_amd._native import CaptionerHipError
    from embodied_captioning_amd.engine import CaptionerEngine
    arch, sd, px = blip_tiny
    eng = CaptionerEngine(arch, dtype="f32s", max_batch=4, max_beams=3, max_len=L)
    eng.load_state_dict(sd)
    with pytest.raises(CaptionerHipError, match="num_beams = 3"):
        eng.generate(px[:4].cuda(), num_beams=3, max_length=L, output_vocab_maxprob=True)
    assert "vocab_maxprob" in eng.generate(px[:4].cuda(), max_length=L, output_vocab_maxprob=True)
    eng.close()


GROUPS3 = [[5, 0, 3], [1], [7, 2, 6, 4]]


def _fuse_against_host(eng, out, want, bar, th, tag, eos=None, min_len=0):
    """fuse_vocab_groups over three groups == the host functions fed the same call's logits (float64).  A device mean is off by at
    most the largest member's bar (the mean of the members' errors) plus 4 fp32 spacings for its own sum and division."""
    from embodied_captioning_amd.captioner import pseudo_caption_fusion as F
    logits, sc = out["logits"].cpu(), out["scored_steps"].cpu()
    means = [group_mean64(want, g) for g in GROUPS3]
    print(f"vocab_fusion {tag}: top float64 group means " + " | ".join(" ".join(f"{v:.4f}" for v in np.sort(m)[::-1][:6]) for m in means))
    margin = min(assert_no_mean_in_band(m, th) for m in means)
    ids, probs, counts = eng.fuse_vocab_groups(out["vocab_maxprob"], GROUPS3, th)
    ids, probs, counts = ids.cpu(), probs.cpu(), counts.cpu()
    kept = 0
    for j, g in enumerate(GROUPS3):
        p = []
        for r in g:
            rows = logits[:int(sc[r]), r].double()
            for t in range(rows.shape[0]):
                if t + 1 < min_len:
                    rows[t, eos] = float("-inf")
            p.append(torch.softmax(rows, dim=-1))
        host_ids, host_p = F.pseudo_caption_tokens(p, float(np.float32(th)))
        c = int(counts[j])
        assert ids[j, :c].tolist() == host_ids.tolist() == kept64(means[j], th).tolist(), (tag, j)
        hp = host_p.numpy()
        assert (np.abs(probs[j, :c].double().numpy() - hp) <= 4.0 * spacing32(hp) + bar[g].max(axis=0)[host_ids.numpy()]).all(), (tag, j)
        assert F.decode_tokens(ids[j, :c].tolist(), lambda i: " ".join(map(str, i))) == F.generate_pseudo_caption(p, float(np.float32(th)), lambda i: " ".join(map(str, i)))
        kept += c
    assert kept > 0, tag                                                         # the threshold keeps something on this fixture
    print(f"vocab_fusion {tag}: th={th} kept={kept} margin_to_th={margin:.3e} (band {threshold_band(th):.3e})")
    with pytest.raises(Exception, match="max_tokens"):
        eng.fuse_vocab_groups(out["vocab_maxprob"], GROUPS3, 0.0, max_tokens=3)


def test_fused_groups_equal_the_host_functions_on_the_same_calls_logits_blip(blip_tiny):
    from embodied_captioning_amd.engine import CaptionerEngine
    arch, sd, px = blip_tiny
    eng = CaptionerEngine(arch, dtype="f32s", max_batch=8, max_beams=1, max_len=L)
    eng.load_state_dict(sd)
    out, want, bar = _check_one_call(eng, px[:8].cuda(), "blip-tiny f32s (fusion)", L - 1, max_length=L)
    _fuse_against_host(eng, out, want, bar, TH["blip"], "blip-tiny")
    eng.close()


def test_fused_groups_equal_the_host_functions_coca_and_blip2():
    from embodied_captioning_amd.config import Blip2Arch, CocaArch
    from embodied_captioning_amd.engine import CaptionerEngine
    from embodied_captioning_amd.weights import procedural_blip2_state_dict, procedural_coca_state_dict, synthetic_pixels
    arch = CocaArch.tiny()
    eng = CaptionerEngine(arch, dtype="f32s", max_batch=8, max_beams=1, max_len=arch.seq_len)
    eng.load_state_dict(procedural_coca_state_dict(arch, 1, eos_boost=4.0))
    out, want, bar = _check_one_call(eng, synthetic_pixels(8, arch.image_size, seed=3).cuda(), "coca-tiny f32s (fusion)", arch.seq_len - 1,
                                eos=arch.eos, min_len=arch.min_seq_len, max_length=arch.seq_len)
    _fuse_against_host(eng, out, want, bar, TH["coca"], "coca-tiny", eos=arch.eos, min_len=arch.min_seq_len)
    eng.close()
    arch = Blip2Arch.tiny()
    eng = CaptionerEngine(arch, dtype="f32s", max_batch=8, max_beams=1, max_len=8)
    eng.load_state_dict(procedural_blip2_state_dict(arch, 11, eos_boost=0.5))
    out, want, bar = _check_one_call(eng, synthetic_pixels(8, arch.image_size, seed=5).cuda(), "blip2-tiny f32s (fusion)", 8, max_length=8)
    _fuse_against_host(eng, out, want, bar, TH["blip2"], "blip2-tiny")
    eng.close()


def test_fused_pseudo_captions_through_the_product_api():
    from embodied_captioning_amd.captioner import pseudo_caption_fusion as F
    from embodied_captioning_amd.captioner.utils.utils import Configuration
    from embodied_captioning_amd.captioner.utils.utils_captioner import select_captioner
    model = select_captioner(Configuration(arch_name="blip", model_name="procedural-tiny:4:2.0", height=224, width=224, dtype="f32s",
                                           batch_size=4, max_length=L).captioner).eval()
    rng = np.random.default_rng(11)
    frames = [rng.integers(0, 256, size=(96, 128, 3), dtype=np.uint8), rng.integers(0, 256, size=(80, 100, 3), dtype=np.uint8)]
    boxes = [[(10, 12, 60, 70), (30, 5, 120, 90), (0, 0, 40, 40)], [(5, 5, 50, 60), (20, 10, 90, 70)]]
    objs = [[1, 1, 2], [1, 2]]
    grouped = {}
    for fr, bx, ob in zip(frames, boxes, objs):
        for b, o in zip(bx, ob):
            grouped.setdefault((0, o), []).append({"image": fr, "pred_box": np.array(b, np.float32)})
    th = TH["blip"]
    got = F.fused_pseudo_captions(grouped, model, th=th)
    assert list(got) == ["(0, 1)", "(0, 2)"] and [len(v["captions"]) for v in got.values()] == [3, 2]
    # the same crops through generate_batch with logits, fused on the host in float64
    from PIL import Image
    crops = [Image.fromarray(np.ascontiguousarray(i["image"][int(i["pred_box"][1]):int(i["pred_box"][3]), int(i["pred_box"][0]):int(i["pred_box"][2]), ::-1]))
             for k in grouped for i in grouped[k]]
    res = model.generate_batch(crops, output_logits=True, output_vocab_maxprob=True)
    assert res["vocab_maxprob"].is_cuda and res["vocab_maxprob"].shape == (5, model.arch.vocab)
    assert res["texts"] == [c for v in got.values() for c in v["captions"]]
    logits = torch.cat([l.cpu() for l in res["logits"]], dim=1)                  # [steps, 5, V]
    sc = res["scored_steps"]
    r0 = 0
    for k in grouped:
        n = len(grouped[k])
        p = [torch.softmax(logits[:int(sc[r]), r].double(), dim=-1) for r in range(r0, r0 + n)]
        mean = torch.stack([q.max(dim=0).values for q in p]).mean(dim=0).numpy()
        assert_no_mean_in_band(mean, th)
        assert got[str(k)]["pseudo_caption"] == F.generate_pseudo_caption(p, float(np.float32(th)), model)
        assert got[str(k)]["token_ids"] == kept64(mean, th).tolist()
        r0 += n
