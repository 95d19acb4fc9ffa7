"""GPU: text-prompted captioning (`CaptionerEngine.generate(prompt_ids=)`, cap_generate_prompted) - the prompt positions run as
one prefill pass, the greedy loop goes on from the last prompt token.

* against HF `BlipForConditionalGeneration.generate(pixel_values, input_ids=...)` on tests/golden/blip_tiny_prompt.npz and
  blip_base_prompt.npz (tools/make_goldens_prompt.py): identical tokens, logits within the project's 1e-3;
* OWN-PREFIX BIT IDENTITY, the kernel test: a caption prompted with its own first four tokens decodes to the bits of the unprompted
  call - sequences, lengths, every later step's logits row and log-prob - on the batch kernels, in the compacted loop and on the
  small-batch path: the prefill leaves the self-attention caches exactly as the single steps do;
* capacity edges (one pass with reserved capacity, chunks of captions without), merged pool passes, the plugin surface, and the
  refusal of a prompt by the BLIP-2 wrapper."""
import types

import numpy as np
import pytest
import torch

from _fusion_ref import prob_bar, softmax64
from _prompt_ref import full_margins, prompted_greedy
from _util import golden_inputs, token_parity

pytestmark = pytest.mark.gpu

BF16_TAU = 0.3            # tests/test_parity_gpu.py: a bf16 row may leave the oracle path only below this oracle margin
P4 = 4


def _engine(arch, dtype, batch, max_len, **kw):
    from embodied_captioning_amd.engine import CaptionerEngine
    return CaptionerEngine(arch, dtype=dtype, max_batch=batch, max_beams=1, max_len=max_len, **kw)


def _step_bar(rows32):
    """tests/test_logprob_generate_gpu.py's bar of a step's log max softmax: (float64 value [n], bar [n]) of fp32 rows [n, V]."""
    x = rows32.double().numpy()
    m = x.max(axis=1, keepdims=True)
    want = -np.log(np.exp(x - m).sum(axis=1))
    ref32 = torch.log_softmax(rows32, dim=-1).max(dim=-1).values.double().numpy()
    ref_err = float(np.abs(ref32 - want).max())
    return want, np.maximum(8.0 * ref_err, 4.0 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64))


# ------------------------------------------------------------------------------------------------ 1. tiny golden
@pytest.mark.parametrize("dtype", ["f32", "f32s"])
def test_tiny_prompt_golden_tokens_logits_and_perplexity(dtype):
    from oracle.blip_ref import compute_perplexity
    from embodied_captioning_amd.engine import perplexity_from_logprobs
    g, meta, arch, sd, px = golden_inputs("blip_tiny_prompt")
    B, L, prompt = meta["batch"], meta["max_length"], g["prompt_ids"].tolist()
    P = len(prompt)
    eng = _engine(arch, dtype, B, L, max_prompt=P)
    eng.load_state_dict(sd)
    out = eng.generate(px.cuda(), max_length=L, prompt_ids=prompt, output_logits=True, output_logprobs=True)
    assert eng.last_prefill_passes == 1
    seq = out["sequences"].cpu().numpy()
    assert np.array_equal(seq, g["greedy_sequences"]), (seq, g["greedy_sequences"])
    assert np.array_equal(seq[:, :P], np.tile(prompt, (B, 1)))
    assert np.array_equal(out["lengths"].cpu().numpy(), g["greedy_lengths"])
    logits = out["logits"].cpu()
    assert tuple(logits.shape) == (L - P, B, arch.vocab)
    live = g["greedy_live"]
    err = np.abs(logits.numpy() - g["greedy_logits_full"])[live]
    print(f"prompt tiny {dtype}: max |logit - HF| over live rows {err.max():.3e}")
    assert err.max() <= 1e-3
    lp, sc = out["token_logprobs"].cpu(), out["scored_steps"].cpu()
    assert tuple(lp.shape) == (B, L - 1) and np.array_equal(sc.numpy(), g["greedy_lengths"] - P)
    ppl = perplexity_from_logprobs(lp, sc)
    for b in range(B):
        n = int(sc[b])
        assert float(lp[b, n:].abs().max()) == 0.0                         # the unused tail stays zero
        # (a) against compute_perplexity of the library's OWN logits: the tolerance of tests/test_logprob_generate_gpu.py
        own_rows = logits[:n, b]
        lp64, bar = _step_bar(own_rows)
        want32 = float(compute_perplexity([r[None] for r in own_rows]))
        own = abs(np.log(want32) + lp64.sum() / n)
        d_own = abs(np.log(float(ppl[b])) - np.log(want32))
        assert (np.abs(lp[b, :n].double().numpy() - lp64) <= bar).all() and d_own <= bar.max() + own, (b, d_own, bar.max(), own)
        # (b) against compute_perplexity of the GOLDEN logits: the same tolerance, plus what THIS row's logits differ from HF's by -
        # two logits rows within d of each other have log max softmax values within 2 d (the maximum moves by at most d, the
        # log-sum-exp by at most d), and so has their mean over the steps; d is measured on the row's scored steps
        hf_rows = torch.from_numpy(g["greedy_logits_full"][:n, b])
        dev = float((own_rows - hf_rows).abs().max())
        hf64, hbar = _step_bar(hf_rows)
        hf32 = float(compute_perplexity([r[None] for r in hf_rows]))
        d_hf = abs(np.log(float(ppl[b])) - np.log(hf32))
        tol_hf = hbar.max() + abs(np.log(hf32) + hf64.sum() / n)
        print(f"prompt tiny {dtype} row {b}: |d ln ppl| own {d_own:.3e}, golden {d_hf:.3e} (tolerance {tol_hf:.3e} + 2 x {dev:.3e})")
        assert d_hf <= tol_hf + 2.0 * dev, (b, d_hf, tol_hf, dev)
    eng.close()


def test_tiny_prompt_golden_bf16_token_parity():
    g, meta, arch, sd, px = golden_inputs("blip_tiny_prompt")
    B, L, prompt = meta["batch"], meta["max_length"], g["prompt_ids"].tolist()
    eng = _engine(arch, "bf16", B, L, max_prompt=len(prompt))
    eng.load_state_dict(sd)
    seq = eng.generate(px.cuda(), max_length=L, prompt_ids=prompt)["sequences"].cpu().numpy()
    exact, diverged, bad = token_parity(seq, g["greedy_sequences"], full_margins(g["greedy_margin"], len(prompt), L), BF16_TAU)
    print(f"prompt tiny bf16: {exact} exact rows, {diverged} diverged at near-ties")
    assert bad is None, bad
    assert np.array_equal(seq[:, :len(prompt)], np.tile(prompt, (B, 1)))
    eng.close()


# ------------------------------------------------------------------------------------------------ 2. base golden
@pytest.fixture(scope="module")
def base_engine():
    """One BLIP-base f32s engine for the base-sized tests (32 rows, capacity for a 4-token prompt in one pass)."""
    g, meta, arch, sd, px = golden_inputs("blip_base256")
    eng = _engine(arch, "f32s", 32, meta["max_length"], max_prompt=P4)
    eng.load_state_dict(sd)
    yield eng
    eng.close()


@pytest.mark.parametrize("path", ["batch", "small"])
def test_base_prompt_golden_on_both_decode_paths(base_engine, path):
    g, meta, arch, sd, px = golden_inputs("blip_base_prompt")
    B, L, prompt = meta["batch"], meta["max_length"], g["prompt_ids"].tolist()
    P = len(prompt)
    eng = base_engine
    eng.set_decode_path(path)
    try:
        out = eng.generate(px.cuda(), max_length=L, prompt_ids=prompt, output_logits=True)
        assert eng.last_decode_path == path and eng.last_prefill_passes == 1
    finally:
        eng.set_decode_path("auto")
    assert np.array_equal(out["sequences"].cpu().numpy(), g["greedy_sequences"])
    assert np.array_equal(out["lengths"].cpu().numpy(), g["greedy_lengths"])
    top = torch.topk(out["logits"].cpu(), 8, dim=-1)
    live = g["greedy_live"]
    assert tuple(top.values.shape) == (L - P, B, 8)
    assert np.array_equal(top.indices.numpy()[live], g["greedy_top8_ids"][live])
    err = np.abs(top.values.numpy() - g["greedy_top8_vals"])[live]
    print(f"prompt base f32s {path}: max |top-8 value - HF| {err.max():.3e}")
    assert err.max() <= 1e-3


# ------------------------------------------------------------------------------------------------ 3. own-prefix bit identity
def _own_prefix_rows(g, arch, n_frames):
    ref = np.asarray(g["greedy_sequences"])[:n_frames]
    lens = np.array([list(r[1:]).index(arch.eos) + 2 if arch.eos in r[1:] else len(r) for r in ref])
    return ref, lens, np.nonzero(lens >= P4 + 1)[0]


@pytest.mark.parametrize("dtype", ["f32s", "bf16"])
def test_own_prefix_prompt_gives_the_unprompted_bits(base_engine, dtype):
    g, meta, arch, sd, px = golden_inputs("blip_base256")
    L = meta["max_length"]
    ref, ref_len, rows = _own_prefix_rows(g, arch, 32)
    assert len(rows) >= 24, len(rows)                                   # the batch kernels and the compacted loop are what runs
    assert int((ref_len[rows] < L).sum()) >= 4                          # captions that end early: rows leave the compacted loop
    eng = base_engine if dtype == "f32s" else _engine(arch, dtype, 32, L, max_prompt=P4)
    if dtype != "f32s":
        eng.load_state_dict(sd)
    pxd = px[:32][rows].cuda()
    prompt = torch.from_numpy(ref[rows, :P4].astype(np.int64))
    base_l = eng.generate(pxd, max_length=L, output_logits=True)
    if dtype == "f32s":
        assert np.array_equal(base_l["sequences"].cpu().numpy(), ref[rows])          # the library is on HF's path: own prefix = golden prefix
        keep = np.arange(len(rows))
    else:
        # bf16 may have left HF's path at a near-tie inside the first four tokens: such a row's golden prefix is not its OWN prefix
        keep = np.nonzero((base_l["sequences"].cpu().numpy()[:, :P4] == ref[rows, :P4]).all(axis=1))[0]
        assert len(keep) >= 24, len(keep)
        assert int((ref_len[rows][keep] < L).sum()) >= 4                # rows still leave the compacted loop early in this leg
        pxd, prompt = pxd[torch.from_numpy(keep).cuda()], prompt[keep]
        base_l = eng.generate(pxd, max_length=L, output_logits=True)
    n = len(keep)
    # with per-step logits: the uncompacted batch loop
    got_l = eng.generate(pxd, max_length=L, prompt_ids=prompt, output_logits=True)
    assert eng.last_decode_path == "batch" and not eng.last_row_compaction and eng.last_prefill_passes == 1
    assert torch.equal(got_l["sequences"], base_l["sequences"]) and torch.equal(got_l["lengths"], base_l["lengths"])
    assert tuple(got_l["logits"].shape) == (L - P4, n, arch.vocab)
    lens = base_l["lengths"].cpu().numpy()
    assert int((lens < L).sum()) >= 4
    # logits are compared for the rows still open at a step: in the uncompacted loop the attention kernels skip a finished caption's
    # row, so what the vocabulary GEMM writes for it is stale in BOTH calls and never read (every live step of every row is covered)
    for j in range(L - P4):
        open_rows = torch.from_numpy(np.nonzero(lens > j + P4)[0]).cuda()          # the step that wrote token j + P4 ran for these
        assert torch.equal(got_l["logits"][j][open_rows], base_l["logits"][j + P4 - 1][open_rows]), (dtype, j)
    # without: the compacted loop, log-probs from the selection kernel
    base_c = eng.generate(pxd, max_length=L, output_logprobs=True)
    got_c = eng.generate(pxd, max_length=L, prompt_ids=prompt, output_logprobs=True)
    assert eng.last_row_compaction and eng.last_decode_path == "batch"
    assert torch.equal(got_c["sequences"], base_c["sequences"]) and torch.equal(got_c["lengths"], base_c["lengths"])
    assert torch.equal(got_c["sequences"], base_l["sequences"])
    assert torch.equal(got_c["token_logprobs"][:, :L - P4], base_c["token_logprobs"][:, P4 - 1:])
    assert torch.equal(got_c["scored_steps"], base_c["scored_steps"] - (P4 - 1))
    assert float(got_c["token_logprobs"][:, L - P4:].abs().max()) == 0.0
    # the first five usable rows: the small-batch path
    five = eng.generate(pxd[:5], max_length=L, prompt_ids=prompt[:5], output_logits=True, output_logprobs=True)
    assert eng.last_decode_path == "small" and not eng.last_row_compaction
    assert torch.equal(five["sequences"], base_l["sequences"][:5]) and torch.equal(five["lengths"], base_l["lengths"][:5])
    assert torch.equal(five["token_logprobs"][:, :L - P4], base_c["token_logprobs"][:5, P4 - 1:])
    for j in range(L - P4):
        open_rows = torch.from_numpy(np.nonzero(lens[:5] > j + P4)[0]).cuda()
        assert torch.equal(five["logits"][j][open_rows], base_l["logits"][j + P4 - 1][:5][open_rows]), (dtype, "small", j)
    if dtype != "f32s":
        eng.close()


# ------------------------------------------------------------------------------------------------ 4. capacity edges
@pytest.fixture(scope="module")
def tiny_long():
    """Tiny architecture, 17 frames, 36 positions: each caption's own 32-token prefix (the longest prompt the library takes), padded
    with fixed ids where the caption is shorter, and the forced-token restatement of that call on the CPU (computed once)."""
    from oracle import blip_ref
    from embodied_captioning_amd.config import BlipArch
    from embodied_captioning_amd.engine import N
    from embodied_captioning_amd.weights import procedural_blip_state_dict, synthetic_pixels
    arch = BlipArch.tiny()
    L, P = 36, N.CAP_MAX_PROMPT
    sd = procedural_blip_state_dict(arch, 5, eos_boost=1.0)
    px = synthetic_pixels(17, arch.image_size, seed=11)
    own = blip_ref.greedy_generate(sd, arch, px, max_length=L)["sequences"].numpy()
    prompt = np.zeros((17, P), dtype=np.int64)
    for b in range(17):
        row = list(own[b])
        n = min([j for j, t in enumerate(row) if t in (arch.eos, arch.pad)] + [P])     # own tokens before the EOS (or a pad id)
        prompt[b, :n] = row[:n]
        prompt[b, n:] = [20 + (7 * b + 3 * j) % 60 for j in range(n, P)]       # fixed filler: never BOS (510), EOS (102) or pad (0)
    ref = prompted_greedy(sd, arch, px, prompt, L)
    return arch, sd, px, prompt, L, ref


def _check_against_restatement(out, ref, rows, P, L, dtype):
    """Tokens as the restatement's wherever its top-2 margin exceeds what the logit bar admits (two logits within 1e-3 of the fp32
    values can swap only when they are within 2e-3), logits within 1e-3 on the rows still on the restatement's path."""
    seq = out["sequences"].cpu().numpy()
    want = ref["sequences"].numpy()[:rows]
    margins = full_margins(ref["margins"].numpy()[:, :rows], P, L)
    exact, diverged, bad = token_parity(seq, want, margins, 2e-3)
    assert bad is None, (dtype, rows, bad)
    T = ref["logits"].shape[0]
    worst = 0.0
    for b in range(rows):
        for j in range(min(T, L - P)):
            if not np.array_equal(seq[b, :P + j], want[b, :P + j]) or margins[P - 1 + j, b] >= 1e8:
                break
            worst = max(worst, float((out["logits"][j, b].cpu() - ref["logits"][j, b]).abs().max()))
    print(f"prompt capacity {dtype} rows {rows}: {exact} exact rows, max |logit - restatement| {worst:.3e}")
    assert worst <= 1e-3


@pytest.mark.parametrize("rows", [1, 3, 17])
@pytest.mark.parametrize("dtype", ["f32", "f32s"])
def test_longest_prompt_with_reserved_capacity_is_one_pass(tiny_long, rows, dtype):
    arch, sd, px, prompt, L, ref = tiny_long
    P = prompt.shape[1]
    eng = _engine(arch, dtype, rows, L, max_prompt=P)
    assert eng.prompt_limit == P
    eng.load_state_dict(sd)
    out = eng.generate(px[:rows].cuda(), max_length=L, prompt_ids=prompt[:rows], output_logits=True)
    assert eng.last_prefill_passes == 1
    assert np.array_equal(out["sequences"].cpu().numpy()[:, :P], prompt[:rows])
    _check_against_restatement(out, ref, rows, P, L, dtype)
    # a prompt beyond the library's limit, and one beyond this engine's, are refused on the host with the limit named
    with pytest.raises(ValueError, match=f"limit is {P}"):
        eng.generate(px[:rows].cuda(), max_length=L + 2, prompt_ids=np.concatenate([prompt[:rows], prompt[:rows, -1:]], axis=1))
    eng.close()


def test_prefill_in_chunks_of_captions_without_reserved_capacity(tiny_long):
    """max_batch 17 and no prompt capacity: 17 workspace rows, an 8-token prompt = 7 rows per caption -> 2 captions per pass, nine
    passes, the last with one caption; the same bits as the engine that holds the batch in one pass."""
    arch, sd, px, prompt, L, ref = tiny_long
    P = 8
    one = _engine(arch, "f32s", 17, L, max_prompt=P)
    one.load_state_dict(sd)
    chunked = _engine(arch, "f32s", 17, L)
    chunked.load_state_dict(sd)
    assert chunked.prompt_limit == 18 and chunked.device_bytes < one.device_bytes
    a = one.generate(px.cuda(), max_length=L, prompt_ids=prompt[:, :P], output_logits=True)
    assert one.last_prefill_passes == 1
    b = chunked.generate(px.cuda(), max_length=L, prompt_ids=prompt[:, :P], output_logits=True)
    assert chunked.last_prefill_passes == 9
    assert torch.equal(a["sequences"], b["sequences"]) and torch.equal(a["lengths"], b["lengths"]) and torch.equal(a["logits"], b["logits"])
    # and the library refuses, at entry, what the workspace cannot take: 17 rows hold 17 positions
    from embodied_captioning_amd.engine import N
    with pytest.raises(ValueError, match="limit is 18"):
        chunked.generate(px.cuda(), max_length=L, prompt_ids=prompt[:, :19])
    unprompted = chunked.generate(px.cuda(), max_length=L)
    assert chunked.last_prefill_passes == 0 and int(unprompted["sequences"][0, 0]) == arch.bos
    one.close(); chunked.close()


def test_handle_without_prompt_capacity_allocates_what_it_always_did():
    """CapConfig.max_prompt = 0 leaves the arena alone; the library's own entry check names its limit before any launch."""
    import ctypes as C
    from embodied_captioning_amd.config import BlipArch
    from embodied_captioning_amd.engine import N
    from embodied_captioning_amd.weights import procedural_blip_state_dict, synthetic_pixels
    arch = BlipArch.tiny()
    plain, cap4 = _engine(arch, "f32s", 2, 12), _engine(arch, "f32s", 2, 12, max_prompt=2)
    assert plain.device_bytes == cap4.device_bytes            # max_prompt 2 = one position per caption = the decode rows
    big = _engine(arch, "f32s", 2, 12, max_prompt=9)
    assert big.device_bytes > plain.device_bytes
    plain.load_state_dict(procedural_blip_state_dict(arch, 3, eos_boost=2.0))
    px = synthetic_pixels(2, arch.image_size, seed=3).cuda()
    ids = torch.empty((2, 12), dtype=torch.int32, device="cuda")
    bad = torch.tensor([[arch.bos, 11, 12, 13]], dtype=torch.int32, device="cuda")      # 3 positions > 2 workspace rows
    rc = plain.lib.cap_generate_prompted(plain._h, C.c_void_p(px.data_ptr()), N.CAP_PIX_F32_NCHW, 2, 12, C.c_void_p(bad.data_ptr()), 1, 4,
                                         C.c_void_p(ids.data_ptr()), None, None, None, None, None, 0,
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc != 0 and "limit of 3 tokens" in N.last_error(), N.last_error()
    for e in (plain, cap4, big):
        e.close()


# ------------------------------------------------------------------------------------------------ 5. merged passes
def test_pool_merged_prompted_passes_equal_the_separate_calls():
    from embodied_captioning_amd.config import BlipArch
    from embodied_captioning_amd.engine import EnginePool
    from embodied_captioning_amd.weights import procedural_blip_state_dict, synthetic_pixels
    arch, L = BlipArch.tiny(), 12
    sd = procedural_blip_state_dict(arch, 5, eos_boost=2.0)
    px = synthetic_pixels(24, arch.image_size, seed=7).cuda()
    eng = _engine(arch, "f32s", 24, L, max_prompt=P4)
    eng.load_state_dict(sd)
    pool = EnginePool(arch, n=1, dtype="f32s", max_batch=24, max_beams=1, max_len=L, weights_of=eng, max_prompt=P4)
    batches = [px[0:8], px[8:16], px[16:24]]
    shared = [arch.bos, 31, 47, 59]
    rng = np.random.default_rng(2)
    per_row = [np.concatenate([np.full((8, 1), arch.bos), rng.integers(10, 100, size=(8, P4 - 1))], axis=1) for _ in range(3)]
    kw = dict(max_length=L, output_logprobs=True)
    for prompts, per_batch in ((shared, [shared] * 3), (per_row, per_row)):
        sep = [eng.generate(b, prompt_ids=p, **kw) for b, p in zip(batches, per_batch)]
        merged = pool.generate_many(batches, coalesce_rows=24, prompt_ids=prompts, **kw)
        assert pool.last_coalesce == [[0, 1, 2]], pool.last_coalesce
        assert pool.engines[0].last_prefill_passes == 1 and pool.engines[0].last_row_compaction
        for j, (a, b) in enumerate(zip(sep, merged)):
            for k in ("sequences", "lengths", "token_logprobs", "scored_steps"):
                assert torch.equal(a[k], b[k]), (j, k)
            assert np.array_equal(b["sequences"][:, :P4].cpu().numpy(), np.broadcast_to(np.asarray(per_batch[j]), (8, P4)))
    # batches whose prompt lengths differ are never merged
    mixed = pool.generate_many(batches, coalesce_rows=24, prompt_ids=[shared, shared[:3], shared], **kw)
    assert pool.last_coalesce is None or all(len(g) == 1 for g in pool.last_coalesce) or isinstance(pool.last_coalesce, str)
    assert torch.equal(mixed[1]["sequences"], eng.generate(batches[1], prompt_ids=shared[:3], **kw)["sequences"])
    pool.close(); eng.close()


# ------------------------------------------------------------------------------------------------ 6. plugin
def _pil(seed, size=(48, 40)):
    from PIL import Image
    rng = np.random.default_rng(seed)
    return Image.fromarray(rng.integers(0, 256, size=(size[1], size[0], 3), dtype=np.uint8), "RGB")


def test_plugin_forward_and_generate_batch_use_the_configured_prompt():
    from embodied_captioning_amd.captioner.utils.utils import Configuration
    from embodied_captioning_amd.captioner.utils.utils_captioner import select_captioner
    prompt = [510, 31, 47, 59]
    kw = dict(arch_name="blip", model_name="procedural-tiny:4:2.0", height=224, width=224, dtype="f32s", batch_size=4, max_length=12)
    model = select_captioner(Configuration(prompt_ids=prompt, **kw).captioner).eval()
    plain = select_captioner(Configuration(**kw).captioner).eval()
    assert model.engine.max_prompt == 4 and plain.engine.max_prompt == 0
    crops = [_pil(1), _pil(2), _pil(3)]
    out = model.generate_batch(crops, output_logits=True)
    assert out["sequences"][:, :4].tolist() == [prompt] * 3
    for i, crop in enumerate(crops):
        one = model(crop)
        n = int(out["lengths"][i])
        assert one["text"] == out["texts"][i] and one["text"].split()[:3] == ["31", "47", "59"]      # the prompt's words are in the text
        assert len(one["logits"]) == n - 4                                                             # the generated steps
        for j, row in enumerate(one["logits"]):
            assert torch.equal(row[0], out["logits"][0][j][i]), (i, j)
    # a call's own prompt overrides the configured one; the unconfigured model takes one per call (prefilled in chunks)
    other = [510, 77, 78]
    o2 = model.generate_batch(crops, prompt_ids=other)
    assert o2["sequences"][:, :3].tolist() == [other] * 3
    o3 = plain.generate_batch(crops, prompt_ids=prompt)
    assert o3["texts"] == out["texts"] and torch.equal(o3["sequences"], out["sequences"])
    assert plain.generate_batch(crops)["sequences"][:, 1].tolist() != [31] * 3
    with pytest.raises(ValueError, match="no tokenizer"):
        plain.generate_batch(crops, prompt="a picture of")


def test_captioner_forwards_the_prompt_key_and_blip2_refuses_it():
    from embodied_captioning_amd.utils.predictor_utils import Captioner
    prompt = [510, 31, 47, 59]
    cap_cfg = types.SimpleNamespace(arch_name="blip", model_name="procedural-tiny:4:2.0", checkpoint_name=None, height=224, width=224,
                                    dtype="f32s", batch_size=4, max_length=12, prompt_ids=prompt)
    cap = Captioner(types.SimpleNamespace(captioner=cap_cfg)).eval()
    assert cap.model.prompt_ids == prompt and cap.model.engine.max_prompt == 4            # the key reached the built model
    texts = cap.caption_batch([_pil(1), _pil(2)])
    assert all(t.split()[:3] == ["31", "47", "59"] for t in texts)
    assert cap.forward(_pil(1)) == texts[0]
    assert cap.caption_batch([_pil(1)], prompt_ids=[510, 77])[0].split()[0] == "77"
    # BLIP-2: the prompt is not built - the key is refused by name, never dropped
    b2 = types.SimpleNamespace(arch_name="blip2", model_name="procedural-blip2:1", checkpoint_name=None, height=224, width=224,
                               prompt="Question: what is this? Answer:")
    with pytest.raises(ValueError, match="captioner.prompt"):
        Captioner(types.SimpleNamespace(captioner=b2))


def test_vocab_maxprob_with_a_prompt_covers_the_generated_steps():
    g, meta, arch, sd, px = golden_inputs("blip_tiny_prompt")
    B, L, prompt = meta["batch"], meta["max_length"], g["prompt_ids"].tolist()
    eng = _engine(arch, "f32s", B, L, max_prompt=len(prompt))
    eng.load_state_dict(sd)
    out = eng.generate(px.cuda(), max_length=L, prompt_ids=prompt, output_logits=True, output_vocab_maxprob=True)
    plain = eng.generate(px.cuda(), max_length=L, prompt_ids=prompt)
    assert set(plain) == {"sequences", "lengths"} and torch.equal(plain["sequences"], out["sequences"])
    assert np.array_equal(out["sequences"].cpu().numpy(), g["greedy_sequences"])
    sc = out["scored_steps"].cpu()
    assert np.array_equal(sc.numpy(), g["greedy_lengths"] - len(prompt))
    logits = out["logits"].cpu()
    for b in range(B):
        # the maximum over the caption's GENERATED steps of the step's softmax, from the returned logits in float64, to the bar of
        # tests/test_vocab_fusion_generate_gpu.py (tests/_fusion_ref.prob_bar)
        rows = logits[:int(sc[b]), b]
        want = softmax64(rows).max(axis=0)
        bar, _ = prob_bar(rows, want)
        err = np.abs(out["vocab_maxprob"][b].cpu().double().numpy() - want)
        print(f"prompt vocab_maxprob row {b}: max error over bar {float((err / bar).max()):.3f}")
        assert (err <= bar).all()
    eng.close()


def test_plugin_pool_slices_per_image_prompts_across_micro_batches():
    """captioner.streams 2, micro-batches of 4: ten crops with one prompt per image through the wrapper's pool (merged passes, and
    preprocessing rounds when the list is longer than a round) give what the one-engine wrapper gives image by image."""
    from embodied_captioning_amd.captioner.utils.utils import Configuration
    from embodied_captioning_amd.captioner.utils.utils_captioner import select_captioner
    kw = dict(arch_name="blip", model_name="procedural-tiny:4:2.0", height=224, width=224, dtype="f32s", batch_size=4, max_length=12,
              max_prompt=4)
    one = select_captioner(Configuration(**kw).captioner).eval()
    crops = [_pil(s) for s in range(10)]
    rng = np.random.default_rng(9)
    rows = np.concatenate([np.full((10, 1), 510), rng.integers(10, 100, size=(10, 3))], axis=1).tolist()
    want = one.generate_batch(crops, prompt_ids=rows)
    assert want["sequences"][:, :4].tolist() == rows
    for i in (0, 5, 9):                                                    # image i alone with its own prompt
        assert one.generate_batch([crops[i]], prompt_ids=rows[i])["texts"][0] == want["texts"][i]
    for coalesce in (0, 8, None):                                          # every micro-batch its own pass / merged pairs / default
        many = select_captioner(Configuration(streams=2, coalesce_rows=coalesce, **kw).captioner).eval()
        got = many.generate_batch(crops, prompt_ids=rows)
        assert got["texts"] == want["texts"] and torch.equal(got["sequences"], want["sequences"]), coalesce
        shared = many.generate_batch(crops, prompt_ids=rows[0])
        assert torch.equal(shared["sequences"], one.generate_batch(crops, prompt_ids=rows[0])["sequences"])
    with pytest.raises(ValueError, match="3 rows for 10 images"):
        one.generate_batch(crops, prompt_ids=rows[:3])
