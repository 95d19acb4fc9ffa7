"""GPU: sampling end to end (`CaptionerEngine.set_sampling`, cap_set_sampling) on the fixture-size BLIP and BLIP-2 models.

* REPLAY: a sampled call returns its own raw step logits; for every emitted token of every row the uniform U is recomputed on the
  host from (seed, the caption's key, the step j) and the token must satisfy the interval rule of tests/_sampling_ref.py on that row
  of logits and the caption's context as HF's processors see it - also with a penalty, an n-gram size and a ban set in force, and
  behind a prompt (the step index does not count prompt positions).
* top_k = 1 is the arg-max: the greedy call's sequences and lengths, bit for bit.
* SAME BITS for a caption with the same key: alone, in its batch, on the small-batch path, from an image state, in the compacted
  loop, in a pool's merged pass.
* different keys or seeds give different captions (on a fixture asserted to be flat enough); num_return_sequences; set -> reset;
  `score` ignores the state; the refusals, by message."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

import _sampling_ref as S
from _repeat_ref import blip2_context

pytestmark = pytest.mark.gpu

L_BLIP = 16
SEED = 0xC0FFEE_0000_0001
SETTINGS = [(0.7, 50, 0.9), (1.0, 0, 1.0), (1.3, 0, 0.8), (1.0, 5, 1.0)]      # (temperature, top_k, top_p)


def _blip(batch, seed=5):
    from embodied_captioning_amd.config import BlipArch
    from embodied_captioning_amd.weights import procedural_blip_state_dict, synthetic_pixels
    arch = BlipArch.tiny()
    return arch, _sd(f"blip{seed}", lambda: procedural_blip_state_dict(arch, seed, eos_boost=1.0)), synthetic_pixels(batch, arch.image_size, seed=seed)


def _blip2(batch, seed=5, **over):
    from embodied_captioning_amd.config import Blip2Arch
    from embodied_captioning_amd.weights import procedural_blip2_state_dict, synthetic_pixels
    arch = dataclasses.replace(Blip2Arch.tiny(), **over)
    key = "blip2" + repr(sorted(over.items()))
    return arch, _sd(key, lambda: procedural_blip2_state_dict(arch, seed, eos_boost=0.3)), synthetic_pixels(batch, arch.image_size, seed=seed)


_SD = {}


def _sd(key, make):
    if key not in _SD:
        _SD[key] = make()
    return _SD[key]


def _engine(arch, sd, dtype, batch, max_len, beams=1, **kw):
    from embodied_captioning_amd.engine import CaptionerEngine
    eng = CaptionerEngine(arch, dtype=dtype, max_batch=batch, max_beams=beams, max_len=max_len, **kw)
    eng.load_state_dict(sd)
    return eng


def _keys(n, base=0):
    """int64 keys with both words in use."""
    return torch.from_numpy(((np.arange(n, dtype=np.uint64) + np.uint64(base)) * np.uint64(0x9E3779B97F4A7C15)).view(np.int64).copy())


def _generated(seq, lens, b, blip2):
    n = int(lens[b])
    return [int(t) for t in (seq[b, :n] if blip2 else seq[b, 1:n])]


def _same(a, b, keys=("sequences", "lengths")):
    return all(torch.equal(a[k], b[k]) for k in keys)


def _replay(arch, out, keys, setting, seed, blip2, prompt=None, penalty=1.0, ngram=0, seqs=()):
    """Every emitted token of every row satisfies the interval rule for its own uniform.  -> (steps replayed, steps at which the token
    is not the raw row's arg-max, the mean number of tokens left by the cuts)."""
    T, k, p = setting
    seq, lens, logits = out["sequences"].cpu().numpy(), out["lengths"].cpu().numpy(), out["logits"].cpu().numpy()
    ku = keys.numpy().view(np.uint64)
    steps = moved = 0
    kept = []
    for b in range(seq.shape[0]):
        gen = _generated(seq, lens, b, blip2)
        if prompt is not None:
            assert gen[:len(prompt) - 1] == list(prompt[1:])
            gen, done = gen[len(prompt) - 1:], list(prompt)
        else:
            done = [] if blip2 else [arch.bos]
        for j, tok in enumerate(gen):
            ctx = blip2_context(done, arch.num_query_tokens, arch.image_token, arch.bos) if blip2 else done
            ban_ctx = [arch.bos] + done if blip2 else done
            ref = S.reference(logits[j, b], T, k, p, context=ctx, penalty=penalty, ngram=ngram, seqs=seqs, eos=arch.eos, ban_context=ban_ctx)
            U = S.uniform64(seed, int(ku[b]), j)
            bad = S.check_draw(ref, tok, U)
            assert bad is None, (b, j, bad, ref["kept"], ref["topp_margin"], S.delta(ref))
            moved += int(tok != int(np.argmax(logits[j, b])))
            kept.append(ref["kept"])
            done = done + [tok]
            steps += 1
    return steps, moved, float(np.mean(kept))


@pytest.mark.parametrize("family,dtype", [("blip", "f32s"), ("blip", "bf16"), ("blip2", "bf16")])
def test_replay_every_token_satisfies_the_interval_rule(family, dtype):
    blip2 = family == "blip2"
    B = 8
    arch, sd, px = (_blip2 if blip2 else _blip)(B)
    L = arch.max_new_tokens if blip2 else L_BLIP
    eng = _engine(arch, sd, dtype, B, L)
    assert eng.sampling == (False, 1.0, 0, 1.0, 0) and not eng.do_sample
    keys = _keys(B, 3)
    total = 0
    for T, k, p in SETTINGS:
        eng.set_sampling(True, T, k, p, SEED)
        assert eng.sampling == (True, float(np.float32(T)), k, float(np.float32(p)), SEED)
        assert (eng.do_sample, eng.temperature, eng.top_k, eng.top_p, eng.sample_seed) == eng.sampling
        out = eng.generate(px.cuda(), max_length=L, output_logits=True, sample_keys=keys, do_sample=True, temperature=T, top_k=k, top_p=p)
        steps, moved, kept = _replay(arch, out, keys, (T, k, p), SEED, blip2)
        total += moved
        print(f"\n{family} {dtype} T={T} k={k} p={p}: {steps} emitted tokens replayed, {moved} are not the arg-max, {kept:.1f} tokens left "
              f"by the cuts on average")
    assert total > 0, "no drawn token differs from the arg-max: the fixture gives sampling nothing to do"
    # with a penalty, an n-gram size and a ban set in force (HF's order: processors, then the warpers)
    eng.set_sampling(True, 0.9, 40, 0.95, SEED)
    eng.set_repeat_controls(1.4, 2)
    mid = eng.generate(px.cuda(), max_length=L, sample_keys=keys)
    s, ln = mid["sequences"].cpu().numpy(), mid["lengths"].cpu().numpy()
    special = {arch.bos, arch.pad, arch.eos} | ({arch.image_token} if blip2 else set())
    seqs = [[t] for t in sorted({_generated(s, ln, b, blip2)[0] for b in range(B)} - special)][:3]
    assert seqs
    eng.set_bad_words(seqs)
    out = eng.generate(px.cuda(), max_length=L, output_logits=True, sample_keys=keys)
    steps, moved, kept = _replay(arch, out, keys, (0.9, 40, 0.95), SEED, blip2, penalty=1.4, ngram=2, seqs=seqs)
    banned = {q[0] for q in seqs}
    assert all(_generated(out["sequences"].cpu().numpy(), out["lengths"].cpu().numpy(), b, blip2)[0] not in banned for b in range(B))
    print(f"\n{family} {dtype} with penalty 1.4, n = 2 and {len(seqs)} banned tokens: {steps} tokens replayed, {moved} not the arg-max")
    eng.close()


def test_prompted_replay_the_step_index_does_not_count_the_prompt():
    B = 8
    arch, sd, px = _blip(B)
    eng = _engine(arch, sd, "f32s", B, L_BLIP, max_prompt=4)
    prompt = [arch.bos, 31, 47, 31]
    keys = _keys(B, 11)
    eng.set_sampling(True, 0.8, 30, 0.9, SEED)
    eng.set_repeat_controls(1.3, 2)
    out = eng.generate(px.cuda(), max_length=L_BLIP, prompt_ids=prompt, output_logits=True, sample_keys=keys)
    assert torch.equal(out["sequences"][:, :len(prompt)].cpu(), torch.tensor([prompt] * B, dtype=torch.int32))
    steps, moved, _ = _replay(arch, out, keys, (0.8, 30, 0.9), SEED, False, prompt=prompt, penalty=1.3, ngram=2)
    print(f"\nprompted: {steps} generated tokens replayed, {moved} not the arg-max")
    eng.close()


@pytest.mark.parametrize("family,dtype", [("blip", "f32s"), ("blip2", "bf16")])
def test_top_k_1_is_the_greedy_call(family, dtype):
    blip2 = family == "blip2"
    B = 8
    arch, sd, px = (_blip2 if blip2 else _blip)(B)
    L = arch.max_new_tokens if blip2 else L_BLIP
    eng = _engine(arch, sd, dtype, B, L)
    free = eng.generate(px.cuda(), max_length=L, output_logits=True)
    # tie-free maxima, asserted on the call's own logits: top_k = 1 keeps every entry tied with the maximum
    lg, ln = free["logits"].cpu().numpy(), free["lengths"].cpu().numpy()
    for b in range(B):
        for j in range(int(ln[b]) - (0 if blip2 else 1)):
            assert (lg[j, b] == lg[j, b].max()).sum() == 1
    for T in (1.0, 0.7):
        eng.set_sampling(True, T, 1, 1.0, SEED)
        assert _same(eng.generate(px.cuda(), max_length=L), free)
    eng.close()


def _sampled_blip_engine(B, setting=(1.0, 0, 0.95), dtype="f32s", seed=5, **kw):
    arch, sd, px = _blip(B, seed=seed)
    eng = _engine(arch, sd, dtype, B, L_BLIP, **kw)
    eng.set_sampling(True, *setting, SEED)
    return arch, sd, px, eng


def test_row_alone_small_path_and_image_state_give_the_batch_bits():
    B = 6
    arch, sd, px, eng = _sampled_blip_engine(B)
    keys = _keys(B, 40)
    eng.set_decode_path("batch")
    ref = eng.generate(px.cuda(), max_length=L_BLIP, output_logits=True, sample_keys=keys)
    assert eng.last_decode_path == "batch"
    _replay(arch, ref, keys, (1.0, 0, 0.95), SEED, False)
    for b in (0, 3, 5):
        one = eng.generate(px[b:b + 1].cuda(), max_length=L_BLIP, sample_keys=keys[b:b + 1])
        assert torch.equal(one["sequences"][0], ref["sequences"][b]) and torch.equal(one["lengths"][0], ref["lengths"][b])
    # the key is the caption's, not the row's: the batch reversed, with its keys reversed
    rev = eng.generate(px.flip(0).cuda(), max_length=L_BLIP, sample_keys=keys.flip(0))
    assert torch.equal(rev["sequences"].flip(0), ref["sequences"]) and torch.equal(rev["lengths"].flip(0), ref["lengths"])
    eng.set_decode_path("small")
    small = eng.generate(px.cuda(), max_length=L_BLIP, sample_keys=keys)
    assert eng.last_decode_path == "small" and _same(small, ref)
    eng.set_decode_path("auto")
    state = eng.image_state(px.cuda())
    assert _same(eng.generate(state, max_length=L_BLIP, sample_keys=keys), ref)
    # the default keys: (call number << 32) | row, counted from set_sampling
    eng.set_sampling(True, 1.0, 0, 0.95, SEED)
    first = eng.generate(px.cuda(), max_length=L_BLIP)
    second = eng.generate(px.cuda(), max_length=L_BLIP)
    k0 = torch.arange(B, dtype=torch.int64)
    assert _same(first, eng.generate(px.cuda(), max_length=L_BLIP, sample_keys=k0))
    assert _same(second, eng.generate(px.cuda(), max_length=L_BLIP, sample_keys=k0 + (1 << 32)))
    assert not torch.equal(first["sequences"], second["sequences"])
    eng.set_sampling(True, 1.0, 0, 0.95, SEED)                                     # setting resets the counter
    assert _same(eng.generate(px.cuda(), max_length=L_BLIP), first)
    eng.close()


def test_compacted_loop_gives_the_uncompacted_bits():
    B = 20                                                                          # above the small-batch row limit
    # the fixture whose captions end early (seed 7), drawn close to the arg-max (a cold top-2) so that they still do: rows leave the
    # loop one by one while the others go on drawing
    arch, sd, px, eng = _sampled_blip_engine(B, (0.3, 2, 1.0), seed=7)
    keys = _keys(B, 100)
    eng.set_row_compaction(True)
    a = eng.generate(px.cuda(), max_length=L_BLIP, sample_keys=keys)
    assert eng.last_row_compaction
    eng.set_row_compaction(False)
    b = eng.generate(px.cuda(), max_length=L_BLIP, sample_keys=keys)
    assert not eng.last_row_compaction
    assert _same(a, b)
    assert len(set(a["lengths"].cpu().tolist())) > 1, "every caption ended at the same step: the compacted loop never dropped a row"
    eng.close()


def test_pool_merged_batches_give_the_single_calls_bits():
    from embodied_captioning_amd.engine import EnginePool
    B, nb = 2, 4
    arch, sd, px, eng = _sampled_blip_engine(nb * B)
    pool = EnginePool(arch, n=2, dtype="f32s", max_batch=2 * B, max_beams=1, max_len=L_BLIP, weights_of=eng)
    pool.set_sampling(True, 1.0, 0, 0.95, SEED)
    assert pool.do_sample
    batches = [px[j * B:(j + 1) * B].cuda() for j in range(nb)]
    outs = pool.generate_many(batches, coalesce_rows=2 * B, max_length=L_BLIP)      # the pool's calls 0 .. 3, merged two by two
    assert isinstance(pool.last_coalesce, list) and any(len(g) > 1 for g in pool.last_coalesce), pool.last_coalesce
    k0 = torch.arange(B, dtype=torch.int64)
    for j, (o, p) in enumerate(zip(outs, batches)):
        assert _same(o, eng.generate(p, max_length=L_BLIP, sample_keys=k0 + (j << 32)))
    unmerged = pool.generate_many(batches, max_length=L_BLIP)                        # calls 4 .. 7, each a pass of its own
    for j, (o, p) in enumerate(zip(unmerged, batches)):
        assert _same(o, eng.generate(p, max_length=L_BLIP, sample_keys=k0 + ((nb + j) << 32)))
    assert not _same(unmerged[0], outs[0])
    given = [_keys(B, 7 * j + 1) for j in range(nb)]
    outs = pool.generate_many(batches, coalesce_rows=2 * B, max_length=L_BLIP, sample_keys=given)
    for o, p, k in zip(outs, batches, given):
        assert _same(o, eng.generate(p, max_length=L_BLIP, sample_keys=k))
    pool.close()
    eng.close()


def test_different_keys_and_seeds_give_different_captions():
    B = 8
    arch, sd, px, eng = _sampled_blip_engine(B, (1.0, 0, 1.0))
    a = eng.generate(px.cuda(), max_length=L_BLIP, output_logits=True, sample_keys=_keys(B, 1))
    # the fixture is flat enough: at the first step no row gives its arg-max more than 0.9
    for b in range(B):
        ref = S.reference(a["logits"][0, b].cpu().numpy(), 1.0, 0, 1.0)
        assert (ref["w"] / ref["total"]).max() < 0.9, b
    b_ = eng.generate(px.cuda(), max_length=L_BLIP, sample_keys=_keys(B, 1000))
    assert int((a["sequences"] != b_["sequences"]).any(dim=1).sum()) >= B // 2
    eng.set_sampling(True, 1.0, 0, 1.0, SEED + 1)
    c = eng.generate(px.cuda(), max_length=L_BLIP, sample_keys=_keys(B, 1))
    assert int((a["sequences"] != c["sequences"]).any(dim=1).sum()) >= B // 2
    # one image, eight keys: eight rows of one state, mostly different captions
    state = eng.image_state(px[:1].cuda())
    d = eng.generate(state.repeat_interleave(8, dim=0), max_length=L_BLIP, sample_keys=_keys(8, 5))
    assert len({tuple(r) for r in d["sequences"].cpu().tolist()}) >= 4
    eng.close()


@pytest.mark.parametrize("family,dtype", [("blip", "f32s"), ("blip2", "bf16")])
def test_num_return_sequences(family, dtype):
    blip2 = family == "blip2"
    B, n = 2, 4
    arch, sd, px = (_blip2 if blip2 else _blip)(B)
    L = arch.max_new_tokens if blip2 else L_BLIP
    eng = _engine(arch, sd, dtype, B * n, L, **({} if blip2 else {"max_score_rows": L - 1}))
    eng.set_sampling(True, 1.0, 0, 0.95, SEED)
    out = eng.generate(px.cuda(), max_length=L, num_return_sequences=n)             # call 0: keys b * n + r
    assert tuple(out["sequences"].shape) == (B * n, L) and tuple(out["lengths"].shape) == (B * n,)
    state = eng.image_state(px.cuda())
    for b in range(B):
        for r in range(n):
            one = eng.generate(state[b:b + 1], max_length=L, sample_keys=torch.tensor([b * n + r], dtype=torch.int64))
            assert torch.equal(one["sequences"][0], out["sequences"][b * n + r]) and torch.equal(one["lengths"][0], out["lengths"][b * n + r])
    again = eng.generate(state, max_length=L, num_return_sequences=n)               # call 1: other keys
    assert not torch.equal(again["sequences"], out["sequences"])
    # the returned captions go to score() as candidates of their image
    seq, ln = out["sequences"].cpu().numpy(), out["lengths"].cpu().numpy()
    if blip2:
        ids = np.full((B * n, L + 1), arch.pad, dtype=np.int32)
        ids[:, 0] = arch.bos
        ids[:, 1:] = seq
        ln = ln + 1
    else:
        ids = seq
    sc = eng.score(state, ids[:, :int(ln.max())], ln, captions_per_image=n)
    assert tuple(sc["token_logprobs"].shape)[0] == B * n and torch.isfinite(sc["token_logprobs"]).all()
    assert (sc["scored"].cpu().numpy() == ln - 1).all()
    with pytest.raises(ValueError, match="num_return_sequences = 5.*max_batch"):
        eng.generate(px.cuda(), max_length=L, num_return_sequences=5)
    eng.set_sampling()
    with pytest.raises(ValueError, match="num_return_sequences"):
        eng.generate(px.cuda(), max_length=L, num_return_sequences=2)
    eng.close()


def test_set_then_reset_is_a_handle_that_never_sampled_and_scoring_ignores_the_state():
    B = 4
    arch, sd, px, eng = _sampled_blip_engine(B, (0.7, 50, 0.9))
    ids = np.full((B, 5), arch.pad, dtype=np.int32)
    ids[:, 0] = arch.bos
    ids[:, 1:5] = [20, 21, 22, 23]
    lens = np.full(B, 5, dtype=np.int32)
    scored = eng.score(px.cuda(), ids, lens)
    eng.generate(px.cuda(), max_length=L_BLIP)
    eng.set_sampling()
    assert eng.sampling == (False, 1.0, 0, 1.0, 0)
    fresh = _engine(arch, sd, "f32s", B, L_BLIP)
    a = eng.generate(px.cuda(), max_length=L_BLIP, output_logits=True, output_logprobs=True)
    b = fresh.generate(px.cuda(), max_length=L_BLIP, output_logits=True, output_logprobs=True)
    assert _same(a, b, ("sequences", "lengths", "logits", "token_logprobs", "scored_steps"))
    plain = fresh.score(px.cuda(), ids, lens)
    assert torch.equal(scored["token_logprobs"], plain["token_logprobs"]) and torch.equal(scored["top_ids"], plain["top_ids"])
    eng.close()
    fresh.close()


def test_refusals_by_message():
    from embodied_captioning_amd import _native as N
    B = 2
    arch, sd, px = _blip(B)
    eng = _engine(arch, sd, "f32s", B, L_BLIP, beams=2)
    with pytest.raises(ValueError, match="temperature"):                             # without sampling: judged as it always was
        eng.generate(px.cuda(), max_length=L_BLIP, temperature=0.5)
    with pytest.raises(ValueError, match="sample_keys"):
        eng.generate(px.cuda(), max_length=L_BLIP, sample_keys=_keys(B))
    eng.set_sampling(True, 0.7, 50, 0.9, 3)
    eng.generate(px.cuda(), max_length=L_BLIP, do_sample=True, temperature=0.7, top_k=50, top_p=0.9)
    for kw, word in (({"temperature": 0.5}, "temperature = 0.5"), ({"top_k": 10}, "top_k = 10"), ({"top_p": 0.5}, "top_p = 0.5"),
                     ({"do_sample": False}, "do_sample = False"), ({"temperature": 1.0}, "temperature = 1.0")):
        with pytest.raises(ValueError, match=word + ".*call set_sampling first"):
            eng.generate(px.cuda(), max_length=L_BLIP, **kw)
    with pytest.raises(N.CaptionerHipError, match="beam sampling is not built"):
        eng.generate(px.cuda(), max_length=L_BLIP, num_beams=2)
    with pytest.raises(N.CaptionerHipError, match="sampling is set on this handle.*beam groups"):
        eng.generate(px.cuda(), max_length=L_BLIP, num_beams=1, num_beam_groups=1)
    for kw in ({"output_logprobs": True}, {"output_vocab_maxprob": True}):
        with pytest.raises(N.CaptionerHipError, match="sampling is set on this handle.*out_logprobs"):
            eng.generate(px.cuda(), max_length=L_BLIP, **kw)
    with pytest.raises(ValueError, match="one key per caption"):
        eng.generate(px.cuda(), max_length=L_BLIP, sample_keys=_keys(B + 1))
    for bad, word in (((True, 0.0), "temperature must be"), ((True, float("nan")), "temperature must be"), ((True, 1.0, -1), "top_k must be"),
                      ((True, 1.0, 0, 0.0), "top_p must be"), ((True, 1.0, 0, 1.5), "top_p must be"), ((True, 1.0, 0, 1.0, -1), "seed must be")):
        with pytest.raises(ValueError, match=word):
            eng.set_sampling(*bad)
    assert eng.sampling == (True, float(np.float32(0.7)), 50, float(np.float32(0.9)), 3)    # a refused call changes nothing
    # the library's own checks (a caller of the C ABI has no host validation in front of it)
    lib = eng.lib
    for (T, k, p), word in (((0.0, 0, 1.0), "temperature = 0"), ((-1.0, 0, 1.0), "temperature = -1"), ((float("nan"), 0, 1.0), "temperature = nan"),
                            ((float("inf"), 0, 1.0), "temperature = inf"), ((1.0, -2, 1.0), "top_k = -2"), ((1.0, 0, 0.0), "top_p = 0"),
                            ((1.0, 0, 1.5), "top_p = 1.5"), ((1.0, 0, float("nan")), "top_p = nan")):
        rc = lib.cap_set_sampling(eng._h, 1, C.c_float(T), k, C.c_float(p), C.c_uint64(0))
        assert rc != 0 and word in lib.cap_last_error().decode(), (word, lib.cap_last_error().decode())
    assert lib.cap_set_sampling(None, 1, C.c_float(1.0), 0, C.c_float(1.0), C.c_uint64(0)) != 0 and "null handle" in lib.cap_last_error().decode()
    assert eng.sampling == (True, float(np.float32(0.7)), 50, float(np.float32(0.9)), 3)
    eng.close()


def test_a_coca_handle_refuses_sampling():
    """The host validation refuses sampling for CoCa, so only a caller of the C ABI can put it on a CoCa handle:
    cap_generate_request then refuses by name, and generates again once it is switched off."""
    from embodied_captioning_amd import _native as N
    from embodied_captioning_amd.config import CocaArch
    from embodied_captioning_amd.engine import CaptionerEngine
    from embodied_captioning_amd.weights import procedural_coca_state_dict, synthetic_pixels
    a = CocaArch.tiny()
    eng = CaptionerEngine(a, dtype="f32s", max_batch=2, max_beams=2, max_len=a.seq_len)
    eng.load_state_dict(procedural_coca_state_dict(a, 1, eos_boost=4.0))
    px = synthetic_pixels(2, a.image_size, seed=1).cuda()
    with pytest.raises(ValueError, match="CoCa"):
        eng.set_sampling(True, 0.7)
    with pytest.raises(ValueError, match="temperature"):
        eng.generate(px, max_length=a.seq_len, temperature=0.5)
    free = eng.generate(px, max_length=a.seq_len)
    assert eng.lib.cap_set_sampling(eng._h, 1, C.c_float(0.7), 0, C.c_float(1.0), C.c_uint64(0)) == 0 and eng.sampling[0]
    with pytest.raises(N.CaptionerHipError, match="sampling is set on this handle.*CoCa"):
        eng.generate(px, max_length=a.seq_len)
    assert eng.lib.cap_set_sampling(eng._h, 0, C.c_float(1.0), 0, C.c_float(1.0), C.c_uint64(0)) == 0
    assert _same(eng.generate(px, max_length=a.seq_len), free)
    eng.close()


def test_the_blip_wrapper_reads_the_keys_and_chunks_num_return_sequences_by_images():
    """captioner.do_sample / temperature / top_k / top_p / sample_seed / num_return_sequences through `BLIP(cfg)`: generate_batch returns
    n captions per image, image-major, from calls of batch_size // n images - the engine's calls 0, 1, ... with their default keys."""
    from embodied_captioning_amd.captioner.models.blip.blip import BLIP
    from embodied_captioning_amd.captioner.utils.utils import Configuration
    from embodied_captioning_amd.weights import synthetic_pixels
    n, N_IMG = 4, 3
    cfg = Configuration(arch_name="blip", model_name="procedural-tiny:5:1.0", max_length=L_BLIP, batch_size=8, do_sample=True,
                        temperature=0.9, top_k=40, top_p=0.95, sample_seed=77, num_return_sequences=n).captioner
    model = BLIP(cfg)
    eng = model.engine
    assert eng.sampling == (True, float(np.float32(0.9)), 40, float(np.float32(0.95)), 77)
    px = synthetic_pixels(N_IMG, model.arch.image_size, seed=5)
    out = model.generate_batch(px)
    assert tuple(out["sequences"].shape) == (N_IMG * n, L_BLIP) and len(out["texts"]) == N_IMG * n
    state = eng.image_state(px.cuda())
    want = []
    for call, (b0, nb) in enumerate(((0, 2), (2, 1))):                              # batch_size // n = 2 images per call
        keys = torch.arange(nb * n, dtype=torch.int64) + (call << 32)
        want.append(eng.generate(state[b0:b0 + nb].repeat_interleave(n, dim=0), max_length=L_BLIP, sample_keys=keys)["sequences"].cpu())
    assert torch.equal(out["sequences"], torch.cat(want))
    one = model.generate_batch(px, num_return_sequences=1)                          # the call's own count wins over the configured one
    assert tuple(one["sequences"].shape) == (N_IMG, L_BLIP)
    with pytest.raises(ValueError, match="exceeds batch_size"):
        model.generate_batch(px, num_return_sequences=9)
    eng.close()
    for kw, word in (({"temperature": 0.5}, "temperature=0.5"), ({"top_k": 5}, "top_k=5"), ({"num_return_sequences": 2}, "needs captioner.do_sample"),
                     ({"do_sample": True, "num_beams": 3}, "beam sampling is not built")):
        with pytest.raises(ValueError, match=word):
            BLIP(Configuration(arch_name="blip", model_name="procedural-tiny:5:1.0", max_length=L_BLIP, batch_size=8, **kw).captioner)
