"""GPU: repetition_penalty / no_repeat_ngram_size end to end (`CaptionerEngine.set_repeat_controls`, cap_set_repeat_controls) on the
fixture-size BLIP and BLIP-2 models.

* REPLAY: a call under the controls returns its own raw step logits; every emitted token must be the restatement's choice
  (tests/_repeat_ref.py) on that row of logits and the caption's context as HF's processors see it - BLIP: BOS, the prompt, the
  generated tokens; BLIP-2: the image placeholders, BOS, the generated tokens.  Exact, in every arithmetic mode: both sides read the
  same fp32 rows and penalise them with the same fp32 multiplication / division.
* INVARIANCES, all bit for bit: a row alone = in its batch, small-batch path = batch path, compacted = uncompacted loop, pixels =
  image state, a pool call with two merged batches = the two calls alone, set -> reset = a handle that never had the controls.
* beam search under an n-gram size repeats no n-gram; controls together with a ban set; scoring ignores the controls; the refusals,
  by message.
* HF GOLDENS (tools/make_goldens_repeat_controls.py: the real HF models' `generate(repetition_penalty=, no_repeat_ngram_size=)` on
  the CPU): greedy under the penalty, under an n-gram size, under both plus a ban, 3 beams under both, BLIP prompted with an n-gram
  that starts in the prompt - tokens and lengths identical, beam scores within 2e-3, on every row whose per-step margins in HF's run
  are all at least the logit bar 1e-3; the generator asserts that at most 1 row in 8 is below it and that every case changes at
  least 2 rows in 8."""
import ctypes as C
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

from _repeat_ref import blip2_context, greedy_choice, has_repeated_ngram, ngram_banned_mask

pytestmark = pytest.mark.gpu

L_BLIP = 16           # with seed 5 the captions are long enough to repeat themselves: the controls have work at this length
SETTINGS = [(1.5, 0), (1.0, 1), (1.0, 2), (1.5, 3), (0.7, 2)]          # (penalty, n-gram size); 0.7 rewards repetition: n-grams get work


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


def _generated(seq, lens, b, blip2):
    """The generated tokens of row b (EOS included, pad not)."""
    n = int(lens[b])
    return [int(t) for t in (seq[b, :n] if blip2 else seq[b, 1:n])]


def _same(a, b, keys=("sequences", "lengths")):
    return all(torch.equal(a[k], b[k]) for k in keys)


def _same_open_logits(a, b):
    """The step logits of two calls, bit for bit, at the steps at which the caption was still open (a finished row's logits are
    whatever the path leaves there: the batch path's head runs over the open rows only)."""
    lens = a["lengths"].cpu().tolist()
    return all(torch.equal(a["logits"][:n - 1, r], b["logits"][:n - 1, r]) for r, n in enumerate(lens))


def _replay(arch, out, p, n, blip2, prompt=None, seqs=()):
    """Every emitted token of every row = the restatement's choice on that step's raw logits and HF's context of the row.  -> steps
    replayed, steps at which that choice is not the raw row's arg-max."""
    seq, lens, logits = out["sequences"].cpu().numpy(), out["lengths"].cpu().numpy(), out["logits"].cpu().numpy()
    steps = bites = 0
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
            want = greedy_choice(logits[j, b], ctx, p, n, seqs, eos=arch.eos, ban_context=ban_ctx)
            assert tok == want, (b, j, tok, want, ctx)
            bites += int(want != int(np.argmax(logits[j, b])))
            done = done + [tok]
            steps += 1
        if n > 0:
            whole = done if not blip2 else [arch.bos] + done
            assert not has_repeated_ngram(whole, n), (b, n, whole)
    return steps, bites


@pytest.mark.parametrize("family,dtype", [("blip", "f32s"), ("blip", "bf16"), ("blip2", "bf16")])
def test_replay_every_token_is_the_restatements_choice(family, dtype):
    blip2 = family == "blip2"
    B = 8
    arch, sd, px = (_blip2 if blip2 else _blip)(B)
    L = arch.max_new_tokens if blip2 else L_BLIP
    eng = _engine(arch, sd, dtype, B, L)
    assert (eng.repetition_penalty, eng.no_repeat_ngram_size) == (1.0, 0) == eng.repeat_controls
    free = eng.generate(px.cuda(), max_length=L, output_logits=True)
    assert _replay(arch, free, 1.0, 0, blip2) == (int(free["lengths"].sum()) - (0 if blip2 else B), 0)      # plain arg-max of its logits
    total = 0
    for p, n in SETTINGS:
        eng.set_repeat_controls(p, n)
        assert eng.repeat_controls == (float(np.float32(p)), n) == (eng.repetition_penalty, eng.no_repeat_ngram_size)
        out = eng.generate(px.cuda(), max_length=L, output_logits=True, repetition_penalty=p, no_repeat_ngram_size=n)
        steps, bites = _replay(arch, out, p, n, blip2)
        total += bites
        if not blip2:
            # BLIP's step 0 sees BOS alone, which the model does not emit: its raw logits are the unconstrained call's, bit for bit
            assert torch.equal(out["logits"][0], free["logits"][0])
        if blip2 and p != 1.0:
            # HF's BLIP-2 context holds the placeholders and BOS: both scores are penalised at the first step already
            x0 = out["logits"][0, 0].cpu().numpy()
            assert torch.equal(out["logits"][0], free["logits"][0])
            from _repeat_ref import processed_row
            y0 = processed_row(x0, blip2_context([], arch.num_query_tokens, arch.image_token, arch.bos), p)
            assert y0[arch.bos] != x0[arch.bos] and y0[arch.image_token] != x0[arch.image_token]
        print(f"\n{family} {dtype} p={p} n={n}: {steps} emitted tokens replayed, the controls changed the choice at {bites} steps, "
              f"{int((out['sequences'] != free['sequences']).any(dim=1).sum())} of {B} captions changed")
    assert total > 0, "no setting changed any choice: the fixture gives the controls nothing to do"
    eng.close()


def test_blip2_with_bos_equal_to_eos_penalises_eos_from_the_first_step():
    """OPT's own BOS and EOS are one id (2).  The tiny architecture with eos = bos: under a penalty the EOS score is penalised at
    every step, as in HF's run, and every token is still the restatement's choice."""
    B = 8
    arch, sd, px = _blip2(B, eos=2)
    assert arch.eos == arch.bos == 2
    L = arch.max_new_tokens
    eng = _engine(arch, sd, "bf16", B, L)
    free = eng.generate(px.cuda(), max_length=L, output_logits=True)
    _replay(arch, free, 1.0, 0, True)
    eng.set_repeat_controls(1.5, 2)
    out = eng.generate(px.cuda(), max_length=L, output_logits=True)
    steps, bites = _replay(arch, out, 1.5, 2, True)
    print(f"\nblip2 eos = bos: {steps} tokens replayed, {bites} choices changed; lengths {free['lengths'].tolist()} -> {out['lengths'].tolist()}")
    eng.close()


@pytest.mark.parametrize("path", ["batch", "small", "compacted"])
def test_prompted_replay_the_context_reaches_across_the_prompt_boundary(path):
    """Prompted generate with the prompt [bos, x, y, x], y = the token most images emit first behind [bos, x]: with n = 2 the
    bigram `x y` of the PROMPT bans y as the first generated token, and the penalty reaches x and y, only because the context holds
    the prompt.  The loop starts at t = P - 1 and the step outputs are indexed from there."""
    B = 20 if path == "compacted" else 8
    arch, sd, px = _blip(B)
    x = 31
    eng = _engine(arch, sd, "f32s", B, L_BLIP, max_prompt=4)
    eng.set_decode_path("batch" if path == "compacted" else path)
    first = eng.generate(px.cuda(), max_length=L_BLIP, prompt_ids=[arch.bos, x])["sequences"][:, 2].cpu().tolist()
    y = max(set(first), key=first.count)
    assert y not in (arch.eos, arch.pad, arch.bos, x)
    prompt = [arch.bos, x, y, x]
    free = eng.generate(px.cuda(), max_length=L_BLIP, prompt_ids=prompt, output_logits=True)
    assert _replay(arch, free, 1.0, 0, False, prompt)[1] == 0
    assert ngram_banned_mask(prompt, arch.vocab, 2)[y]
    for p, n in ((1.0, 2), (1.3, 2), (1.5, 0)):
        eng.set_repeat_controls(p, n)
        out = eng.generate(px.cuda(), max_length=L_BLIP, prompt_ids=prompt, output_logits=True)
        steps, bites = _replay(arch, out, p, n, False, prompt)
        got = out["sequences"][:, len(prompt)].cpu().tolist()
        assert torch.equal(out["logits"][0], free["logits"][0])
        assert torch.equal(out["sequences"][:, :len(prompt)].cpu(), torch.tensor([prompt] * B, dtype=torch.int32))
        if n == 2:
            assert all(g != y for g in got)
        if path == "compacted":          # the same call without per-step logits runs compacted, to the same tokens
            eng.set_row_compaction(True)
            c = eng.generate(px.cuda(), max_length=L_BLIP, prompt_ids=prompt)
            assert eng.last_row_compaction and _same(c, out)
            eng.set_row_compaction(False)
        else:
            assert eng.last_decode_path == path
        print(f"\nprompted {path} p={p} n={n}: {steps} generated tokens replayed, {bites} choices changed, y = {y}, first tokens {got}")
    eng.close()


def _controlled_blip_engine(B, p=1.5, n=2, dtype="f32s", **kw):
    arch, sd, px = _blip(B)
    eng = _engine(arch, sd, dtype, B, L_BLIP, **kw)
    free = eng.generate(px.cuda(), max_length=L_BLIP)
    eng.set_repeat_controls(p, n)
    return arch, sd, px, eng, free


def test_row_alone_small_path_and_image_state_give_the_batch_bits():
    B = 6
    arch, sd, px, eng, free = _controlled_blip_engine(B)
    eng.set_decode_path("batch")
    ref = eng.generate(px.cuda(), max_length=L_BLIP, output_logits=True)
    assert eng.last_decode_path == "batch"
    _replay(arch, ref, 1.5, 2, False)
    for b in (0, 3):
        one = eng.generate(px[b:b + 1].cuda(), max_length=L_BLIP, output_logits=True)
        assert torch.equal(one["sequences"][0], ref["sequences"][b]) and torch.equal(one["lengths"][0], ref["lengths"][b])
        assert torch.equal(one["logits"][:, 0], ref["logits"][:, b])
    eng.set_decode_path("small")
    small = eng.generate(px.cuda(), max_length=L_BLIP, output_logits=True)
    assert eng.last_decode_path == "small" and _same(small, ref) and _same_open_logits(small, ref)
    eng.set_decode_path("auto")
    state = eng.image_state(px.cuda())
    assert _same(eng.generate(state, max_length=L_BLIP), ref)
    eng.close()
    # beams: no repeated n-gram in the best hypotheses (BOS included), with and without the penalty, and from an image state
    eng = _engine(arch, sd, "f32s", B, L_BLIP, beams=3)
    for p, n in ((1.0, 2), (0.7, 2), (1.5, 1), (0.7, 3)):
        eng.set_repeat_controls(p, n)
        ob = eng.generate(px.cuda(), num_beams=3, max_length=L_BLIP)
        s, ln = ob["sequences"].cpu().numpy(), ob["lengths"].cpu().numpy()
        for b in range(B):
            assert not has_repeated_ngram([arch.bos] + _generated(s, ln, b, False), n), (p, n, b, s[b])
        assert _same(eng.generate(eng.image_state(px.cuda()), num_beams=3, max_length=L_BLIP), ob, ("sequences", "lengths", "sequences_scores"))
    eng.close()


def test_compacted_loop_gives_the_uncompacted_bits():
    B = 20                                                                          # above the small-batch row limit
    # the fixture whose captions end early (seed 7), with every first token but the most frequent one banned: those captions keep
    # their early EOS and leave the loop one by one, while the others go on under the controls and the ban
    arch, sd, px = _blip(B, seed=7)
    eng = _engine(arch, sd, "f32s", B, L_BLIP)
    first = eng.generate(px.cuda(), max_length=L_BLIP)["sequences"][:, 1].cpu().tolist()
    special = {arch.bos, arch.pad, arch.eos}
    eng.set_bad_words([[t] for t in sorted(set(first) - special - {max(set(first), key=first.count)})])
    eng.set_repeat_controls(1.5, 2)
    eng.set_row_compaction(True)
    a = eng.generate(px.cuda(), max_length=L_BLIP)
    assert eng.last_row_compaction
    eng.set_row_compaction(False)
    b = eng.generate(px.cuda(), max_length=L_BLIP)
    assert not eng.last_row_compaction
    assert _same(a, b)
    n = a["lengths"].cpu().numpy()
    assert len(set(n.tolist())) > 1, "every caption ended at the same step: the compacted loop never dropped a row"
    eng.close()


def test_pool_merged_batches_give_the_single_calls_bits():
    from embodied_captioning_amd.engine import EnginePool
    B = 4
    arch, sd, px, eng, free = _controlled_blip_engine(2 * B, 1.5, 2)
    pool = EnginePool(arch, n=2, dtype="f32s", max_batch=2 * B, max_beams=1, max_len=L_BLIP, weights_of=eng)
    pool.set_repeat_controls(1.5, 2)
    assert (pool.repetition_penalty, pool.no_repeat_ngram_size) == (1.5, 2)
    batches = [px[:B].cuda(), px[B:].cuda()]
    outs = pool.generate_many(batches, coalesce_rows=2 * B, max_length=L_BLIP)
    assert pool.last_coalesce is not None
    for o, p in zip(outs, batches):
        assert _same(o, eng.generate(p, max_length=L_BLIP))
    pool.close()
    eng.close()


def test_set_then_reset_is_a_handle_that_never_had_the_controls_and_scoring_ignores_them():
    B = 4
    arch, sd, px, eng, _ = _controlled_blip_engine(B, 1.5, 2)
    ids = np.full((B, 5), arch.pad, dtype=np.int32)
    ids[:, 0] = arch.bos
    ids[:, 1:5] = [20, 21, 20, 21]                                                  # a repeated bigram among the GIVEN tokens
    lens = np.full(B, 5, dtype=np.int32)
    scored = eng.score(px.cuda(), ids, lens)
    eng.set_repeat_controls()
    assert eng.repeat_controls == (1.0, 0)
    fresh = _engine(arch, sd, "f32s", B, L_BLIP)
    a = eng.generate(px.cuda(), max_length=L_BLIP, output_logits=True, output_logprobs=True)
    b = fresh.generate(px.cuda(), max_length=L_BLIP, output_logits=True, output_logprobs=True)
    assert _same(a, b, ("sequences", "lengths", "logits", "token_logprobs", "scored_steps"))
    plain = fresh.score(px.cuda(), ids, lens)
    assert torch.equal(scored["token_logprobs"], plain["token_logprobs"]) and torch.equal(scored["top_ids"], plain["top_ids"])
    eng.close()
    fresh.close()


def test_controls_together_with_a_ban_set():
    """HF's order: penalty, n-grams, bad words.  The ban set holds every row's first token under the controls alone and a 2-token
    sequence from those captions; every token is the restatement's choice under all three, and the ban's own context is unchanged."""
    B = 8
    for blip2 in (False, True):
        arch, sd, px = (_blip2 if blip2 else _blip)(B)
        L = arch.max_new_tokens if blip2 else L_BLIP
        eng = _engine(arch, sd, "bf16" if blip2 else "f32s", B, L)
        eng.set_repeat_controls(1.5, 2)
        mid = eng.generate(px.cuda(), max_length=L)
        s, ln = mid["sequences"].cpu().numpy(), mid["lengths"].cpu().numpy()
        gens = [_generated(s, ln, b, blip2) for b in range(B)]
        special = {arch.bos, arch.pad, arch.eos} | ({arch.image_token} if blip2 else set())
        seqs = [[t] for t in sorted({g[0] for g in gens if g[0] not in special})]
        pair = next(([g[j], g[j + 1]] for g in sorted(gens, key=len, reverse=True) for j in range(1, len(g) - 1)
                     if not ({g[j], g[j + 1]} & (special | {q[0] for q in seqs}))), None)
        assert seqs and pair, gens
        seqs.append(pair)
        eng.set_bad_words(seqs)
        out = eng.generate(px.cuda(), max_length=L, output_logits=True, bad_words_ids=seqs, repetition_penalty=1.5, no_repeat_ngram_size=2)
        steps, bites = _replay(arch, out, 1.5, 2, blip2, seqs=seqs)
        banned_first = {q[0] for q in seqs if len(q) == 1}
        for b in range(B):                                                          # a row whose first token is banned has changed
            assert gens[b][0] not in banned_first or not torch.equal(out["sequences"][b], mid["sequences"][b]), b
        eng.set_repeat_controls()                                                   # the ban stays when the controls go
        only_ban = eng.generate(px.cuda(), max_length=L, output_logits=True)
        _replay(arch, only_ban, 1.0, 0, blip2, seqs=seqs)
        eng.close()


def test_blip2_beams_and_image_state_under_the_controls():
    B = 3
    arch, sd, px = _blip2(B)
    L = arch.max_new_tokens
    eng = _engine(arch, sd, "bf16", B, L, beams=3)
    free = eng.generate(px.cuda(), max_length=L)
    for p, n in ((1.5, 2), (0.7, 2)):
        eng.set_repeat_controls(p, n)
        g = eng.generate(px.cuda(), max_length=L)
        ob = eng.generate(px.cuda(), num_beams=3, max_length=L)
        for o in (g, ob):
            s, ln = o["sequences"].cpu().numpy(), o["lengths"].cpu().numpy()
            assert all(not has_repeated_ngram([arch.bos] + _generated(s, ln, b, True), n) for b in range(B))
        state = eng.image_state(px.cuda())
        assert _same(eng.generate(state, max_length=L), g)
        assert _same(eng.generate(state, num_beams=3, max_length=L), ob, ("sequences", "lengths", "sequences_scores"))
        one = eng.generate(px[1:2].cuda(), max_length=L)
        assert torch.equal(one["sequences"][0], g["sequences"][1])
    with pytest.raises(ValueError, match="no_repeat_ngram_size = .* is beyond"):
        eng.set_repeat_controls(1.0, L + arch.num_query_tokens + 2)
    assert eng.repeat_controls == (float(np.float32(0.7)), 2)                       # a refused call leaves the controls in force
    eng.close()


def test_refusals_by_message():
    from embodied_captioning_amd import _native as N
    B = 2
    arch, sd, px, eng, _ = _controlled_blip_engine(B, 1.5, 2)
    for kw in ({"repetition_penalty": 1.3}, {"no_repeat_ngram_size": 3}, {"repetition_penalty": 1.0}, {"no_repeat_ngram_size": 0}):
        with pytest.raises(ValueError, match="call set_repeat_controls first"):
            eng.generate(px.cuda(), max_length=L_BLIP, **kw)
    eng.generate(px.cuda(), max_length=L_BLIP, repetition_penalty=1.5, no_repeat_ngram_size=2)
    for kw in ({"output_logprobs": True}, {"output_vocab_maxprob": True}):
        with pytest.raises(N.CaptionerHipError, match="repetition controls are set on this handle"):
            eng.generate(px.cuda(), max_length=L_BLIP, **kw)
    with pytest.raises(ValueError, match="temperature"):
        eng.generate(px.cuda(), max_length=L_BLIP, temperature=0.5)
    with pytest.raises(N.CaptionerHipError, match="repetition controls are set on this handle.*beam groups do not take them"):
        eng.generate(px.cuda(), max_length=L_BLIP, num_beams=1, num_beam_groups=1)
    for bad, word in (((0.0, 0), "repetition_penalty must be"), ((1.0, -1), "no_repeat_ngram_size must be"), ((1.0, L_BLIP + 1), "is beyond")):
        with pytest.raises(ValueError, match=word):
            eng.set_repeat_controls(*bad)
    # the library's own checks (a caller of the C ABI has no host validation in front of it)
    lib = eng.lib
    for (p, n), word in (((0.0, 0), "repetition_penalty = 0"), ((-1.0, 0), "repetition_penalty = -1"), ((float("nan"), 0), "repetition_penalty = nan"),
                         ((float("inf"), 0), "repetition_penalty = inf"), ((1.0, -2), "no_repeat_ngram_size = -2"),
                         ((1.0, L_BLIP + 1), f"no_repeat_ngram_size = {L_BLIP + 1} is beyond")):
        assert lib.cap_set_repeat_controls(eng._h, C.c_float(p), n) != 0 and word in lib.cap_last_error().decode(), (word, lib.cap_last_error().decode())
    assert lib.cap_set_repeat_controls(None, C.c_float(1.5), 0) != 0 and "null handle" in lib.cap_last_error().decode()
    assert eng.repeat_controls == (1.5, 2)                                           # a refused call changes nothing
    eng.close()
    # a BLIP-2 handle needs its placeholder id before a control goes on
    arch2, sd2, px2 = _blip2(1)
    e2 = _engine(arch2, sd2, "bf16", 1, arch2.max_new_tokens)
    assert lib.cap_set_repeat_controls(e2._h, C.c_float(1.5), 0) != 0 and "cap_set_image_token" in lib.cap_last_error().decode()
    assert lib.cap_set_repeat_controls(e2._h, C.c_float(1.0), 0) == 0
    assert lib.cap_set_image_token(e2._h, -1) != 0 and lib.cap_set_image_token(e2._h, arch2.image_token) == 0
    assert lib.cap_set_repeat_controls(e2._h, C.c_float(1.5), 0) == 0
    e2.close()


def test_a_coca_handle_with_the_controls_refuses_to_generate():
    """The host validation refuses the controls for CoCa, so only a caller of the C ABI can put them on a CoCa handle:
    cap_generate_request then refuses by name - greedy, beams and beam groups - and generates again once they are reset."""
    from embodied_captioning_amd import _native as N
    from embodied_captioning_amd.config import CocaArch
    from embodied_captioning_amd.engine import CaptionerEngine
    from embodied_captioning_amd.weights import procedural_coca_state_dict, synthetic_pixels
    a = CocaArch.tiny()
    eng = CaptionerEngine(a, dtype="f32s", max_batch=2, max_beams=2, max_len=a.seq_len)
    eng.load_state_dict(procedural_coca_state_dict(a, 1, eos_boost=4.0))
    px = synthetic_pixels(2, a.image_size, seed=1).cuda()
    for kw in ((1.5, 0), (1.0, 2)):
        with pytest.raises(ValueError, match="CoCa"):
            eng.set_repeat_controls(*kw)
    with pytest.raises(ValueError, match="CoCa"):
        eng.generate(px, max_length=a.seq_len, repetition_penalty=1.3)
    free = eng.generate(px, max_length=a.seq_len, repetition_penalty=1.0, no_repeat_ngram_size=0)
    assert eng.lib.cap_set_repeat_controls(eng._h, C.c_float(1.5), 2) == 0 and eng.repeat_controls == (1.5, 2)
    for kw in ({}, {"num_beams": 2}, {"num_beams": 2, "num_beam_groups": 2}):
        with pytest.raises(N.CaptionerHipError, match="repetition controls are set on this handle.*CoCa captioner"):
            eng.generate(px, max_length=a.seq_len, **kw)
    assert eng.lib.cap_set_repeat_controls(eng._h, C.c_float(1.0), 0) == 0
    assert _same(eng.generate(px, max_length=a.seq_len), free)
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ HF goldens
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCORE_BAR = 2e-3          # tests/test_configs_gpu.py (BLIP beam 3), tests/test_blip2_beam_gpu.py, tests/test_bad_words_generate_gpu.py


def _golden_rows(g, meta, key, lens):
    """Rows whose every step margin in HF's run reaches the bar (the generator asserted: all but 1 in 8 at the most, and that the
    case changes at least 2 rows in 8 against HF's unconstrained run); their lengths must be HF's."""
    assert meta["rows_changed"][key] >= 2 and meta["rows_below_bar"][key] * 8 <= meta["batch"]
    ok = np.nonzero(g[f"{key}_margin"].min(axis=0) >= meta["bar"])[0]
    assert len(ok) * 8 >= 7 * len(lens), (key, "more than 1 row in 8 below the bar", g[f"{key}_margin"].min(axis=0))
    for b in ok:
        assert int(lens[b]) == int(g[f"{key}_lengths"][b]), (key, b, int(lens[b]), int(g[f"{key}_lengths"][b]))
    return ok


def _golden_cases(meta, ban):
    p, n = meta["penalty"], meta["ngram"]
    return (("penalty", (p, 0), [], {}), ("ngram", (1.0, n), [], {}), ("all", (p, n), ban, {}), ("beams3", (p, n), [], {"num_beams": 3}))


@pytest.mark.parametrize("dtype", ["f32", "f32s"])
def test_blip_tiny_matches_hf_under_the_controls(dtype):
    from embodied_captioning_amd.config import BlipArch
    from embodied_captioning_amd.weights import procedural_blip_state_dict, synthetic_pixels
    g = np.load(os.path.join(GOLDEN, "blip_tiny_repeat_controls.npz"))
    meta = json.loads(str(g["meta"]))
    arch, B, L = BlipArch(**meta["arch"]), meta["batch"], meta["max_length"]
    sd = procedural_blip_state_dict(arch, meta["seed"], eos_boost=meta["eos_boost"])
    px = synthetic_pixels(B, arch.image_size, seed=meta["seed"]).cuda()
    prompt = g["prompt_ids"].tolist()
    assert prompt[1] == prompt[3] and len(prompt) == 4                          # [bos, x, y, x]: the n-gram starts in the prompt
    eng = _engine(arch, sd, dtype, B, L, beams=3, max_prompt=len(prompt))
    cases = _golden_cases(meta, json.loads(str(g["ban"]))) + (("prompted", (meta["penalty"], meta["ngram_prompted"]), [], {"prompt_ids": prompt}),)
    for key, ctl, ban, kw in cases:
        eng.set_repeat_controls(*ctl)
        eng.set_bad_words(ban)
        first = len(prompt) if key == "prompted" else 1
        out = eng.generate(px, max_length=L, **kw)
        seq, lens = out["sequences"].cpu().numpy(), out["lengths"].cpu().numpy()
        ok = _golden_rows(g, meta, key, lens)
        for b in ok:
            n = int(lens[b]) - first
            assert np.array_equal(seq[b, first:first + n], g[f"{key}_ids"][b, :n]), (key, b, seq[b], g[f"{key}_ids"][b])
        if key == "beams3":
            err = np.abs(out["sequences_scores"].cpu().numpy() - g["beams3_scores"])[ok]
            print(f"\nblip {dtype} beams3 under the controls: score error {err.max():.3e} over rows {ok.tolist()}")
            assert err.max() < SCORE_BAR
        if key == "prompted":
            assert np.array_equal(seq[:, :first], np.tile(prompt, (B, 1))) and (seq[:, first] != prompt[2]).all()
    eng.close()


@pytest.mark.parametrize("dtype", ["f32", "f32s"])
def test_blip2_tiny_matches_hf_under_the_controls(dtype):
    from embodied_captioning_amd.config import Blip2Arch
    from embodied_captioning_amd.weights import procedural_blip2_state_dict, synthetic_pixels
    g = np.load(os.path.join(GOLDEN, "blip2_tiny_repeat_controls.npz"))
    meta = json.loads(str(g["meta"]))
    arch, B = Blip2Arch(**meta["arch"]), meta["batch"]
    n_new = arch.max_new_tokens
    sd = procedural_blip2_state_dict(arch, meta["seed"], eos_boost=meta["eos_boost"])
    px = synthetic_pixels(B, arch.image_size, seed=meta["seed"]).cuda()
    eng = _engine(arch, sd, dtype, B, n_new, beams=3)
    for key, ctl, ban, kw in _golden_cases(meta, json.loads(str(g["ban"]))):
        eng.set_repeat_controls(*ctl)
        eng.set_bad_words(ban)
        out = eng.generate(px, max_length=n_new, **kw)
        seq, lens = out["sequences"].cpu().numpy(), out["lengths"].cpu().numpy()
        ok = _golden_rows(g, meta, key, lens)
        for b in ok:
            assert np.array_equal(seq[b, :int(lens[b])], g[f"{key}_ids"][b, :int(lens[b])]), (key, b, seq[b], g[f"{key}_ids"][b])
        if key == "beams3":
            err = np.abs(out["sequences_scores"].cpu().numpy() - g["beams3_scores"])[ok]
            print(f"\nblip2 {dtype} beams3 under the controls: score error {err.max():.3e} over rows {ok.tolist()}")
            assert err.max() < SCORE_BAR
    eng.close()
