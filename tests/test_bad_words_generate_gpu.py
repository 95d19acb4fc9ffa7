"""GPU: bad_words_ids end to end (`CaptionerEngine.set_bad_words`, cap_set_bad_words) on the fixture-size BLIP and BLIP-2 models.

* REPLAY: a call with a set that bans every row's unconstrained first token and one 2-token sequence of the unconstrained captions
  returns its own raw step logits; every emitted token must be the restatement's choice (tests/_bad_words_ref.py) on that row of
  logits and the caption's context as HF's processor sees it.  Exact, in every arithmetic mode: both sides read the same fp32 rows.
* INVARIANCES, all bit for bit: a row alone = in its batch, small-batch path = batch path, compacted = uncompacted loop, pixels =
  image state, a pool call with two merged batches = the two calls alone, set -> clear = a handle that never had a set.
* HF GOLDENS (tools/make_goldens_bad_words.py: the real HF models' `generate(bad_words_ids=...)` on the CPU): greedy, greedy behind a
  prompt whose last token starts a banned sequence, 3 beams - tokens and lengths identical, beam scores within 2e-3 (the bar of the
  existing BLIP / BLIP-2 beam goldens), on every row whose per-step margins in HF's run are all at least the logit bar 1e-3; the
  generator asserts that at most 1 row in 8 is below it.
* beam search under the set emits no banned token or sequence; scoring ignores the set; the refusals, by message."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from _bad_words_ref import greedy_choice

pytestmark = pytest.mark.gpu

L_BLIP = 12


def _blip(batch, seed=7):
    from embodied_captioning_amd.config import BlipArch
    from embodied_captioning_amd.weights import procedural_blip_state_dict, synthetic_pixels
    arch = BlipArch.tiny()
    return arch, _sd("blip", lambda: procedural_blip_state_dict(arch, seed, eos_boost=1.0)), synthetic_pixels(batch, arch.image_size, seed=seed)


def _blip2(batch, seed=5):
    from embodied_captioning_amd.config import Blip2Arch
    from embodied_captioning_amd.weights import procedural_blip2_state_dict, synthetic_pixels
    arch = Blip2Arch.tiny()
    return arch, _sd("blip2", lambda: procedural_blip2_state_dict(arch, seed, eos_boost=0.3)), synthetic_pixels(batch, arch.image_size, seed=seed)


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


def _pair(gens, special, singles):
    """A 2-token sequence from inside the longest of the captions that holds one without a special or singly banned token."""
    for g in sorted(gens, key=len, reverse=True):
        for j in range(1, len(g) - 1):
            if not ({g[j], g[j + 1]} & (special | set(singles))):
                return [g[j], g[j + 1]]
    return None


_SETS = {}


def _ban_set(family, dtype):
    """The set of a family's tests, from 8 rows, computed once: every row's unconstrained first token; one 2-token sequence taken
    from the unconstrained captions; and one taken from the captions decoded with the single tokens banned - so a sequence is sure
    to be met on the way, not only on a path the single tokens already closed.  -> (set, captions under the single tokens alone)."""
    if (family, dtype) not in _SETS:
        blip2 = family == "blip2"
        arch, sd, px = (_blip2 if blip2 else _blip)(8)
        L = arch.max_new_tokens if blip2 else L_BLIP
        eng = _engine(arch, sd, dtype, 8, L)
        free = eng.generate(px.cuda(), max_length=L)
        seq, lens = free["sequences"].cpu().numpy(), free["lengths"].cpu().numpy()
        gens = [_generated(seq, lens, b, blip2) for b in range(8)]
        special = {arch.bos, arch.pad, arch.eos}
        singles = sorted({g[0] for g in gens if g and g[0] not in special})
        eng.set_bad_words([[t] for t in singles])
        mid = eng.generate(px.cuda(), max_length=L)
        seq, lens = mid["sequences"].cpu().numpy(), mid["lengths"].cpu().numpy()
        gens1 = [_generated(seq, lens, b, blip2) for b in range(8)]
        eng.close()
        pairs = [_pair(gens, special, singles), _pair(gens1, special, singles)]
        assert singles and all(pairs), (gens, gens1, "the captions are too short to take a ban from")
        _SETS[family, dtype] = ([[t] for t in singles] + [p for i, p in enumerate(pairs) if p not in pairs[:i]], gens1)
    return _SETS[family, dtype]


def _contains_ban(gen, seqs):
    return any(gen[i:i + len(s)] == list(s) for s in seqs for i in range(len(gen) - len(s) + 1))


def _replay(arch, out, seqs, blip2, prompt=None):
    """Every emitted token of every row = the restatement's choice on that step's raw logits and the row's context (BOS, the prompt
    where there is one, the tokens generated so far)."""
    seq, lens, logits = out["sequences"].cpu().numpy(), out["lengths"].cpu().numpy(), out["logits"].cpu().numpy()
    steps = 0
    for b in range(seq.shape[0]):
        gen = _generated(seq, lens, b, blip2)
        ctx = [arch.bos]
        if prompt is not None:
            assert gen[:len(prompt) - 1] == list(prompt[1:])
            ctx, gen = list(prompt), gen[len(prompt) - 1:]
        for j, tok in enumerate(gen):
            want = greedy_choice(logits[j, b], ctx, seqs, eos=arch.eos)
            assert tok == want, (b, j, tok, want, ctx)
            ctx.append(tok)
            steps += 1
        assert not _contains_ban(gen, seqs), (b, gen)
    return steps


@pytest.mark.parametrize("family,dtype", [("blip", "f32s"), ("blip", "bf16"), ("blip2", "bf16")])
def test_replay_every_token_is_the_restatements_choice(family, dtype):
    blip2 = family == "blip2"
    B = 8
    arch, sd, px = (_blip2 if blip2 else _blip)(B)
    L = arch.max_new_tokens if blip2 else L_BLIP
    seqs, under_singles = _ban_set(family, dtype)
    eng = _engine(arch, sd, dtype, B, L)
    free = eng.generate(px.cuda(), max_length=L, output_logits=True)
    fseq, flens = free["sequences"].cpu().numpy(), free["lengths"].cpu().numpy()
    assert _replay(arch, free, [], blip2) > B                                    # the unconstrained call is plain arg-max of its logits
    eng.set_bad_words(seqs)
    n_multi = sum(len(q) > 1 for q in seqs)
    assert eng.bad_words == seqs and eng.bad_words_counts == (len(seqs) - n_multi, n_multi)
    out = eng.generate(px.cuda(), max_length=L, output_logits=True, bad_words_ids=seqs)
    steps = _replay(arch, out, seqs, blip2)
    seq, lens = out["sequences"].cpu().numpy(), out["lengths"].cpu().numpy()
    changed = 0
    for b in range(B):
        if _contains_ban(_generated(fseq, flens, b, blip2), seqs):
            assert _generated(seq, lens, b, blip2) != _generated(fseq, flens, b, blip2), b
            changed += 1
    assert changed == B                                                             # every row's first token was banned
    # and a 2-token sequence bit on the way: some caption is not what the single tokens alone give
    assert any(_generated(seq, lens, b, blip2) != under_singles[b] for b in range(B))
    # step 0 sees the same context as the unconstrained call: its raw logits are that call's, bit for bit
    assert torch.equal(out["logits"][0], free["logits"][0])
    print(f"\n{family} {dtype}: {steps} emitted tokens replayed, {changed} of {B} captions changed, set {seqs}")
    eng.close()


@pytest.mark.parametrize("path", ["batch", "small", "compacted"])
def test_prompted_replay_a_sequence_matches_across_the_prompt_boundary(path):
    """Prompted generate under a set whose sequences START in the prompt: [last prompt token, x] and [the two prompt tokens, y] ban x
    and y as first generated tokens only because the context holds the prompt; a sequence through BOS's neighbour that the prompt
    does not spell bans nothing.  The loop starts at t = P - 1 and the step outputs are indexed from there."""
    B = 20 if path == "compacted" else 8
    arch, sd, px = _blip(B)
    prompt = [arch.bos, 31, 47]
    eng = _engine(arch, sd, "f32s", B, L_BLIP, max_prompt=len(prompt))
    eng.set_decode_path("batch" if path == "compacted" else path)
    free = eng.generate(px.cuda(), max_length=L_BLIP, prompt_ids=prompt, output_logits=True)
    assert _replay(arch, free, [], False, prompt) > B
    first = free["sequences"][:, len(prompt)].cpu().tolist()
    x = max(set(first), key=first.count)
    assert x not in (arch.eos, arch.pad, arch.bos)
    runner_up = int(torch.topk(free["logits"][0, first.index(x)], 2).indices[1])          # what that row takes once x is banned
    seqs = [[47, x], [31, 47, runner_up], [48, 47, 60], [31, 46, 61]]
    eng.set_bad_words(seqs)
    out = eng.generate(px.cuda(), max_length=L_BLIP, prompt_ids=prompt, output_logits=True, bad_words_ids=seqs)
    steps = _replay(arch, out, seqs, False, prompt)
    got = out["sequences"][:, len(prompt)].cpu().tolist()
    assert all(g not in (x, runner_up) for g in got) and torch.equal(out["logits"][0], free["logits"][0])
    assert torch.equal(out["sequences"][:, :len(prompt)].cpu(), torch.tensor([prompt] * B, dtype=torch.int32))
    if path == "compacted":          # the same call without per-step logits runs compacted, to the same tokens
        eng.set_row_compaction(True)
        c = eng.generate(px.cuda(), max_length=L_BLIP, prompt_ids=prompt)
        assert eng.last_row_compaction and _same(c, out)
    else:
        assert eng.last_decode_path == path
    print(f"\nprompted {path}: {steps} generated tokens replayed, first tokens {first} -> {got}")
    eng.close()


def _banned_blip_engine(B, dtype="f32s", **kw):
    arch, sd, px = _blip(B)
    seqs, _ = _ban_set("blip", dtype)
    eng = _engine(arch, sd, dtype, B, L_BLIP, **kw)
    free = eng.generate(px.cuda(), max_length=L_BLIP)
    eng.set_bad_words(seqs)
    return arch, sd, px, eng, seqs, free


def _same(a, b, keys=("sequences", "lengths")):
    return all(torch.equal(a[k], b[k]) for k in keys)


def test_row_alone_small_path_and_image_state_give_the_batch_bits():
    B = 6
    arch, sd, px, eng, seqs, free = _banned_blip_engine(B)
    eng.set_decode_path("batch")
    ref = eng.generate(px.cuda(), max_length=L_BLIP, output_logits=True)
    assert eng.last_decode_path == "batch" and not _same(ref, free)
    for b in (0, 3):
        one = eng.generate(px[b:b + 1].cuda(), max_length=L_BLIP, output_logits=True)
        assert torch.equal(one["sequences"][0], ref["sequences"][b]) and torch.equal(one["lengths"][0], ref["lengths"][b])
        assert torch.equal(one["logits"][:, 0], ref["logits"][:, b])
    eng.set_decode_path("small")
    small = eng.generate(px.cuda(), max_length=L_BLIP, output_logits=True)
    assert eng.last_decode_path == "small" and _same(small, ref, ("sequences", "lengths", "logits"))
    eng.set_decode_path("auto")
    state = eng.image_state(px.cuda())
    assert _same(eng.generate(state, max_length=L_BLIP), ref)
    # beams under the same set: no banned token or sequence in the best hypotheses, and they are not the unbanned search's
    eng.close()
    eng = _engine(arch, sd, "f32s", B, L_BLIP, beams=3)
    fb = eng.generate(px.cuda(), num_beams=3, max_length=L_BLIP)
    eng.set_bad_words(seqs)
    ob = eng.generate(px.cuda(), num_beams=3, max_length=L_BLIP)
    s, n = ob["sequences"].cpu().numpy(), ob["lengths"].cpu().numpy()
    assert all(not _contains_ban(_generated(s, n, b, False), seqs) for b in range(B))
    assert not torch.equal(ob["sequences"], fb["sequences"])
    assert _same(eng.generate(eng.image_state(px.cuda()), num_beams=3, max_length=L_BLIP), ob, ("sequences", "lengths", "sequences_scores"))
    eng.close()


def test_compacted_loop_gives_the_uncompacted_bits():
    B = 20                                                                          # above the small-batch row limit
    arch, sd, px, eng, seqs, free = _banned_blip_engine(B)
    # without the single token most captions start with: those captions keep their early EOS and leave the loop one by one, while
    # the set still bites in the others
    first = free["sequences"][:, 1].cpu().tolist()
    seqs = [q for q in seqs if q != [max(set(first), key=first.count)]]
    eng.set_bad_words(seqs)
    eng.set_row_compaction(True)
    a = eng.generate(px.cuda(), max_length=L_BLIP)
    assert eng.last_row_compaction
    eng.set_row_compaction(False)
    b = eng.generate(px.cuda(), max_length=L_BLIP)
    assert not eng.last_row_compaction
    assert _same(a, b) and not _same(a, free)
    s, n = a["sequences"].cpu().numpy(), a["lengths"].cpu().numpy()
    assert all(not _contains_ban(_generated(s, n, r, False), seqs) for r in range(B))
    assert len(set(n.tolist())) > 1, "every caption ended at the same step: the compacted loop never dropped a row"
    eng.close()


def test_pool_merged_batches_give_the_single_calls_bits():
    from embodied_captioning_amd.engine import EnginePool
    B = 4
    arch, sd, px, eng, seqs, free = _banned_blip_engine(2 * B)
    pool = EnginePool(arch, n=2, dtype="f32s", max_batch=2 * B, max_beams=1, max_len=L_BLIP, weights_of=eng)
    pool.set_bad_words(seqs)
    assert pool.bad_words == seqs
    batches = [px[:B].cuda(), px[B:].cuda()]
    outs = pool.generate_many(batches, coalesce_rows=2 * B, max_length=L_BLIP)
    assert pool.last_coalesce is not None
    for o, p in zip(outs, batches):
        assert _same(o, eng.generate(p, max_length=L_BLIP))
    pool.close()
    eng.close()


def test_set_then_clear_is_a_handle_that_never_had_a_set_and_scoring_ignores_it():
    B = 4
    arch, sd, px, eng, seqs, _ = _banned_blip_engine(B)
    ids = np.full((B, 4), arch.pad, dtype=np.int32)
    ids[:, 0] = arch.bos
    ids[:, 1:4] = np.arange(20, 23)
    ids[:, 1] = seqs[0][0]                                                          # a banned token among the GIVEN tokens
    lens = np.full(B, 4, dtype=np.int32)
    scored = eng.score(px.cuda(), ids, lens)
    eng.set_bad_words([])
    assert eng.bad_words == [] and eng.bad_words_counts == (0, 0)
    fresh = _engine(arch, sd, "f32s", B, L_BLIP)
    a = eng.generate(px.cuda(), max_length=L_BLIP, output_logits=True, output_logprobs=True)
    b = fresh.generate(px.cuda(), max_length=L_BLIP, output_logits=True, output_logprobs=True)
    assert _same(a, b, ("sequences", "lengths", "logits", "token_logprobs", "scored_steps"))
    plain = fresh.score(px.cuda(), ids, lens)
    assert torch.equal(scored["token_logprobs"], plain["token_logprobs"]) and torch.equal(scored["top_ids"], plain["top_ids"])
    eng.close()
    fresh.close()


def test_blip2_beams_and_image_state_under_the_set():
    B = 3
    arch, sd, px = _blip2(B)
    L = arch.max_new_tokens
    eng = _engine(arch, sd, "bf16", B, L, beams=3)
    free = eng.generate(px.cuda(), max_length=L)
    seqs, _ = _ban_set("blip2", "bf16")
    fb = eng.generate(px.cuda(), num_beams=3, max_length=L)
    eng.set_bad_words(seqs)
    g = eng.generate(px.cuda(), max_length=L)
    ob = eng.generate(px.cuda(), num_beams=3, max_length=L)
    for o in (g, ob):
        s, n = o["sequences"].cpu().numpy(), o["lengths"].cpu().numpy()
        assert all(not _contains_ban(_generated(s, n, b, True), seqs) for b in range(B))
    assert not torch.equal(g["sequences"], free["sequences"])
    state = eng.image_state(px.cuda())
    assert _same(eng.generate(state, max_length=L), g)
    assert _same(eng.generate(state, num_beams=3, max_length=L), ob, ("sequences", "lengths", "sequences_scores"))
    one = eng.generate(px[1:2].cuda(), max_length=L)
    assert torch.equal(one["sequences"][0], g["sequences"][1])
    with pytest.raises(ValueError, match="image placeholder"):
        eng.set_bad_words([[5, arch.image_token]])
    assert eng.bad_words == seqs                                                    # a refused set leaves the one in force
    eng.close()


def test_refusals_by_message():
    from embodied_captioning_amd import _native as N
    B = 2
    arch, sd, px, eng, seqs, _ = _banned_blip_engine(B)
    with pytest.raises(ValueError, match="differs from the set in force"):
        eng.generate(px.cuda(), max_length=L_BLIP, bad_words_ids=seqs + [[9]])
    with pytest.raises(ValueError, match="differs from the set in force"):
        eng.generate(px.cuda(), max_length=L_BLIP, bad_words_ids=[])
    eng.generate(px.cuda(), max_length=L_BLIP, bad_words_ids=seqs + [[arch.eos]])         # [eos] alone is dropped: the same set
    for kw in ({"output_logprobs": True}, {"output_vocab_maxprob": True}):
        with pytest.raises(N.CaptionerHipError, match="bad words are set on this handle"):
            eng.generate(px.cuda(), max_length=L_BLIP, **kw)
    with pytest.raises(ValueError, match="force_words_ids"):
        eng.generate(px.cuda(), max_length=L_BLIP, force_words_ids=[[5]])
    # beam groups under a set: refused as such, ahead of "groups are CoCa's"
    with pytest.raises(N.CaptionerHipError, match="bad words are set on this handle.*beam groups do not take them"):
        eng.generate(px.cuda(), max_length=L_BLIP, num_beams=1, num_beam_groups=1)
    # the library's own checks (a caller of the C ABI has no host validation in front of it)
    lib = eng.lib

    def lib_set(rows):
        flat = [t for q in rows for t in q]
        offs = np.cumsum([0] + [len(q) for q in rows]).tolist()
        rc = lib.cap_set_bad_words(eng._h, (C.c_int32 * max(len(flat), 1))(*flat), (C.c_int32 * len(offs))(*offs), len(rows),
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream))
        return rc, lib.cap_last_error().decode()
    for rows, word in (([[5], []], "is empty"), ([[arch.vocab]], "outside the vocabulary"), ([[5, arch.bos]], "BOS"), ([[arch.pad]], "pad"),
                       ([list(range(3, 12))], "at most 8"), ([[5, 6 + i % 300] for i in range(1025)], "more than 1024")):
        rc, msg = lib_set(rows)
        assert rc != 0 and word in msg, (word, msg)
    assert eng.bad_words_counts == (sum(len(q) == 1 for q in seqs), sum(len(q) > 1 for q in seqs))      # a refused set changes nothing
    rc, msg = lib_set([[arch.eos]])                                                  # only [eos]: dropped, the set is empty
    assert rc == 0 and eng.bad_words_counts == (0, 0)
    eng.close()


def test_a_coca_handle_with_a_set_refuses_to_generate():
    """The host validation refuses a set for CoCa, so only a caller of the C ABI can put one on a CoCa handle: cap_generate_request
    then refuses by name - greedy, beams and beam groups - and generates again once the set is cleared."""
    from embodied_captioning_amd import _native as N
    from embodied_captioning_amd.config import CocaArch
    from embodied_captioning_amd.engine import CaptionerEngine
    from embodied_captioning_amd.weights import procedural_coca_state_dict, synthetic_pixels
    a = CocaArch.tiny()
    eng = CaptionerEngine(a, dtype="f32s", max_batch=2, max_beams=2, max_len=a.seq_len)
    eng.load_state_dict(procedural_coca_state_dict(a, 1, eos_boost=4.0))
    px = synthetic_pixels(2, a.image_size, seed=1).cuda()
    with pytest.raises(ValueError, match="CoCa"):
        eng.set_bad_words([[5]])
    free = eng.generate(px, max_length=a.seq_len)

    def lib_set(rows):
        flat = [t for q in rows for t in q]
        offs = np.cumsum([0] + [len(q) for q in rows]).tolist()
        return eng.lib.cap_set_bad_words(eng._h, (C.c_int32 * max(len(flat), 1))(*flat), (C.c_int32 * len(offs))(*offs), len(rows),
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream))
    ok = [t for t in range(5, 9) if t not in (a.sot, a.eos, a.pad)][:1]
    assert lib_set([ok]) == 0 and eng.bad_words_counts == (1, 0)
    for kw in ({}, {"num_beams": 2}, {"num_beams": 2, "num_beam_groups": 2}):
        with pytest.raises(N.CaptionerHipError, match="bad words are set on this handle.*CoCa captioner"):
            eng.generate(px, max_length=a.seq_len, **kw)
    assert lib_set([]) == 0 and eng.bad_words_counts == (0, 0)
    assert _same(eng.generate(px, max_length=a.seq_len), free)
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ HF goldens
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCORE_BAR = 2e-3          # tests/test_configs_gpu.py (BLIP beam 3), tests/test_blip2_beam_gpu.py


def _compare_golden(g, key, bar, ids, lens, scores=None):
    """Rows whose every step margin in HF's run reaches the bar: tokens up to the caption's end, lengths, beam scores."""
    ok = np.nonzero(g[f"{key}_margin"].min(axis=0) >= bar)[0]
    assert len(ok) * 8 >= 7 * ids.shape[0], (key, "more than 1 row in 8 below the bar", g[f"{key}_margin"].min(axis=0))
    want, want_len = g[f"{key}_ids"], g[f"{key}_lengths"]
    for b in ok:
        assert int(lens[b]) == int(want_len[b]), (key, b, int(lens[b]), int(want_len[b]), ids[b], want[b])
    return ok, want


@pytest.mark.parametrize("dtype", ["f32", "f32s"])
def test_blip_tiny_matches_hf_under_the_ban(dtype):
    from embodied_captioning_amd.config import BlipArch
    from embodied_captioning_amd.weights import procedural_blip_state_dict, synthetic_pixels
    g = np.load(os.path.join(GOLDEN, "blip_tiny_bad_words.npz"))
    meta = json.loads(str(g["meta"]))
    arch, B, L, bar = BlipArch(**meta["arch"]), meta["batch"], meta["max_length"], meta["bar"]
    sd = procedural_blip_state_dict(arch, meta["seed"], eos_boost=meta["eos_boost"])
    px = synthetic_pixels(B, arch.image_size, seed=meta["seed"]).cuda()
    ban, ban_p, prompt = json.loads(str(g["ban"])), json.loads(str(g["ban_prompt"])), g["prompt_ids"].tolist()
    assert ban_p[-1][0] == prompt[-1] and len(ban_p[-1]) == 2                   # the prompt's last token starts a banned sequence
    eng = _engine(arch, sd, dtype, B, L, beams=3, max_prompt=len(prompt))
    eng.set_bad_words(ban)
    for key, kw, first in (("greedy", {}, 1), ("beams3", {"num_beams": 3}, 1), ("prompted", {"prompt_ids": prompt}, len(prompt))):
        if key == "prompted":
            eng.set_bad_words(ban_p)
        out = eng.generate(px, max_length=L, **kw)
        seq, lens = out["sequences"].cpu().numpy(), out["lengths"].cpu().numpy()
        ok, want = _compare_golden(g, key, bar, seq, lens)
        for b in ok:
            n = int(lens[b]) - first
            assert np.array_equal(seq[b, first:first + n], want[b, :n]), (key, b, seq[b], want[b])
        if key == "beams3":
            err = np.abs(out["sequences_scores"].cpu().numpy() - g["beams3_scores"])[ok]
            print(f"\nblip {dtype} beams3 under the ban: score error {err.max():.3e} over rows {ok.tolist()}")
            assert err.max() < SCORE_BAR
        if key == "prompted":
            assert np.array_equal(seq[:, :first], np.tile(prompt, (B, 1)))
    eng.close()


@pytest.mark.parametrize("dtype", ["f32", "f32s"])
def test_blip2_tiny_matches_hf_under_the_ban(dtype):
    from embodied_captioning_amd.config import Blip2Arch
    from embodied_captioning_amd.weights import procedural_blip2_state_dict, synthetic_pixels
    g = np.load(os.path.join(GOLDEN, "blip2_tiny_bad_words.npz"))
    meta = json.loads(str(g["meta"]))
    arch, B, bar = Blip2Arch(**meta["arch"]), meta["batch"], meta["bar"]
    n_new = arch.max_new_tokens
    sd = procedural_blip2_state_dict(arch, meta["seed"], eos_boost=meta["eos_boost"])
    px = synthetic_pixels(B, arch.image_size, seed=meta["seed"]).cuda()
    eng = _engine(arch, sd, dtype, B, n_new, beams=3)
    eng.set_bad_words(json.loads(str(g["ban"])))
    for key, kw in (("greedy", {}), ("beams3", {"num_beams": 3})):
        out = eng.generate(px, max_length=n_new, **kw)
        seq, lens = out["sequences"].cpu().numpy(), out["lengths"].cpu().numpy()
        ok, want = _compare_golden(g, key, bar, seq, lens)
        for b in ok:
            assert np.array_equal(seq[b, :int(lens[b])], want[b, :int(lens[b])]), (key, b, seq[b], want[b])
        if key == "beams3":
            err = np.abs(out["sequences_scores"].cpu().numpy() - g["beams3_scores"])[ok]
            print(f"\nblip2 {dtype} beams3 under the ban: score error {err.max():.3e} over rows {ok.tolist()}")
            assert err.max() < SCORE_BAR
    eng.close()
