"""GPU: CaptionerEngine on CoCa against the float64 goldens of tools/make_goldens_coca.py directly (HF CLIP vision trunk and
text tower, torch.nn pooler and decoder, full-prefix greedy loop), not against oracle/coca_ref.py.  The bars are those the
restatement tests hold (test_coca_gpu.py); every test prints its measured errors."""
import numpy as np
import pytest
import torch

from _util import coca_golden, pad_to, strided, token_parity

pytestmark = pytest.mark.gpu

# (encoder tokens / pooled, step top-8 logits); None = not held in that mode
TINY_BARS = {"f32": (2e-4, 1e-3), "f32s": (2e-4, 1e-3), "bf16": (0.15, None)}
FULL_BARS = {"f32": (2e-3, 1e-3), "f32s": (2e-3, 1e-3), "bf16": (0.25, 0.35)}
BF16_TAU = 0.3                                    # token_parity: a bf16 row may leave the golden path only at a near-tie


def _engine(a, dtype, batch, cross_cache="auto"):
    from embodied_captioning_amd.engine import CaptionerEngine
    return CaptionerEngine(a, dtype=dtype, max_batch=batch, max_beams=1, max_len=a.seq_len, cross_cache=cross_cache)


def _encoder_error(eng, g, sd, px):
    """max |engine - golden| over the strided sample of the image tokens and over pooled (token 0 @ visual.proj)."""
    tok = eng.encode(px.cuda()).cpu().double()      # [B, Q, E]: row 0 the pooled token before visual.proj, rows 1.. image_embs
    e_tok = np.abs(strided(tok[:, 1:], g["tokens_stride"]) - g["tokens_sample"]).max()
    e_pool = np.abs((tok[:, 0] @ sd["visual.proj"].double()).numpy() - g["pooled"]).max()
    return max(e_tok, e_pool)


def _step_top8_errors(logits, g, steps=None):
    """Per step: max |engine - golden| at the golden's top-8 ids of the rows active at that step."""
    act = g["step_active"]
    errs = []
    for t in range(act.shape[0] if steps is None else steps):
        rows = np.nonzero(act[t])[0]
        ids = torch.from_numpy(g["step_top8_ids"][t][rows]).long()
        ours = torch.gather(logits[t, torch.from_numpy(rows)].double(), 1, ids).numpy()
        errs.append(np.abs(ours - g["step_top8_vals"][t][rows]).max())
    return np.array(errs)


def _margins(g, L):
    """The golden's top-1 / top-2 margins as token_parity reads them: [L-1, B], inactive rows never near a tie."""
    m = np.full((L - 1, g["step_margin"].shape[1]), 1e9)
    m[: g["step_margin"].shape[0]] = np.where(g["step_active"], g["step_margin"], 1e9)
    return m


MODES = [("f32", "auto"), ("f32s", "auto"), ("f32s", "fp32"), ("bf16", "auto")]
CASES = [("coca_tiny", "b0_"), ("coca_tiny", "b4_"), ("coca_width", "")]


@pytest.mark.parametrize("dtype,cross_cache", MODES, ids=[f"{d}-{c}" for d, c in MODES])
@pytest.mark.parametrize("name,part", CASES, ids=["tiny_b0", "tiny_b4", "width"])
def test_engine_matches_fp64_golden(name, part, dtype, cross_cache):
    """Tiny (eos_boost 0 and 4: long and early-EOS rows) and production width with two layers per tower: encoder tokens and
    pooled, greedy sequences, and every step's logits at the golden's top-8 ids."""
    g, meta, a, sd, px = coca_golden(name, part)
    enc_bar, logit_bar = (TINY_BARS if name == "coca_tiny" else FULL_BARS)[dtype]
    eng = _engine(a, dtype, meta["batch"], cross_cache)
    try:
        eng.load_state_dict(sd)
        if "tokens_sample" in g:                     # the eos_boost 4 part shares the image side of the eos_boost 0 part
            err = _encoder_error(eng, g, sd, px)
            print(f"{name}{part} {dtype}/{cross_cache}: encoder {err:.3g}")
            assert err < enc_bar, err
        out = eng.generate(px.cuda(), max_length=a.seq_len, output_logits=True)
        seq = out["sequences"].cpu().numpy()
        want = pad_to(g["sequences"], a.seq_len, a.pad)
        logits = out["logits"].cpu()
        if dtype == "bf16":
            if logit_bar is not None:
                e0 = _step_top8_errors(logits, g, steps=1).max()
                print(f"{name}{part} {dtype}: step-0 top-8 {e0:.3g}")
                assert e0 < logit_bar, e0
            if name == "coca_tiny":
                exact, diverged, bad = token_parity(seq, want, _margins(g, a.seq_len), BF16_TAU)
                print(f"{name}{part} {dtype}: {exact} rows exact, {diverged} left the golden path at a near-tie")
                assert bad is None, bad
        else:
            assert np.array_equal(seq, want), (seq, want)
            errs = _step_top8_errors(logits, g)
            print(f"{name}{part} {dtype}/{cross_cache}: step top-8 max {errs.max():.3g} (step 0 {errs[0]:.3g})")
            assert errs.max() < logit_bar, errs
        if dtype == "f32s":
            assert eng.saturations(reset=True) == 0
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------- full coca_ViT-L-14
@pytest.fixture(scope="module", params=["f32s", "bf16"])
def l14_224(request):
    g, meta, a, sd, px = coca_golden("coca_l14_image")
    eng = _engine(a, request.param, meta["batch"])
    eng.load_state_dict(sd)
    yield request.param, eng, g, a, sd, px
    eng.close()


@pytest.fixture(scope="module", params=["f32s", "bf16"])
def l14_336(request):
    g, meta, a, sd, px = coca_golden("coca_l14_336_image")
    assert a.n_tokens == 577 and meta["weights_image_size"] == 224
    eng = _engine(a, request.param, meta["batch"])
    eng.load_state_dict(sd)
    yield request.param, eng, g, a, sd, px
    eng.close()


def test_l14_224_encoder_matches_fp64_golden(l14_224):
    dtype, eng, g, a, sd, px = l14_224
    err = _encoder_error(eng, g, sd, px)
    print(f"coca_l14_image {dtype}: encoder {err:.3g}")
    assert err < FULL_BARS[dtype][0], err
    if dtype == "f32s":
        assert eng.saturations(reset=True) == 0


def test_l14_224_first_tokens_and_step0_match_fp64_golden(l14_224):
    """Step-0 logits at the golden's top-8 ids, and (f32s) the first greedy tokens (seq_len 8) identical."""
    dtype, eng, g, a, sd, px = l14_224
    out = eng.generate(px.cuda(), max_length=a.seq_len, output_logits=True)
    e0 = _step_top8_errors(out["logits"].cpu(), g, steps=1).max()
    print(f"coca_l14_image {dtype}: step-0 top-8 {e0:.3g}")
    assert e0 < FULL_BARS[dtype][1], e0
    seq = out["sequences"].cpu().numpy()
    if dtype == "f32s":
        assert np.array_equal(seq, pad_to(g["sequences"], a.seq_len, a.pad)), (seq, g["sequences"])
        assert eng.saturations(reset=True) == 0
    else:
        assert (seq[:, 0] == a.sot).all() and (seq[:, -1] == a.eos).all()


def test_l14_336_encoder_matches_fp64_golden(l14_336):
    """336 px (577 tokens, the online-softmax ViT attention kernel), position table of a 224-px checkpoint resized at load."""
    dtype, eng, g, a, sd, px = l14_336
    err = _encoder_error(eng, g, sd, px)
    print(f"coca_l14_336_image {dtype}: encoder {err:.3g}")
    assert err < FULL_BARS[dtype][0], err
    if dtype == "f32s":
        assert eng.saturations(reset=True) == 0
