"""CPU: the CoCa restatement (oracle/coca_ref.py) against float64 goldens computed by implementations that are not it
(tools/make_goldens_coca.py): HuggingFace CLIPVisionModel for the vision trunk, CLIPTextModel for the unimodal text tower,
torch.nn modules for the attentional pooler and the multimodal decoder, and a full-prefix greedy loop.  Then the bars are
shown to catch a wrong composition, and the loader is shown to take the pooler's packed in_proj."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _util import coca_golden, strided
from embodied_captioning_amd.coca_weights import derive_coca_tensors
from oracle import coca_ref as R

# restatement (fp32) against the fp64 goldens; measured 1e-6 .. 7e-6
TOK_ATOL = 2e-5          # trunk / image tokens / pooled / text tokens (values up to ~6)
NORM_RTOL = 1e-5         # per-token L2 norms
LOGIT_ATOL = 5e-5        # top-8 logits and logsumexp of every step (values up to ~12)

CASES = [("coca_tiny", "b0_"), ("coca_tiny", "b4_"), ("coca_width", "")]
IMAGE_CASES = [("coca_tiny", "b0_"), ("coca_width", "")]


def _ids(cases):
    return [n + ("_" + p.rstrip("_") if p else "") for n, p in cases]


def _encode_with_layers(sd, a, px, monkeypatch):
    """R.encode_image, recording the trunk after ln_pre and after every vision block (HF hidden_states[0..])."""
    seen = []
    ln, block = R._ln, R._block

    def rec_ln(x, sd_, p, eps):
        y = ln(x, sd_, p, eps)
        if p == "visual.ln_pre":
            seen.append(y)
        return y

    def rec_block(x, sd_, p, *args, **kw):
        y = block(x, sd_, p, *args, **kw)
        if p.startswith("visual.transformer."):
            seen.append(y)
        return y

    with monkeypatch.context() as m:
        m.setattr(R, "_ln", rec_ln)
        m.setattr(R, "_block", rec_block)
        pooled, tokens = R.encode_image(sd, a, px)
    return pooled, tokens, seen


@pytest.mark.parametrize("name,part", IMAGE_CASES, ids=_ids(IMAGE_CASES))
def test_restatement_image_side_matches_hf_clip_golden(name, part, monkeypatch):
    g, meta, a, sd, px = coca_golden(name, part)
    pooled, tokens, layers = _encode_with_layers(sd, a, px, monkeypatch)
    assert len(layers) == a.v_layers + 1 == g["trunk_layer_norms"].shape[0]
    for i, h in enumerate(layers):
        np.testing.assert_allclose(h.norm(dim=-1).numpy(), g["trunk_layer_norms"][i], rtol=NORM_RTOL, atol=0,
                                   err_msg=f"trunk token norms after {'ln_pre' if i == 0 else f'block {i - 1}'}")
    np.testing.assert_allclose(strided(layers[-1], g["trunk_stride"]), g["trunk_sample"], rtol=0, atol=TOK_ATOL)
    np.testing.assert_allclose(strided(tokens, g["tokens_stride"]), g["tokens_sample"], rtol=0, atol=TOK_ATOL)
    np.testing.assert_allclose(tokens.norm(dim=-1).numpy(), g["tokens_norm"], rtol=NORM_RTOL, atol=0)
    np.testing.assert_allclose(pooled.numpy(), g["pooled"], rtol=0, atol=TOK_ATOL)


@pytest.mark.parametrize("name,part", CASES, ids=_ids(CASES))
def test_restatement_text_tower_matches_hf_clip_golden(name, part):
    g, meta, a, sd, px = coca_golden(name, part)
    tt = R.text_tokens_full(sd, a, torch.from_numpy(g["sequences"]))
    np.testing.assert_allclose(strided(tt, g["text_stride"]), g["text_sample"], rtol=0, atol=TOK_ATOL)
    np.testing.assert_allclose(tt.norm(dim=-1).numpy(), g["text_norm"], rtol=NORM_RTOL, atol=0)


def _step_errors(g, logits):
    """Per step: max |restatement - golden| over the golden's top-8 ids of the active rows, and of the logsumexp."""
    act = g["step_active"]
    assert len(logits) == act.shape[0]
    top, lse = [], []
    for t, lg in enumerate(logits):
        ids = torch.from_numpy(g["step_top8_ids"][t][act[t]]).long()
        assert lg.shape[0] == ids.shape[0]
        top.append(np.abs(torch.gather(lg, 1, ids).numpy() - g["step_top8_vals"][t][act[t]]).max())
        lse.append(np.abs(torch.logsumexp(lg, -1).numpy() - g["step_logsumexp"][t][act[t]]).max())
    return np.array(top), np.array(lse)


@pytest.mark.parametrize("name,part", CASES, ids=_ids(CASES))
def test_restatement_greedy_decode_matches_golden(name, part):
    g, meta, a, sd, px = coca_golden(name, part)
    _, tokens = R.encode_image(sd, a, px)
    out = R.generate_top1(sd, a, px, image_embs=tokens)          # the KV-cached step
    assert np.array_equal(out["text"].numpy(), g["sequences"]), (out["text"], g["sequences"])
    top, lse = _step_errors(g, out["logits"])
    assert top.max() < LOGIT_ATOL, top
    assert lse.max() < LOGIT_ATOL, lse


def test_goldens_cover_early_eos_and_full_length_rows():
    """The tiny fixture's two eos_boost parts give both kinds of rows, so the decode rules above are exercised."""
    _, _, a, _, _ = coca_golden("coca_tiny", "b0_")
    long = coca_golden("coca_tiny", "b0_")[0]["sequences"]
    short = coca_golden("coca_tiny", "b4_")[0]["sequences"]
    assert long.shape[1] == a.seq_len and (long[:, -1] == a.eos).all()
    ends = [list(r).index(a.eos) for r in short]
    assert min(ends) >= a.min_seq_len and min(ends) < short.shape[1] - 1
    assert (short == a.pad).any()


# ------------------------------------------------------------------------------------------------------ sensitivity
def _tanh_gelu(monkeypatch):
    f = types.SimpleNamespace(**vars(F))
    f.gelu = lambda x: F.gelu(x, approximate="tanh")
    monkeypatch.setattr(R, "F", f)


def _skip_ln_1_kv(monkeypatch):
    ln = R._ln
    monkeypatch.setattr(R, "_ln", lambda x, sd, p, eps: x if p.endswith(".ln_1_kv") else ln(x, sd, p, eps))


def _ln_final_on_decoder_input(monkeypatch):
    tt = R.text_tokens_full
    monkeypatch.setattr(R, "text_tokens_full", lambda sd, a, text: R._ln(tt(sd, a, text), sd, "text.ln_final", a.eps))


def _shift(key):
    def perturb(sd):
        sd = dict(sd)
        sd[key] = torch.roll(sd[key], 1, 0)
        return sd
    return perturb


PERTURBATIONS = {
    "none": (None, None),
    "tanh_gelu": (_tanh_gelu, None),
    "visual_pos_one_row_off": (None, _shift("visual.positional_embedding")),
    "text_pos_one_row_off": (None, _shift("text.positional_embedding")),
    "skip_ln_1_kv": (_skip_ln_1_kv, None),
    "ln_final_on_decoder_input": (_ln_final_on_decoder_input, None),
}


@pytest.mark.parametrize("what", list(PERTURBATIONS))
def test_bars_catch_a_wrong_composition(what, monkeypatch):
    """Each perturbation is a composition mistake the restatement could have made and the HIP path would then copy.  Against
    the golden, through the checks above (image tokens, text tower, step logits of the first steps on the golden's prefix),
    it must miss a bar by at least 10x, and every perturbation must fail the step-logit bar on its own.  Unperturbed,
    everything is within the bars.  (Measured on the tiny fixture: tanh-GELU 33x on the image tokens and 7x on the logits;
    the other three miss by 2 000x and more.)"""
    g, meta, a, sd, px = coca_golden("coca_tiny", "b0_")
    patch, edit = PERTURBATIONS[what]
    if patch is not None:
        patch(monkeypatch)
    if edit is not None:
        sd = edit(sd)
    _, tokens = R.encode_image(sd, a, px)
    text = torch.from_numpy(g["sequences"])
    tt = R.text_tokens_full(sd, a, text)
    lg = [R.last_logits_full(sd, a, tokens, text[:, :n]) for n in (1, 2, 3)]
    top, _ = _step_errors({k: g[k][:3] for k in ("step_active", "step_top8_ids", "step_top8_vals", "step_logsumexp")}, lg)
    ratios = {"image tokens": np.abs(strided(tokens, g["tokens_stride"]) - g["tokens_sample"]).max() / TOK_ATOL,
              "text tower": np.abs(strided(tt, g["text_stride"]) - g["text_sample"]).max() / TOK_ATOL,
              "step logits": top.max() / LOGIT_ATOL}
    if what == "none":
        assert max(ratios.values()) < 1, ratios
        return
    assert max(ratios.values()) >= 10, f"{what}: {ratios}"
    assert ratios["step logits"] > 1, f"{what}: {ratios}"


# ---------------------------------------------------------------------------------------------------------- loader
def test_derive_accepts_the_poolers_packed_in_proj():
    """When the pooler's width equals the vision width (CocaArch.tiny()), nn.MultiheadAttention - and so an open_clip
    checkpoint - holds ONE packed attn_pool.attn.in_proj_weight instead of q/k/v_proj_weight: same derived tensors."""
    import torch.nn as nn
    from embodied_captioning_amd.config import CocaArch
    from embodied_captioning_amd.weights import procedural_coca_state_dict
    a = CocaArch.tiny()
    assert a.embed_dim == a.v_hidden
    sd = procedural_coca_state_dict(a, 4)
    p = "visual.attn_pool.attn."
    packed = {k: v for k, v in sd.items() if not k.endswith(("q_proj_weight", "k_proj_weight", "v_proj_weight"))}
    packed[p + "in_proj_weight"] = torch.cat([sd[p + "q_proj_weight"], sd[p + "k_proj_weight"], sd[p + "v_proj_weight"]], 0)
    # the layout is the module's own
    mha = nn.MultiheadAttention(a.embed_dim, a.pool_heads, kdim=a.v_hidden, vdim=a.v_hidden, batch_first=True)
    assert set(mha.state_dict()) == {k[len(p):] for k in packed if k.startswith(p)}
    want, got = derive_coca_tensors(sd, a), derive_coca_tensors(packed, a)
    assert set(want) == set(got)
    for k in want:
        assert torch.equal(want[k], got[k]), k
