#!/usr/bin/env python
"""Golden vectors for the CoCa path, computed in float64 from implementations that are not oracle/coca_ref.py:

  * vision trunk: HuggingFace `CLIPVisionModel` (hidden_act "gelu", pre_layrnorm = open_clip ln_pre, no post_layernorm:
    hidden_states[-1] is the trunk the pooler reads);
  * attentional pooler: torch.nn modules - LayerNorm ln_k on the tokens, LayerNorm ln_q on the learned queries,
    `nn.MultiheadAttention(E, pool_heads, kdim=vdim=v_hidden)`, LayerNorm ln_post; pooled = token 0 @ visual.proj;
  * unimodal text tower: HuggingFace `CLIPTextModel` whose vocabulary has one extra row (= text.cls_emb) and whose position
    table has context_length + 1 rows; the cls id is appended to every prefix and the per-token outputs are
    hidden_states[-1][:, :-1] (before final_layer_norm, which open_clip applies to the pooled cls branch only);
  * multimodal decoder: per layer a causal `nn.TransformerEncoderLayer(norm_first=True, activation="gelu")` and a
    cross-attention block of nn.LayerNorm ln_1 / ln_1_kv, nn.MultiheadAttention and a Linear-GELU-Linear MLP; then
    ln_final and @ text_projection;
  * greedy decode: the top-k(1) loop of the reference's CoCa `generate` with full-prefix recompute every step (no KV cache):
    MinLength(min_seq_len, eos), forced EOS at cur_len + 1 == seq_len, rows whose last token is EOS / pad emit pad.

Weights are not stored: every fixture holds arch, seed, eos_boost and batch, and the weights / pixels are re-drawn from
embodied_captioning_amd.weights.  Runs in the build container only (transformers); the tests never import it.

    python tools/make_goldens_coca.py [name ...]      # names: coca_tiny coca_width coca_l14_image coca_l14_336_image
"""
import dataclasses
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from embodied_captioning_amd.coca_weights import coca_library_state_dict  # noqa: E402
from embodied_captioning_amd.config import CocaArch  # noqa: E402
from embodied_captioning_amd.weights import procedural_coca_state_dict, synthetic_pixels  # noqa: E402

SAMPLE = 2048            # about this many values per strided sample


def _sample(x):
    """Every s-th value of each batch row, s chosen for about SAMPLE values a row -> (s, [B, n])."""
    s = max(1, x[0].numel() // SAMPLE)
    return np.array(s), x.reshape(x.shape[0], -1)[:, ::s].numpy()


def _load(mod: nn.Module, sd):
    mod.load_state_dict({k: v.double() for k, v in sd.items()}, strict=True)
    return mod


# ------------------------------------------------------------------------------------------------------ image side
def vision_model(a: CocaArch, sd):
    from transformers import CLIPVisionConfig, CLIPVisionModel
    c = CLIPVisionConfig(hidden_size=a.v_hidden, intermediate_size=a.v_mlp, num_hidden_layers=a.v_layers,
                         num_attention_heads=a.v_heads, image_size=a.image_size, patch_size=a.patch_size, num_channels=3,
                         hidden_act="gelu", layer_norm_eps=a.eps, attention_dropout=0.0, attn_implementation="eager")
    m = CLIPVisionModel(c).double().eval()
    v = "visual."
    hf = {"embeddings.class_embedding": sd[v + "class_embedding"],
          "embeddings.patch_embedding.weight": sd[v + "conv1.weight"],
          "embeddings.position_embedding.weight": sd[v + "positional_embedding"],
          "pre_layrnorm.weight": sd[v + "ln_pre.weight"], "pre_layrnorm.bias": sd[v + "ln_pre.bias"],
          # not on the path read here (hidden_states[-1] precedes it); present only for strict loading
          "post_layernorm.weight": torch.ones(a.v_hidden), "post_layernorm.bias": torch.zeros(a.v_hidden)}
    D = a.v_hidden
    for i in range(a.v_layers):
        o, h = f"{v}transformer.resblocks.{i}.", f"encoder.layers.{i}."
        w, b = sd[o + "attn.in_proj_weight"], sd[o + "attn.in_proj_bias"]
        for j, n in enumerate(("q", "k", "v")):
            hf[h + f"self_attn.{n}_proj.weight"] = w[j * D:(j + 1) * D]
            hf[h + f"self_attn.{n}_proj.bias"] = b[j * D:(j + 1) * D]
        hf[h + "self_attn.out_proj.weight"] = sd[o + "attn.out_proj.weight"]
        hf[h + "self_attn.out_proj.bias"] = sd[o + "attn.out_proj.bias"]
        for src, dst in (("ln_1", "layer_norm1"), ("ln_2", "layer_norm2"), ("mlp.c_fc", "mlp.fc1"), ("mlp.c_proj", "mlp.fc2")):
            hf[h + dst + ".weight"] = sd[o + src + ".weight"]
            hf[h + dst + ".bias"] = sd[o + src + ".bias"]
    return _load(m, hf)


class Pooler(nn.Module):
    def __init__(self, a: CocaArch):
        super().__init__()
        E = a.embed_dim
        self.query = nn.Parameter(torch.zeros(a.pool_queries, E))
        self.ln_q, self.ln_k = nn.LayerNorm(E, eps=a.eps), nn.LayerNorm(a.v_hidden, eps=a.eps)
        self.attn = nn.MultiheadAttention(E, a.pool_heads, kdim=a.v_hidden, vdim=a.v_hidden, batch_first=True)
        self.ln_post = nn.LayerNorm(E, eps=a.eps)
        self.proj = nn.Parameter(torch.zeros(E, E))

    def forward(self, x):
        k = self.ln_k(x)
        q = self.ln_q(self.query).unsqueeze(0).expand(x.shape[0], -1, -1)
        out = self.ln_post(self.attn(q, k, k, need_weights=False)[0])
        return out[:, 0] @ self.proj, out[:, 1:]


def pooler(a: CocaArch, sd):
    p = "visual.attn_pool."
    want = {k[len(p):]: t for k, t in sd.items() if k.startswith(p)}
    for n in ("weight", "bias"):
        want[f"ln_post.{n}"] = sd[f"visual.ln_post.{n}"]
    want["proj"] = sd["visual.proj"]
    m = Pooler(a).double().eval()
    if m.attn.in_proj_weight is not None:            # kdim == embed_dim: nn.MultiheadAttention keeps ONE packed in_proj
        want["attn.in_proj_weight"] = torch.cat([want.pop(f"attn.{n}_proj_weight") for n in "qkv"], 0)
    return _load(m, want)


# ------------------------------------------------------------------------------------------------------- text side
def text_model(a: CocaArch, sd):
    from transformers import CLIPTextConfig, CLIPTextModel
    c = CLIPTextConfig(vocab_size=a.vocab + 1, hidden_size=a.t_hidden, intermediate_size=a.t_ffn, num_hidden_layers=a.t_layers,
                       num_attention_heads=a.t_heads, max_position_embeddings=a.context_length + 1, hidden_act="gelu",
                       layer_norm_eps=a.eps, attention_dropout=0.0, attn_implementation="eager", bos_token_id=a.sot,
                       eos_token_id=a.eos, pad_token_id=a.pad)
    m = CLIPTextModel(c).double().eval()
    T = a.t_hidden
    hf = {"embeddings.token_embedding.weight": torch.cat([sd["text.token_embedding.weight"], sd["text.cls_emb"][None]], 0),
          "embeddings.position_embedding.weight": sd["text.positional_embedding"],
          "final_layer_norm.weight": sd["text.ln_final.weight"], "final_layer_norm.bias": sd["text.ln_final.bias"]}
    for i in range(a.t_layers):
        o, h = f"text.transformer.resblocks.{i}.", f"encoder.layers.{i}."
        w, b = sd[o + "attn.in_proj_weight"], sd[o + "attn.in_proj_bias"]
        for j, n in enumerate(("q", "k", "v")):
            hf[h + f"self_attn.{n}_proj.weight"] = w[j * T:(j + 1) * T]
            hf[h + f"self_attn.{n}_proj.bias"] = b[j * T:(j + 1) * T]
        hf[h + "self_attn.out_proj.weight"] = sd[o + "attn.out_proj.weight"]
        hf[h + "self_attn.out_proj.bias"] = sd[o + "attn.out_proj.bias"]
        for src, dst in (("ln_1", "layer_norm1"), ("ln_2", "layer_norm2"), ("mlp.c_fc", "mlp.fc1"), ("mlp.c_proj", "mlp.fc2")):
            hf[h + dst + ".weight"] = sd[o + src + ".weight"]
            hf[h + dst + ".bias"] = sd[o + src + ".bias"]
    sdm = m.state_dict()
    missing = set(sdm) - set(hf)
    assert missing <= {"embeddings.position_ids"}, missing     # a buffer, when the version saves it
    for k in missing:
        hf[k] = sdm[k]
    return _load(m, hf)


def text_tokens(tm, a: CocaArch, text):
    """Per-token outputs of the unimodal tower on `text` (the cls id appended, as open_clip's embed_cls does)."""
    ids = torch.cat([text, torch.full((text.shape[0], 1), a.vocab, dtype=torch.int64)], 1)
    return tm(input_ids=ids, output_hidden_states=True).hidden_states[-1][:, :-1]


class CrossBlock(nn.Module):
    def __init__(self, a: CocaArch):
        super().__init__()
        T = a.t_hidden
        self.ln_1, self.ln_1_kv, self.ln_2 = (nn.LayerNorm(T, eps=a.eps) for _ in range(3))
        self.attn = nn.MultiheadAttention(T, a.t_heads, batch_first=True)
        self.mlp = nn.Sequential()
        self.mlp.add_module("c_fc", nn.Linear(T, a.t_ffn)); self.mlp.add_module("gelu", nn.GELU())
        self.mlp.add_module("c_proj", nn.Linear(a.t_ffn, T))

    def forward(self, x, img):
        kv = self.ln_1_kv(img)
        x = x + self.attn(self.ln_1(x), kv, kv, need_weights=False)[0]
        return x + self.mlp(self.ln_2(x))


class Decoder(nn.Module):
    def __init__(self, a: CocaArch):
        super().__init__()
        T = a.t_hidden
        self.selfs = nn.ModuleList(nn.TransformerEncoderLayer(T, a.t_heads, a.t_ffn, dropout=0.0, activation="gelu", layer_norm_eps=a.eps,
                                                              batch_first=True, norm_first=True) for _ in range(a.mm_layers))
        self.cross = nn.ModuleList(CrossBlock(a) for _ in range(a.mm_layers))
        self.ln_final = nn.LayerNorm(T, eps=a.eps)
        self.text_projection = nn.Parameter(torch.zeros(T, a.vocab))

    def forward(self, x, img):
        n = x.shape[1]
        mask = nn.Transformer.generate_square_subsequent_mask(n, dtype=x.dtype)
        for s, c in zip(self.selfs, self.cross):
            x = c(s(x, src_mask=mask, is_causal=True), img)
        return self.ln_final(x) @ self.text_projection


def decoder(a: CocaArch, sd):
    want = {"ln_final.weight": sd["text_decoder.ln_final.weight"], "ln_final.bias": sd["text_decoder.ln_final.bias"],
            "text_projection": sd["text_decoder.text_projection"]}
    for i in range(a.mm_layers):
        o = f"text_decoder.resblocks.{i}."
        for src, dst in (("attn.in_proj_weight", "self_attn.in_proj_weight"), ("attn.in_proj_bias", "self_attn.in_proj_bias"),
                         ("attn.out_proj.weight", "self_attn.out_proj.weight"), ("attn.out_proj.bias", "self_attn.out_proj.bias"),
                         ("mlp.c_fc.weight", "linear1.weight"), ("mlp.c_fc.bias", "linear1.bias"),
                         ("mlp.c_proj.weight", "linear2.weight"), ("mlp.c_proj.bias", "linear2.bias"),
                         ("ln_1.weight", "norm1.weight"), ("ln_1.bias", "norm1.bias"), ("ln_2.weight", "norm2.weight"), ("ln_2.bias", "norm2.bias")):
            want[f"selfs.{i}.{dst}"] = sd[o + src]
        o = f"text_decoder.cross_attn.{i}."
        for k, t in sd.items():
            if k.startswith(o):
                want[f"cross.{i}.{k[len(o):]}"] = t
    return _load(Decoder(a).double().eval(), want)


def greedy(a: CocaArch, tm, dec, img, seq_len):
    """The top-k(1) loop, whole prefix recomputed each step.  -> (text [B, <= seq_len], per step [B, V] logits with the
    MinLength mask applied, NaN rows where the row had finished)."""
    B = img.shape[0]
    text = torch.full((B, 1), a.sot, dtype=torch.int64)
    steps = []
    while True:
        cur_len = text.shape[1]
        active = ~((text[:, -1] == a.eos) | (text[:, -1] == a.pad))
        if not active.any():
            break
        logits = dec(text_tokens(tm, a, text), img)[:, -1].clone()
        if cur_len < a.min_seq_len:
            logits[:, a.eos] = float("-inf")
        logits[~active] = float("nan")
        steps.append(logits)
        nxt = torch.full((B,), a.pad, dtype=torch.int64)
        nxt[active] = a.eos if cur_len + 1 == seq_len else logits[active].argmax(-1)
        text = torch.cat([text, nxt[:, None]], 1)
        if text.shape[1] >= seq_len:
            break
    return text, torch.stack(steps, 0)


# ----------------------------------------------------------------------------------------------------------- runs
def run(a: CocaArch, seed: int, batch: int, eos_boost: float, decode_len, weights_image_size=None, image=True):
    """weights_image_size: draw the weights for that input size and resize the position table to `a`'s at load.
    image=False: the image-side values are not stored (a second eos_boost of the same weights and pixels)."""
    wa = dataclasses.replace(a, image_size=weights_image_size or a.image_size)
    sd = coca_library_state_dict(procedural_coca_state_dict(wa, seed, eos_boost=eos_boost), a)
    sd = {k: v.double() for k, v in sd.items() if not k.startswith("derived.")}
    px = synthetic_pixels(batch, a.image_size, seed=seed).double()
    import transformers
    out = {}
    with torch.no_grad():
        hs = vision_model(a, sd)(pixel_values=px, output_hidden_states=True).hidden_states
        trunk = hs[-1]
        pooled, tokens = pooler(a, sd)(trunk)
        if image:
            out["trunk_layer_norms"] = torch.stack([h.norm(dim=-1) for h in hs], 0).numpy()      # [v_layers + 1, B, n_tokens]
            out["trunk_stride"], out["trunk_sample"] = _sample(trunk)
            out["tokens_stride"], out["tokens_sample"] = _sample(tokens)
            out["tokens_norm"] = tokens.norm(dim=-1).numpy()
            out["pooled"] = pooled.numpy()
        if decode_len:
            tm, dec = text_model(a, sd), decoder(a, sd)
            text, steps = greedy(a, tm, dec, tokens, decode_len)
            out["sequences"] = text.numpy()
            act = ~torch.isnan(steps[..., 0])                                                     # [S, B]
            fill = torch.where(act[..., None], steps, torch.full_like(steps, float("-inf")))
            t8 = torch.topk(fill, 8, dim=-1)
            out["step_active"] = act.numpy()
            out["step_top8_ids"] = np.where(act[..., None].numpy(), t8.indices.numpy(), -1).astype(np.int32)
            out["step_top8_vals"] = np.where(act[..., None].numpy(), t8.values.numpy(), 0.0)       # 0 / -1 where inactive
            out["step_logsumexp"] = np.where(act.numpy(), torch.logsumexp(fill, -1).numpy(), 0.0)
            out["step_margin"] = np.where(act.numpy(), (t8.values[..., 0] - t8.values[..., 1]).numpy(), 0.0)
            # the unimodal tower on the final sequences (the prefix of every step is a prefix of these, causally the same)
            tt = text_tokens(tm, a, text)
            out["text_stride"], out["text_sample"] = _sample(tt)
            out["text_norm"] = tt.norm(dim=-1).numpy()
            print("sequences", text.tolist())
    out["meta"] = np.array(json.dumps(dict(seed=seed, batch=batch, eos_boost=eos_boost, arch=dataclasses.asdict(a),
                                           decode_len=decode_len, weights_image_size=wa.image_size, transformers=transformers.__version__)))
    return out


def width_arch() -> CocaArch:
    """Production widths of coca_ViT-L-14 (1024 / 16 heads / patch 14 vision at 224 px, 768 / 12 heads text, vocab 49408),
    two layers per tower."""
    return dataclasses.replace(CocaArch(), v_layers=2, t_layers=2, mm_layers=2)


def fixtures():
    tiny = CocaArch.tiny()
    l14 = dataclasses.replace(CocaArch(), seq_len=8, min_seq_len=3)
    a336 = dataclasses.replace(CocaArch(), image_size=336)
    return {
        # eos_boost 0: rows of full length; eos_boost 4: early EOS and pad
        "coca_tiny": lambda: (run(tiny, 1, 4, 0.0, tiny.seq_len), run(tiny, 1, 4, 4.0, tiny.seq_len, image=False)),
        "coca_width": lambda: run(width_arch(), 2, 2, 2.0, width_arch().seq_len),
        "coca_l14_image": lambda: run(l14, 0, 2, 2.0, l14.seq_len),
        # the position table of a 224-pixel checkpoint resized to 577 rows at load (coca_library_state_dict)
        "coca_l14_336_image": lambda: run(a336, 0, 1, 0.0, None, weights_image_size=224),
    }


def main():
    torch.manual_seed(0)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    gold = os.path.join(ROOT, "tests", "golden")
    todo = fixtures()
    names = [n for n in sys.argv[1:] if not n.startswith("-")] or list(todo)
    for name in names:
        r = todo[name]()
        if isinstance(r, tuple):                          # coca_tiny: one file, an eos_boost 0 part and an eos_boost 4 part
            r = {f"{p}_{k}": v for p, part in zip(("b0", "b4"), r) for k, v in part.items()}
        path = os.path.join(gold, name + ".npz")
        np.savez_compressed(path, **r)
        print(name, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
