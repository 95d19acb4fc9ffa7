"""Architecture constants of the captioner forward path.

BLIP-base values follow the HF config defaults the checkpoint's ``config.json``
overrides at load time (HF:models/blip/configuration_blip.py:52-107; SURVEY.md §8
"Model constants").  CoCa values follow the reference's
``experimenting_env/captioner/models/coca/model_configs/coca_ViT-L-14.json:1-30``.
"""
from __future__ import annotations

import dataclasses
import json
import os


@dataclasses.dataclass
class BlipArch:
    # vision tower (ViT-B/16)
    image_size: int = 224
    patch_size: int = 16
    v_hidden: int = 768
    v_layers: int = 12
    v_heads: int = 12
    v_mlp: int = 3072
    v_eps: float = 1e-5
    # text decoder (BERT-style, post-LN, cross-attention to image tokens)
    t_hidden: int = 768
    t_layers: int = 12
    t_heads: int = 12
    t_ffn: int = 3072
    vocab: int = 30524
    max_pos: int = 512
    t_eps: float = 1e-12
    bos: int = 30522
    eos: int = 102      # sep_token_id: what BlipForConditionalGeneration.generate passes as eos
    pad: int = 0

    @property
    def grid(self) -> int:
        return self.image_size // self.patch_size

    @property
    def n_patches(self) -> int:
        return self.grid * self.grid

    @property
    def n_tokens(self) -> int:
        return self.n_patches + 1

    @property
    def v_head_dim(self) -> int:
        return self.v_hidden // self.v_heads

    @property
    def t_head_dim(self) -> int:
        return self.t_hidden // self.t_heads

    def encoder_flops_per_image(self) -> float:
        """2*MAC of patch-embed + 12x(QKV, QK^T, PV, proj, FC1, FC2); BASELINE.md §4."""
        n, d, m = self.n_tokens, self.v_hidden, self.v_mlp
        per_layer = 2.0 * n * d * 3 * d + 2 * 2.0 * n * n * d + 2.0 * n * d * d + 2 * 2.0 * n * d * m
        patch = 2.0 * self.n_patches * (3 * self.patch_size ** 2) * d
        return per_layer * self.v_layers + patch

    def cross_kv_flops_per_image(self) -> float:
        return self.t_layers * 2 * 2.0 * self.n_tokens * self.v_hidden * self.t_hidden

    def decode_flops_per_token(self) -> float:
        d, f, v = self.t_hidden, self.t_ffn, self.vocab
        per_layer = 2.0 * d * d * 4 + 2.0 * d * d * 2 + 2 * 2.0 * d * f   # self q,k,v,o + cross q,o + ffn
        return per_layer * self.t_layers + 2.0 * d * d + 2.0 * d * v

    @staticmethod
    def tiny() -> "BlipArch":
        """Fixture-sized config (tests/golden/blip_tiny*.npz): hidden 128 (2 heads of 64), 2 layers, vocab 512,
        32x32 image with 8x8 patches (17 tokens)."""
        return BlipArch(image_size=32, patch_size=8, v_hidden=128, v_layers=2, v_heads=2, v_mlp=256,
                        t_hidden=128, t_layers=2, t_heads=2, t_ffn=256, vocab=512, max_pos=40,
                        bos=510, eos=102, pad=0)

    @staticmethod
    def from_hf_config(path_or_dict) -> "BlipArch":
        """Read a HF ``config.json`` (checkpoint directory or parsed dict)."""
        if isinstance(path_or_dict, (str, os.PathLike)):
            p = path_or_dict
            if os.path.isdir(p):
                p = os.path.join(p, "config.json")
            with open(p) as f:
                cfg = json.load(f)
        else:
            cfg = dict(path_or_dict)
        v = cfg.get("vision_config", {})
        t = cfg.get("text_config", {})
        a = BlipArch()
        a.image_size = v.get("image_size", 384)
        a.patch_size = v.get("patch_size", 16)
        a.v_hidden = v.get("hidden_size", 768)
        a.v_layers = v.get("num_hidden_layers", 12)
        a.v_heads = v.get("num_attention_heads", 12)
        a.v_mlp = v.get("intermediate_size", 3072)
        a.v_eps = v.get("layer_norm_eps", 1e-5)
        a.t_hidden = t.get("hidden_size", 768)
        a.t_layers = t.get("num_hidden_layers", 12)
        a.t_heads = t.get("num_attention_heads", 8)
        a.t_ffn = t.get("intermediate_size", 3072)
        a.vocab = t.get("vocab_size", 30524)
        a.max_pos = t.get("max_position_embeddings", 512)
        a.t_eps = t.get("layer_norm_eps", 1e-12)
        a.bos = t.get("bos_token_id", 30522)
        a.eos = t.get("sep_token_id", 102)
        a.pad = t.get("pad_token_id", 0)
        return a


@dataclasses.dataclass
class CocaArch:
    """CoCa ViT-L/14 - reference ``experimenting_env/captioner/models/coca/model_configs/coca_ViT-L-14.json:1-30``
    (+ open_clip defaults: 256 pooler queries, mlp_ratio 4, LayerNorm eps 1e-5, exact GELU)."""
    image_size: int = 224
    patch_size: int = 14
    v_hidden: int = 1024
    v_layers: int = 24
    v_heads: int = 16
    v_mlp: int = 4096
    embed_dim: int = 768          # pooler output width = text width
    pool_queries: int = 256
    pool_heads: int = 8
    t_hidden: int = 768
    t_layers: int = 12            # unimodal text tower
    mm_layers: int = 12           # multimodal decoder (each layer = causal self-attn block + cross-attn block)
    t_heads: int = 12
    t_ffn: int = 3072
    vocab: int = 49408
    context_length: int = 76
    eps: float = 1e-5
    sot: int = 49406
    eos: int = 49407
    pad: int = 0
    seq_len: int = 30             # coca_model.py:209 generate defaults
    min_seq_len: int = 5

    @property
    def grid(self) -> int:
        return self.image_size // self.patch_size

    @property
    def n_tokens(self) -> int:
        return self.grid * self.grid + 1

    @property
    def n_image_embs(self) -> int:
        return self.pool_queries - 1

    @staticmethod
    def tiny() -> "CocaArch":
        return CocaArch(image_size=28, patch_size=14, v_hidden=128, v_layers=2, v_heads=2, v_mlp=256, embed_dim=128,
                        pool_queries=8, pool_heads=2, t_hidden=128, t_layers=2, mm_layers=2, t_heads=2, t_ffn=256,
                        vocab=512, context_length=20, sot=510, eos=511, pad=0, seq_len=12, min_seq_len=3)


@dataclasses.dataclass
class MiniLMArch:
    """sentence-transformers/all-MiniLM-L6-v2 (the caption embedder of the reference: goal_exploration.py:57,
    pseudolabeler.py:568): HF BertModel 6 x 384, 12 heads of 32, FFN 1536, post-LN eps 1e-12, WordPiece vocab 30522,
    then mean pooling over the attention mask and L2 normalisation -> 384-d."""
    hidden: int = 384
    layers: int = 6
    heads: int = 12
    ffn: int = 1536
    vocab: int = 30522
    max_pos: int = 512
    eps: float = 1e-12
    cls: int = 101
    sep: int = 102
    pad: int = 0
    max_seq_length: int = 256      # sentence-transformers truncation for this model

    @staticmethod
    def tiny() -> "MiniLMArch":
        return MiniLMArch(hidden=64, layers=2, heads=2, ffn=128, vocab=300, max_pos=40, cls=1, sep=2, pad=0,
                          max_seq_length=32)


@dataclasses.dataclass
class Blip2Arch:
    """BLIP-2 OPT (reference `captioner/models/blip2/blip2.py:19-22`: `Salesforce/blip2-opt-2.7b`) - HF defaults of
    `HF:models/blip_2/configuration_blip_2.py` for the vision tower (ViT-g/14: 39 x 1408, 16 heads of 88) and the
    Q-Former (12 x 768, 32 queries, cross-attention every 2nd layer), `facebook/opt-2.7b` for the language model
    (32 x 2560, 32 heads of 80, FFN 10240, ReLU, pre-LN, learned positions with offset 2, tied LM head)."""
    image_size: int = 224
    patch_size: int = 14
    v_hidden: int = 1408
    v_layers: int = 39
    v_heads: int = 16
    v_mlp: int = 6144
    v_eps: float = 1e-6
    q_hidden: int = 768
    q_layers: int = 12
    q_heads: int = 12
    q_ffn: int = 3072
    q_cross_freq: int = 2
    q_eps: float = 1e-12
    num_query_tokens: int = 32
    t_hidden: int = 2560
    t_layers: int = 32
    t_heads: int = 32
    t_ffn: int = 10240
    vocab: int = 50272
    max_pos: int = 2048
    t_eps: float = 1e-5
    bos: int = 2
    eos: int = 50118          # generation_config of blip2-opt-2.7b ("\n"); OPT's own eos is 2
    pad: int = 1
    image_token: int = 50265
    max_new_tokens: int = 20  # HF generate default when the caller gives no length (blip2.py:26 gives none)

    @property
    def n_patches(self) -> int:
        return (self.image_size // self.patch_size) ** 2

    @property
    def n_tokens(self) -> int:
        return self.n_patches + 1

    @staticmethod
    def tiny() -> "Blip2Arch":
        # head dims of the real model's kinds: vision 24 (not a power of two, like 88), q-former 64, language model 16
        return Blip2Arch(image_size=28, patch_size=14, v_hidden=192, v_layers=2, v_heads=8, v_mlp=256, q_hidden=128, q_layers=2,
                         q_heads=2, q_ffn=256, num_query_tokens=8, t_hidden=64, t_layers=2, t_heads=4, t_ffn=128, vocab=512,
                         max_pos=64, eos=3, image_token=511)

    @staticmethod
    def small() -> "Blip2Arch":
        # the fixture geometry with OPT widths the int8 weight stream takes (`load_in_8bit`: multiples of 256)
        return Blip2Arch(image_size=28, patch_size=14, v_hidden=192, v_layers=2, v_heads=8, v_mlp=256, q_hidden=128, q_layers=2,
                         q_heads=2, q_ffn=256, num_query_tokens=8, t_hidden=256, t_layers=2, t_heads=4, t_ffn=512, vocab=512,
                         max_pos=64, eos=3, image_token=511)


@dataclasses.dataclass
class Blip2ItmArch:
    """BLIP-2 image-text matching / contrastive scorer, HF `Blip2ForImageTextRetrieval` (the port of the LAVIS
    `blip2_image_text_matching` model behind the reference's `--method blip2_itm | blip2_itc`,
    experimenting_env/captioner/pseudocaptioner.py:34-37).  Defaults = `Salesforce/blip2-itm-vit-g`: ViT-g/14 at 224 px (39 x 1408,
    16 heads of 88), Q-Former 12 x 768 (12 heads, 32 queries, cross-attention every 2nd layer) WITH its text side (BERT word /
    position embeddings, vocabulary 30523, 512 positions), projections to 256.  `...-vit-g-coco` is the same at 364 px."""
    image_size: int = 224
    patch_size: int = 14
    v_hidden: int = 1408
    v_layers: int = 39
    v_heads: int = 16
    v_mlp: int = 6144
    v_eps: float = 1e-6
    q_hidden: int = 768
    q_layers: int = 12
    q_heads: int = 12
    q_ffn: int = 3072
    q_cross_freq: int = 2
    q_eps: float = 1e-12
    num_query_tokens: int = 32
    vocab: int = 30523
    max_pos: int = 512
    pad: int = 0
    projection_dim: int = 256
    max_text_len: int = 32        # the reference's tokenizer call: truncation=True, max_length=32 (:292)

    @property
    def n_patches(self) -> int:
        return (self.image_size // self.patch_size) ** 2

    @property
    def n_tokens(self) -> int:
        return self.n_patches + 1

    @staticmethod
    def tiny() -> "Blip2ItmArch":
        """Fixture-sized config (tests/golden/blip2_itm_tiny.npz): the tiny BLIP-2 tower (28 px, 5 tokens, heads of 24) and Q-Former
        (2 x 128, heads of 64, 8 queries), vocabulary 300, 40 positions, projection 64."""
        return Blip2ItmArch(image_size=28, patch_size=14, v_hidden=192, v_layers=2, v_heads=8, v_mlp=256, q_hidden=128, q_layers=2,
                            q_heads=2, q_ffn=256, num_query_tokens=8, vocab=300, max_pos=40, projection_dim=64)

    @staticmethod
    def width(image_size: int = 224) -> "Blip2ItmArch":
        """Production widths with two layers per tower (tests/golden/blip2_itm_width.npz)."""
        return Blip2ItmArch(image_size=image_size, v_layers=2, q_layers=2)

    def hf_config_dict(self) -> dict:
        """The `Blip2Config` of this arch (what `from_hf_config` reads back)."""
        return dict(
            num_query_tokens=self.num_query_tokens, image_text_hidden_size=self.projection_dim, image_token_index=None,
            vision_config=dict(hidden_size=self.v_hidden, num_hidden_layers=self.v_layers, num_attention_heads=self.v_heads,
                               intermediate_size=self.v_mlp, image_size=self.image_size, patch_size=self.patch_size,
                               layer_norm_eps=self.v_eps, hidden_act="gelu", qkv_bias=True),
            qformer_config=dict(hidden_size=self.q_hidden, num_hidden_layers=self.q_layers, num_attention_heads=self.q_heads,
                                intermediate_size=self.q_ffn, cross_attention_frequency=self.q_cross_freq, layer_norm_eps=self.q_eps,
                                encoder_hidden_size=self.v_hidden, vocab_size=self.vocab, max_position_embeddings=self.max_pos,
                                pad_token_id=self.pad, hidden_act="gelu", use_qformer_text_input=True))

    @staticmethod
    def from_hf_config(path_or_dict) -> "Blip2ItmArch":
        """Read a HF `Blip2Config` ``config.json`` (checkpoint directory, file or parsed dict) of an image-text retrieval
        checkpoint: `qformer_config.use_qformer_text_input` must be true and `image_token_index` absent."""
        if isinstance(path_or_dict, (str, os.PathLike)):
            p = path_or_dict
            if os.path.isdir(p):
                p = os.path.join(p, "config.json")
            with open(p) as f:
                cfg = json.load(f)
        else:
            cfg = dict(path_or_dict)
        v = cfg.get("vision_config") or {}
        q = cfg.get("qformer_config") or {}
        d = Blip2ItmArch()
        if not q.get("use_qformer_text_input", False):
            raise ValueError("this BLIP-2 checkpoint has no Q-Former text side (qformer_config.use_qformer_text_input is false): "
                             "it is a captioning checkpoint, not an image-text matching one")
        if cfg.get("image_token_index") is not None:
            raise ValueError("BLIP-2 checkpoints with image placeholder ids (image_token_index) are not supported by the scorer")
        for name, c in (("vision_config", v), ("qformer_config", q)):
            if c.get("hidden_act", "gelu") != "gelu":
                raise ValueError(f"{name}.hidden_act {c.get('hidden_act')!r} is not supported (the towers run exact gelu)")
        if not v.get("qkv_bias", True):
            raise ValueError("vision_config.qkv_bias = false is not supported")
        if q.get("encoder_hidden_size", v.get("hidden_size", d.v_hidden)) != v.get("hidden_size", d.v_hidden):
            raise ValueError("qformer_config.encoder_hidden_size differs from the vision tower's width")
        return Blip2ItmArch(
            image_size=v.get("image_size", d.image_size), patch_size=v.get("patch_size", d.patch_size),
            v_hidden=v.get("hidden_size", d.v_hidden), v_layers=v.get("num_hidden_layers", d.v_layers),
            v_heads=v.get("num_attention_heads", d.v_heads), v_mlp=v.get("intermediate_size", d.v_mlp),
            v_eps=v.get("layer_norm_eps", d.v_eps),
            q_hidden=q.get("hidden_size", d.q_hidden), q_layers=q.get("num_hidden_layers", d.q_layers),
            q_heads=q.get("num_attention_heads", d.q_heads), q_ffn=q.get("intermediate_size", d.q_ffn),
            q_cross_freq=q.get("cross_attention_frequency", d.q_cross_freq), q_eps=q.get("layer_norm_eps", d.q_eps),
            num_query_tokens=cfg.get("num_query_tokens", d.num_query_tokens), vocab=q.get("vocab_size", 30522),
            max_pos=q.get("max_position_embeddings", d.max_pos), pad=q.get("pad_token_id", d.pad),
            projection_dim=cfg.get("image_text_hidden_size", d.projection_dim))


@dataclasses.dataclass
class ClipArch:
    """HF `CLIPModel` (the reference's `--method clip` scorer: `openai/clip-vit-base-patch32`,
    experimenting_env/captioner/pseudocaptioner.py:39-46).  Defaults = ViT-B/32: a 224 px image tower of 12 x 768 (12 heads,
    MLP 3072, patch 32: 50 tokens), a causal text tower of 12 x 512 (8 heads, FFN 2048, 77 positions, vocab 49408), both
    projected to 512; pre-LN, eps 1e-5, quick GELU.  `eos_token_id` decides the pooled text row (HF's rule): 2 (the legacy
    OpenAI configs) pools at argmax(ids), anything else at the first `eos_token_id`."""
    image_size: int = 224
    patch_size: int = 32
    v_hidden: int = 768
    v_layers: int = 12
    v_heads: int = 12
    v_mlp: int = 3072
    t_hidden: int = 512
    t_layers: int = 12
    t_heads: int = 8
    t_ffn: int = 2048
    vocab: int = 49408
    max_pos: int = 77
    projection_dim: int = 512
    eps: float = 1e-5
    hidden_act: str = "quick_gelu"
    bos_token_id: int = 49406
    eos_token_id: int = 49407
    pad_token_id: int = 1

    ACTS = ("quick_gelu", "gelu")

    def __post_init__(self):
        if self.hidden_act not in self.ACTS:
            raise ValueError(f"CLIP hidden_act {self.hidden_act!r} is not supported (the towers run {' / '.join(self.ACTS)})")

    @property
    def grid(self) -> int:
        return self.image_size // self.patch_size

    @property
    def n_tokens(self) -> int:
        return self.grid * self.grid + 1

    def image_flops(self) -> float:
        """2*MAC per image: patch GEMM + per layer q|k|v, QK^T, PV, out_proj, fc1, fc2 (+ the head)."""
        n, d, m = self.n_tokens, self.v_hidden, self.v_mlp
        per_layer = 2.0 * n * d * 3 * d + 2 * 2.0 * n * n * d + 2.0 * n * d * d + 2 * 2.0 * n * d * m
        patch = 2.0 * (n - 1) * (3 * self.patch_size ** 2) * d
        return per_layer * self.v_layers + patch + 2.0 * d * self.projection_dim

    def text_flops_per_token(self) -> float:
        """2*MAC per caption token of the text tower's GEMMs (attention excluded: it is O(L) per token)."""
        t, f = self.t_hidden, self.t_ffn
        return self.t_layers * (2.0 * t * 3 * t + 2.0 * t * t + 2 * 2.0 * t * f)

    @staticmethod
    def tiny() -> "ClipArch":
        """Fixture-sized config (tests/golden/clip_tiny.npz): 32 px images with 8 px patches (17 tokens), both towers 2 x 128
        (heads of 64), vocab 300, 16 positions, projection 64."""
        return ClipArch(image_size=32, patch_size=8, v_hidden=128, v_layers=2, v_heads=2, v_mlp=256, t_hidden=128, t_layers=2,
                        t_heads=2, t_ffn=256, vocab=300, max_pos=16, projection_dim=64, bos_token_id=298, eos_token_id=299,
                        pad_token_id=0)

    @staticmethod
    def from_hf_config(path_or_dict) -> "ClipArch":
        """Read a HF `CLIPConfig` ``config.json`` (checkpoint directory, file or parsed dict)."""
        if isinstance(path_or_dict, (str, os.PathLike)):
            p = path_or_dict
            if os.path.isdir(p):
                p = os.path.join(p, "config.json")
            with open(p) as f:
                cfg = json.load(f)
        else:
            cfg = dict(path_or_dict)
        v = cfg.get("vision_config") or {}
        t = cfg.get("text_config") or {}
        d = ClipArch()
        acts = {v.get("hidden_act", d.hidden_act), t.get("hidden_act", d.hidden_act)}
        if len(acts) != 1:
            raise ValueError(f"CLIP towers with different activations {sorted(acts)} are not supported")
        return ClipArch(
            image_size=v.get("image_size", d.image_size), patch_size=v.get("patch_size", d.patch_size),
            v_hidden=v.get("hidden_size", d.v_hidden), v_layers=v.get("num_hidden_layers", d.v_layers),
            v_heads=v.get("num_attention_heads", d.v_heads), v_mlp=v.get("intermediate_size", d.v_mlp),
            t_hidden=t.get("hidden_size", d.t_hidden), t_layers=t.get("num_hidden_layers", d.t_layers),
            t_heads=t.get("num_attention_heads", d.t_heads), t_ffn=t.get("intermediate_size", d.t_ffn),
            vocab=t.get("vocab_size", d.vocab), max_pos=t.get("max_position_embeddings", d.max_pos),
            projection_dim=cfg.get("projection_dim", d.projection_dim),
            eps=v.get("layer_norm_eps", t.get("layer_norm_eps", d.eps)), hidden_act=acts.pop(),
            bos_token_id=t.get("bos_token_id", d.bos_token_id), eos_token_id=t.get("eos_token_id", d.eos_token_id),
            pad_token_id=t.get("pad_token_id", d.pad_token_id))
