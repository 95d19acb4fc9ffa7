"""CPU: the CLIP scorer's host side - the float64 HF goldens, config / checkpoint loading, tokenisation and the pooled-row rule,
HF's shortest-edge crop geometry, and the pseudo-caption driver with a stub scorer."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _tool():
    spec = importlib.util.spec_from_file_location("make_goldens_clip", os.path.join(ROOT, "tools", "make_goldens_clip.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("name", ["clip_tiny", "clip_b32"])
def test_goldens_reproduce_from_hf_clipmodel(name):
    pytest.importorskip("transformers")
    g = np.load(os.path.join(GOLDEN, f"{name}.npz"))
    res = _tool().compute(name)
    for k in ("ids", "lens", "group_images", "group_captions", "group_rank"):
        assert np.array_equal(res[k], g[k]), k
    for k in ("image_embeds", "text_embeds", "logits_per_image", "group_margin"):
        assert np.abs(res[k] - g[k]).max() < 1e-9, k
    if "frames" in g:
        assert np.array_equal(res["frames"], g["frames"])
    # the fixture's pooled rows are HF's: first <eot> (eos_token_id != 2)
    from embodied_captioning_amd.captioner.clip_scorer import pooled_positions
    from embodied_captioning_amd.config import ClipArch
    a = ClipArch.tiny() if name == "clip_tiny" else ClipArch()
    assert [p + 1 for p in pooled_positions(g["ids"], a.eos_token_id)] == g["lens"].tolist()


def test_arch_from_hf_config_round_trip_and_checkpoint_dir(tmp_path):
    transformers = pytest.importorskip("transformers")
    from embodied_captioning_amd.config import ClipArch
    from embodied_captioning_amd.weights import clip_param_specs, load_hf_clip_checkpoint, procedural_clip_state_dict
    t = _tool()
    for a in (ClipArch(), ClipArch.tiny(), ClipArch(hidden_act="gelu", eos_token_id=2)):
        cfg = transformers.CLIPConfig(**t.hf_config_dict(a))
        assert ClipArch.from_hf_config(cfg.to_dict()) == a
    with pytest.raises(ValueError, match="gelu_new"):
        ClipArch(hidden_act="gelu_new")
    d = t.hf_config_dict(ClipArch.tiny())
    d["vision_config"]["hidden_act"] = "relu"
    d["text_config"]["hidden_act"] = "relu"
    with pytest.raises(ValueError, match="relu"):
        ClipArch.from_hf_config(d)
    # save_pretrained of procedural weights loads back with every key accounted for
    a = ClipArch.tiny()
    m = t.hf_model(a, 4, dtype=torch.float32)
    m.save_pretrained(str(tmp_path))
    arch, sd = load_hf_clip_checkpoint(str(tmp_path))
    assert arch == a
    want = procedural_clip_state_dict(a, 4)
    extra = {"vision_model.embeddings.patch_embedding.bias"}
    assert set(sd) == set(want) | extra
    assert {n for n, *_ in clip_param_specs(a)} | {"logit_scale"} == set(want)
    for k, v in want.items():
        assert torch.equal(sd[k].float().reshape(v.shape), v), k
    assert not sd["vision_model.embeddings.patch_embedding.bias"].any()


def _toy_tokenizer(tmp_path, eos_token_id):
    transformers = pytest.importorskip("transformers")
    from embodied_captioning_amd.captioner.clip_bpe import vocab_from_merges
    merges = [("t", "h"), ("th", "e</w>"), ("c", "a"), ("ca", "t</w>"), ("s", "a"), ("sa", "t</w>"), ("o", "n</w>"), ("m", "a"),
              ("ma", "t</w>")]
    vocab = vocab_from_merges(merges, ("<|startoftext|>", "<|endoftext|>"))
    sid = {s: i for i, s in enumerate(vocab)}
    tok = transformers.CLIPTokenizer(vocab=sid, merges=[tuple(m) for m in merges])
    return tok, sid


@pytest.mark.parametrize("legacy", [False, True])
def test_tokenisation_and_pooled_rule_match_hf(tmp_path, legacy):
    transformers = pytest.importorskip("transformers")
    from embodied_captioning_amd.captioner.clip_scorer import pooled_positions, tokenize_captions
    tok, sid = _toy_tokenizer(tmp_path, None)
    eot = sid["<|endoftext|>"]
    caps = ["the cat", "the cat sat on the mat", "a", "mat"]
    rows = tokenize_captions(tok, caps, 77)
    assert rows == [tok(c)["input_ids"] for c in caps]
    assert all(r[0] == sid["<|startoftext|>"] and r[-1] == eot for r in rows)
    with pytest.raises(ValueError, match="the cat sat"):
        tokenize_captions(tok, ["the cat sat on the mat " * 20], 77)
    with pytest.raises(TypeError):
        tokenize_captions(None, ["the cat"], 77)
    # HF's pooled row on the padded batch (the tokenizer pads with <eot>): a tiny text model's pooler_output is that row
    eos = 2 if legacy else eot
    cfg = transformers.CLIPTextConfig(vocab_size=len(sid), hidden_size=32, intermediate_size=64, num_hidden_layers=1,
                                      num_attention_heads=2, max_position_embeddings=77, eos_token_id=eos)
    model = transformers.CLIPTextModel(cfg).eval()
    batch = tok(caps, padding=True, return_tensors="pt")
    with torch.no_grad():
        out = model(input_ids=batch["input_ids"])
    pos = pooled_positions(batch["input_ids"].tolist(), eos)
    assert pos == [len(r) - 1 for r in rows]
    assert torch.equal(out.pooler_output, out.last_hidden_state[torch.arange(len(caps)), torch.tensor(pos)])


def test_text_batches_are_padded_per_chunk_and_lens_end_at_the_pooled_row():
    """`get_text_features` through a stub engine: rows go in chunks of batch_size, each padded (shared `pad_rows`) to ITS longest row
    with the pad id, and lens are pooled position + 1 - not the row length, which a row with ids behind its <eot> shows."""
    from embodied_captioning_amd.captioner.clip_scorer import ClipScorer
    from embodied_captioning_amd.config import ClipArch

    class Engine:
        calls = []

        def embed_text(self, ids, lens):
            self.calls.append((ids.clone(), lens.clone()))
            return torch.zeros((ids.shape[0], 4))

    arch = ClipArch.tiny()
    sot, eot, pad = arch.bos_token_id, arch.eos_token_id, arch.pad_token_id
    assert eot != 2                                    # not the legacy argmax rule: the FIRST <eot> pools
    rows = [[sot, 5, 6, eot], [sot, 7, eot, 9, 9, 9], [sot, eot], [sot, 5, 6, 7, 8, eot], [sot, 5, eot]]
    sc = object.__new__(ClipScorer)
    sc.arch, sc.tokenizer, sc.batch_size, sc.device, sc.engine = arch, None, 2, torch.device("cpu"), Engine()
    assert sc.get_text_features(rows).shape == (5, 4)
    assert [tuple(i.shape) for i, _ in Engine.calls] == [(2, 6), (2, 6), (1, 3)]
    assert [ln.tolist() for _, ln in Engine.calls] == [[4, 3], [2, 6], [3]]
    for (ids, lens), chunk in zip(Engine.calls, (rows[0:2], rows[2:4], rows[4:5])):
        assert ids.dtype == lens.dtype == torch.int32
        for b, r in enumerate(chunk):
            assert ids[b].tolist() == r + [pad] * (ids.shape[1] - len(r))
    assert sc.get_text_features([]).shape == (0, arch.projection_dim)


def test_hf_shortest_edge_geometry_matches_clip_image_processor():
    transformers = pytest.importorskip("transformers")
    from PIL import Image
    from embodied_captioning_amd.preprocess import hf_shortest_edge_geometry, shorter_side_geometry
    proc = transformers.CLIPImageProcessorPil(do_normalize=False, do_rescale=False, do_convert_rgb=True)
    S = 224
    rng = np.random.default_rng(0)
    differs = 0
    for w, h in [(37, 91), (91, 37), (224, 224), (225, 224), (223, 300), (300, 223), (17, 1001), (640, 481), (481, 640), (99, 100),
                 (333, 777), (1280, 721)]:
        a = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        nw, nh, left, top = hf_shortest_edge_geometry(w, h, S)
        ours = np.asarray(Image.fromarray(a).resize((nw, nh), Image.BICUBIC))[top:top + S, left:left + S]
        ref = proc(images=Image.fromarray(a), return_tensors="np")["pixel_values"][0].transpose(1, 2, 0)
        assert ours.shape == ref.shape == (S, S, 3), (w, h)
        assert np.array_equal(ours.astype(np.float32), ref.astype(np.float32)), (w, h)
        differs += hf_shortest_edge_geometry(w, h, S) != shorter_side_geometry(w, h, S)
    assert differs > 0                     # truncated, not rounded: the open_clip geometry is a different function


class _StubScorer:
    """Score = the image's mean red value // 10 (the crop's BGR -> RGB swap shows), ties by construction."""

    def __init__(self):
        self.calls = []

    def score_pairs(self, images, captions):
        self.calls.append((len(images), [c.shape for c in images], list(captions)))
        return [float(c[..., 0].mean()) // 10 for c in images]


def _frame(h, w, red):
    f = np.zeros((h, w, 3), dtype=np.uint8)
    f[..., 2] = red                        # BGR: channel 2 is red
    return f


def test_clip_pseudo_captions_stub_sorting_ties_json_and_clamping(tmp_path):
    from embodied_captioning_amd.pseudocaptioner import clip_pseudo_captions, crop_rect, host_crops
    fa, fb = _frame(480, 640, 200), _frame(720, 1280, 50)
    grouped = {
        (0, 1): [{"image": fa, "pred_box": np.array([10, 10, 100, 100], np.float32), "caption": "low"},
                 {"image": fb, "pred_box": np.array([0, 0, 50, 50], np.float32), "caption": "a"},
                 {"image": fb, "pred_box": np.array([5, 5, 60, 60], np.float32), "caption": "b"},
                 {"image": fa, "pred_box": np.array([20, 20, 40, 40], np.float32), "caption": "high"}],
        (0, 2): [{"image": fb, "pred_box": np.array([1200, 700, 1279, 719], np.float32), "caption": "edge"}],
    }
    stub = _StubScorer()
    out = clip_pseudo_captions(grouped, stub, crop=host_crops)
    assert len(stub.calls) == 1 and stub.calls[0][0] == 5              # one batched call for every pair of every group
    assert stub.calls[0][2] == ["low", "a", "b", "high", "edge"]       # images handed back in pair order (crops are frame-major)
    assert [s[:2] for s in stub.calls[0][1][:4]] == [(108, 108), (55, 55), (65, 65), (24, 24)]
    g = out[str((0, 1))]
    # scores 20, 5, 5, 20 -> sorted descending, equal scores keep input order
    assert [c for _, c in g["captions_list"]] == ["low", "high", "a", "b"]
    assert g["pseudocaption"] == g["captions_list"][0]
    json.loads(json.dumps(out))
    assert set(out) == {"(0, 1)", "(0, 2)"} and set(g) == {"captions_list", "pseudocaption"}
    # expand_box against the hard-coded (1280, 1280), then the numpy slice clamps to the real 1280 x 720 frame
    r = crop_rect(np.array([1200, 700, 1279, 719], np.float32), fb.shape)
    assert r == (1192, 698, 1280, 720)
    assert stub.calls[0][1][4] == (720 - 698, 1280 - 1192, 3)


def test_group_records_filter_and_refused_methods(tmp_path):
    from embodied_captioning_amd import pseudocaptioner as P
    from embodied_captioning_amd.pseudolabeler import record_name, save_record
    img = _frame(64, 96, 10)
    inst = {"captions": ["a red chair", "a man running", "a lamp"],
            "pred_boxes": [np.array([1, 2, 30, 40], np.float32)] * 3,
            "infos": [{"id_episode": 3, "id_object": 1}, {"id_episode": 3, "id_object": 1}, {"id_episode": 3, "id_object": 2}]}
    f = save_record(str(tmp_path), record_name(3, 5)[:-4], inst, img)
    g = P.group_records([f])
    assert list(g) == [(3, 1), (3, 2)]
    assert [d["caption"] for d in g[(3, 1)]] == ["a red chair"]      # "running" is a banned word
    assert g[(3, 1)][0]["filename"] == f and np.array_equal(g[(3, 1)][0]["image"], img)
    for m in P.REFUSED_METHODS:
        with pytest.raises(SystemExit, match=m):
            P.main(["--file_path", str(tmp_path), "--output_csv_path", str(tmp_path / "o.json"), "--method", m])
