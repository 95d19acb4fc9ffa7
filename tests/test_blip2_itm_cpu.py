"""CPU: the BLIP-2 image-text scorer's host side - the float64 HF goldens (`Blip2ForImageTextRetrieval` on procedural weights),
config / checkpoint loading, the reference's tokenisation (truncation at 32), and the pseudo-caption driver with a stub scorer."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _tool():
    spec = importlib.util.spec_from_file_location("make_goldens_blip2_itm", os.path.join(ROOT, "tools", "make_goldens_blip2_itm.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("name", ["blip2_itm_tiny", "blip2_itm_width"])
def test_goldens_reproduce_from_hf_blip2_image_text_retrieval(name):
    import transformers  # noqa: F401  (the float64 HF model is the oracle: its absence is a failure, not a skip)
    t = _tool()
    g = np.load(os.path.join(GOLDEN, f"{name}.npz"))
    res = t.compute(name)
    assert set(res) == set(g.files)
    prefixes = ("", "s364_") if name == "blip2_itm_width" else ("",)
    for pre in prefixes:
        for k in t.INT_KEYS:
            assert np.array_equal(res[pre + k], g[pre + k]), pre + k
        for k in t.FLOAT_KEYS:
            if k.startswith("ref_err"):
                continue        # the float32 / bfloat16 runs depend on the host's BLAS blocking: recorded, compared loosely below
            assert res[pre + k].dtype == g[pre + k].dtype, pre + k
            # (the compact fixture stores its features as float32: equal after the same cast)
            assert np.abs(res[pre + k].astype(np.float64) - g[pre + k].astype(np.float64)).max() < 1e-9, pre + k
        for k in ("ref_err_fp32", "ref_err_bf16"):
            assert g[pre + k].shape == (len(t.ERR_KEYS),) and (g[pre + k] > 0).all(), pre + k
            assert (res[pre + k] < 4 * g[pre + k]).all() and (g[pre + k] < 4 * res[pre + k]).all(), (pre + k, res[pre + k], g[pre + k])
        # ragged lengths: at least one row of 1-3 tokens and one of the full 32; ids beyond a row's length are padding
        lens = g[pre + "lens"]
        assert lens.min() <= 3 and lens.max() == 32 and g[pre + "ids"].shape[1] == 32
        assert all((g[pre + "ids"][b, n:] == 0).all() for b, n in enumerate(lens))
        # the ITC matrix is the max over the queries of the stored features; the probabilities are the logits' softmax
        sc = np.einsum("iqp,tp->iqt", g[pre + "itc_image"].astype(np.float64), g[pre + "itc_text"].astype(np.float64)).max(1)
        assert np.abs(sc - g[pre + "itc_scores"]).max() < (1e-6 if name == "blip2_itm_width" else 1e-12)
        lg = g[pre + "itm_logits"]
        assert np.abs(1 / (1 + np.exp(lg[:, 0] - lg[:, 1])) - g[pre + "itm_prob"]).max() < 1e-12
    assert int(g["image_size"]) == (224 if name == "blip2_itm_width" else 28)


@pytest.mark.parametrize("name", ["blip2_itm_tiny", "blip2_itm_width"])
def test_hf_margins_leave_three_of_four_groups_above_twice_the_fp32_bar(name):
    """The GPU ranking test only looks at groups whose HF margin exceeds twice the mode's bar; in f32 / f32s at least 3 of every 4
    groups must qualify - the fixture is chosen so that HF's own margins satisfy that."""
    t = _tool()
    g = np.load(os.path.join(GOLDEN, f"{name}.npz"))
    err = dict(zip(t.ERR_KEYS, g["ref_err_fp32"]))
    for head, key in (("itm", "itm_prob"), ("itc", "itc_scores")):
        margin = g[f"group_{head}_margin"]
        ok = int((margin > 2 * 8 * err[key]).sum())
        assert 4 * ok >= 3 * len(margin), (head, margin, err[key])


def test_arch_from_hf_config_round_trip_and_checkpoint_dir(tmp_path):
    import transformers
    from embodied_captioning_amd.config import Blip2ItmArch
    from embodied_captioning_amd.weights import blip2_itm_param_specs, load_hf_blip2_itm_checkpoint, procedural_blip2_itm_state_dict
    t = _tool()
    for a in (Blip2ItmArch(), Blip2ItmArch.tiny(), Blip2ItmArch.width(364)):
        cfg = transformers.Blip2Config(**a.hf_config_dict())
        assert Blip2ItmArch.from_hf_config(cfg.to_dict()) == a
    assert Blip2ItmArch().n_tokens == 257 and Blip2ItmArch.width(364).n_tokens == 677
    d = Blip2ItmArch.tiny().hf_config_dict()
    d["qformer_config"]["use_qformer_text_input"] = False
    with pytest.raises(ValueError, match="use_qformer_text_input"):
        Blip2ItmArch.from_hf_config(d)
    d = Blip2ItmArch.tiny().hf_config_dict()
    d["image_token_index"] = 7
    with pytest.raises(ValueError, match="image_token_index"):
        Blip2ItmArch.from_hf_config(d)
    # save_pretrained of procedural weights loads back with every key accounted for
    a = Blip2ItmArch.tiny()
    m = t.hf_model(a, 4, dtype=torch.float32)
    m.save_pretrained(str(tmp_path))
    arch, sd = load_hf_blip2_itm_checkpoint(str(tmp_path))
    assert arch == a
    want = procedural_blip2_itm_state_dict(a, 4)
    assert set(sd) == set(want) == {n for n, *_ in blip2_itm_param_specs(a)}
    for k, v in want.items():
        assert torch.equal(sd[k].float().reshape(v.shape), v), k
    # every Q-Former layer carries both FFN sets and all three heads have a bias
    for i in range(a.q_layers):
        for ffn in ("intermediate", "output", "intermediate_query", "output_query"):
            assert f"qformer.encoder.layer.{i}.{ffn}.dense.weight" in sd
    assert {"vision_projection.bias", "text_projection.bias", "itm_head.bias"} <= set(sd)
    # LAVIS files are refused by name
    lavis = tmp_path / "blip2_pretrained.pth"
    lavis.write_bytes(b"")
    with pytest.raises(RuntimeError, match="HF-format"):
        load_hf_blip2_itm_checkpoint(str(lavis))
    empty = tmp_path / "empty"
    empty.mkdir()
    (empty / "config.json").write_text(json.dumps(transformers.Blip2Config(**a.hf_config_dict()).to_dict()))
    with pytest.raises(RuntimeError, match="HF-format"):
        load_hf_blip2_itm_checkpoint(str(empty))
    (empty / "model.safetensors.index.json").write_text("{}")          # a sharded directory is named as such
    with pytest.raises(RuntimeError, match="SHARDED"):
        load_hf_blip2_itm_checkpoint(str(empty))


def _toy_bert_tokenizer(tmp_path):
    import transformers
    words = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", "the", "cat", "sat", "on", "mat", "a", "red", "chair"]
    vf = tmp_path / "vocab.txt"
    vf.write_text("\n".join(words) + "\n")
    return transformers.BertTokenizer(str(vf)), {w: i for i, w in enumerate(words)}


def test_tokenisation_truncates_at_32_and_pads_per_batch(tmp_path):
    from embodied_captioning_amd.captioner.blip2_itm_scorer import pad_rows, tokenize_captions
    tok, sid = _toy_bert_tokenizer(tmp_path)
    caps = ["the cat", "the cat sat on the mat", "a", "a red chair " * 20]
    rows = tokenize_captions(tok, caps, 32)
    # the reference's call (:292), one caption at a time
    assert rows == [tok(c, truncation=True, max_length=32)["input_ids"] for c in caps]
    assert all(r[0] == sid["[CLS]"] and r[-1] == sid["[SEP]"] for r in rows)
    assert [len(r) for r in rows] == [4, 8, 3, 32]                     # the long caption is truncated, not refused
    assert rows[3][1:31] == [sid["a"], sid["red"], sid["chair"]] * 10
    ids, lens = pad_rows(rows[:3], pad=0)
    assert ids.shape == (3, 8) and ids.dtype == torch.int32 and lens.tolist() == [4, 8, 3]      # padded to THIS batch's longest row
    assert ids[0].tolist() == rows[0] + [0] * 4 and ids[2, 3:].eq(0).all()
    # HF's own padded batch has the same ids and mask
    batch = tok(caps[:3], truncation=True, padding=True, max_length=32, return_tensors="pt")
    assert torch.equal(batch["input_ids"].int(), ids) and batch["attention_mask"].sum(1).tolist() == lens.tolist()
    # procedural checkpoints have no vocabulary: id rows go through as they are, cut to 32 keeping the last id
    with pytest.raises(TypeError):
        tokenize_captions(None, ["the cat"], 32)
    long_row = [1] + list(range(10, 60)) + [2]
    assert tokenize_captions(None, [[1, 7, 2], long_row], 32) == [[1, 7, 2], [1] + list(range(10, 40)) + [2]]
    with pytest.raises(ValueError):
        tokenize_captions(None, [[]], 32)


def test_pixel_batches_slice_tensors_that_need_no_resize_and_refuse_other_arrays():
    """The shared `pixel_batches` on inputs that need no device: normalised float tensors and uint8 frames already at the tower's
    size go through as slices of at most batch_size, in order; a lone [3, S, S] image is a batch of one; anything that is not uint8
    [H, W, 3] is refused by name before any resize."""
    from embodied_captioning_amd.preprocess import pixel_batches
    S = 8
    for x in (torch.randn(7, 3, S, S), torch.randint(0, 256, (7, S, S, 3), dtype=torch.uint8)):
        got = list(pixel_batches(x, S, 3, "cpu", center_crop=False))
        assert [b.shape[0] for b in got] == [3, 3, 1] and torch.equal(torch.cat(got), x)
        assert all(b.data_ptr() == x[i * 3:].data_ptr() for i, b in enumerate(got))       # views, not copies
        assert len(list(pixel_batches(x, S, 7, "cpu", center_crop=True, geometry="hf"))) == 1
    one = torch.randn(3, S, S)
    got = list(pixel_batches(one, S, 4, "cpu"))
    assert len(got) == 1 and got[0].shape == (1, 3, S, S) and torch.equal(got[0][0], one)
    assert list(pixel_batches(torch.zeros(0, 3, S, S), S, 4, "cpu")) == [] and list(pixel_batches([], S, 4, "cpu")) == []
    for bad in ([np.zeros((5, 6, 3), np.float32)], [np.zeros((5, 6), np.uint8)], [np.zeros((5, 6, 4), np.uint8)]):
        with pytest.raises(ValueError, match="images must be PIL, uint8"):
            list(pixel_batches(bad, S, 4, "cpu"))


class _StubScorer:
    """Score = the image's mean red value / 100 (the crop's BGR -> RGB swap shows)."""

    def __init__(self):
        self.calls = []

    def score_pairs(self, images, captions, head="itm"):
        self.calls.append((len(images), [c.shape for c in images], list(captions), head))
        return [float(c[..., 0].mean()) / 100 for c in images]


def _frame(h, w, red):
    f = np.zeros((h, w, 3), dtype=np.uint8)
    f[..., 2] = red                        # BGR: channel 2 is red
    return f


@pytest.mark.parametrize("head", ["itm", "itc"])
def test_blip2_pseudo_scores_stub_one_call_reference_shape_and_order(head):
    from embodied_captioning_amd.pseudocaptioner import blip2_pseudo_scores, host_crops
    fa, fb = _frame(480, 640, 200), _frame(720, 1280, 50)
    grouped = {
        (0, 1): [{"image": fa, "pred_box": np.array([10, 10, 100, 100], np.float32), "caption": "low"},
                 {"image": fb, "pred_box": np.array([0, 0, 50, 50], np.float32), "caption": "a"},
                 {"image": fb, "pred_box": np.array([5, 5, 60, 60], np.float32), "caption": "b"},
                 {"image": fa, "pred_box": np.array([20, 20, 40, 40], np.float32), "caption": "high"}],
        (0, 2): [{"image": fb, "pred_box": np.array([1200, 700, 1279, 719], np.float32), "caption": "edge"}],
        (0, 3): [],
    }
    stub = _StubScorer()
    out = blip2_pseudo_scores(grouped, stub, head, crop=host_crops)
    assert len(stub.calls) == 1 and stub.calls[0][0] == 5 and stub.calls[0][3] == head      # one batched call for every pair
    assert stub.calls[0][2] == ["low", "a", "b", "high", "edge"]
    assert [s[:2] for s in stub.calls[0][1][:4]] == [(108, 108), (55, 55), (65, 65), (24, 24)]   # shared crop step of --method clip
    # the reference's blip2_score output: captions and scores in INPUT order, nothing sorted, no pseudocaption
    assert out == {"(0, 1)": {"captions": ["low", "a", "b", "high"], "scores": [2.0, 0.5, 0.5, 2.0]},
                   "(0, 2)": {"captions": ["edge"], "scores": [0.5]}}
    json.loads(json.dumps(out))
    assert blip2_pseudo_scores({}, stub, head, crop=host_crops) == {} and len(stub.calls) == 1


def test_driver_accepts_blip2_methods_and_refuses_the_rest_by_name(tmp_path, monkeypatch):
    from embodied_captioning_amd import pseudocaptioner as P
    from embodied_captioning_amd.captioner import blip2_itm_scorer as S
    from embodied_captioning_amd.pseudolabeler import record_name, save_record
    assert P.REFUSED_METHODS == ("llm", "mobileclip", "openclip")
    img = _frame(64, 96, 10)
    inst = {"captions": ["a red chair", "a lamp"], "pred_boxes": [np.array([1, 2, 30, 40], np.float32)] * 2,
            "infos": [{"id_episode": 3, "id_object": 1}, {"id_episode": 3, "id_object": 2}]}
    save_record(str(tmp_path), record_name(3, 5)[:-4], inst, img)
    made = []

    class Fake:
        def __init__(self, name, device, dtype, batch_size):
            made.append((name, dtype, batch_size))

        def close(self):
            made.append("closed")

    monkeypatch.setattr(S, "Blip2ItmScorer", Fake)
    seen = []
    monkeypatch.setattr(P, "blip2_pseudo_scores", lambda grouped, scorer, head: seen.append((list(grouped), head)) or {"k": {"captions": [], "scores": []}})
    for method, head in (("blip2_itm", "itm"), ("blip2_itc", "itc")):
        out = tmp_path / f"{method}.json"
        assert P.main(["--file_path", str(tmp_path), "--output_csv_path", str(out), "--method", method, "--dtype", "bf16"]) == 0
        assert json.loads(out.read_text()) == {"k": {"captions": [], "scores": []}}
        assert seen[-1] == ([(3, 1), (3, 2)], head)
    assert made == [("Salesforce/blip2-itm-vit-g-coco", "bf16", 256), "closed"] * 2
    assert P.main(["--file_path", str(tmp_path), "--output_csv_path", str(tmp_path / "m.json"), "--method", "blip2_itm", "--model", "/some/dir"]) == 0
    assert made[-2][0] == "/some/dir"
    for m in ("llm", "mobileclip", "openclip"):
        with pytest.raises(SystemExit, match=m):
            P.main(["--file_path", str(tmp_path), "--output_csv_path", str(tmp_path / "o.json"), "--method", m])
    with pytest.raises(SystemExit, match="unknown"):
        P.main(["--file_path", str(tmp_path), "--output_csv_path", str(tmp_path / "o.json"), "--method", "blip3"])


def test_scorer_without_a_gpu_raises_and_names_are_parsed(monkeypatch):
    from embodied_captioning_amd._native import CaptionerHipError
    from embodied_captioning_amd.captioner import blip2_itm_scorer as S
    from embodied_captioning_amd.config import Blip2ItmArch
    assert S._parse_procedural("procedural-blip2-itm-tiny:7") == (Blip2ItmArch.tiny(), 7)
    assert S._parse_procedural("procedural-blip2-itm") == (Blip2ItmArch(), 0)
    assert S._parse_procedural("Salesforce/blip2-itm-vit-g") is None
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(CaptionerHipError, match="GPU"):          # there is no CPU fallback in this project
        S.Blip2ItmScorer("procedural-blip2-itm-tiny:3", dtype="f32")
    with pytest.raises(ValueError, match="int8"):
        S.Blip2ItmScorer("procedural-blip2-itm-tiny:3", dtype="int8")
    with pytest.raises(FileNotFoundError, match="HF-format"):
        S.Blip2ItmScorer("/nonexistent/blip2_pretrained.pth")
