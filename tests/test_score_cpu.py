"""CPU: the host side of caption scoring - the restatement (tests/_score_ref.py) against the HF golden, `validate_score_ids`,
`score_summary`, `likelihood_pseudo_captions` on a stub scorer, and the CLI's routing of `--method blip_ll`.  Needs no GPU.
"""
import json
import os

import numpy as np
import pytest
import torch

from _score_ref import blip_score, random_captions

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "blip_tiny_score.npz")


def _golden():
    from embodied_captioning_amd.config import BlipArch
    from embodied_captioning_amd.weights import procedural_blip_state_dict, synthetic_pixels
    g = np.load(GOLDEN)
    meta = json.loads(str(g["meta"]))
    arch = BlipArch(**meta["arch"])
    return g, meta, arch, procedural_blip_state_dict(arch, meta["seed"], eos_boost=meta["eos_boost"]), \
        synthetic_pixels(meta["batch"], arch.image_size, seed=meta["seed"])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_restatement_reproduces_the_hf_golden(dtype):
    g, meta, arch, sd, px = _golden()
    ids, lens = g["ids"], g["lens"]
    assert ids.shape == (12, 12) and sorted(set(lens.tolist())) == [2, 5, 7, 9, 12]     # lengths 2, a middle one and L per image
    ref = blip_score(sd, arch, px, ids, lens, meta["captions_per_image"], dtype)
    live = np.arange(11)[None, :] < (lens[:, None] - 1)
    assert np.array_equal(ref["live"], live)
    assert np.abs(ref["token_logprobs"] - g["token_logprobs"])[live].max() <= 1e-4
    sure = live & (g["margin"] > 1e-4)
    assert np.array_equal(ref["top_ids"][sure], g["top_ids"][sure])
    assert float(np.abs(g["token_logprobs"][~live]).max()) == 0.0 and bool((g["token_logprobs"][live] < 0).all())
    own = meta["own_caption_row"]                                  # HF's own greedy caption, its [SEP] included: its own arg-max path
    n = int(lens[own]) - 1
    assert int(ids[own, n]) == arch.eos and np.array_equal(g["top_ids"][own, :n], ids[own, 1:n + 1])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_blip2_restatement_reproduces_the_hf_golden(dtype):
    from _score_ref import blip2_score
    from embodied_captioning_amd.config import Blip2Arch
    from embodied_captioning_amd.weights import procedural_blip2_state_dict, synthetic_pixels
    g = np.load(os.path.join(os.path.dirname(GOLDEN), "blip2_tiny_score.npz"))
    meta = json.loads(str(g["meta"]))
    arch = Blip2Arch(**meta["arch"])
    sd = procedural_blip2_state_dict(arch, meta["seed"], eos_boost=meta["eos_boost"])
    px = synthetic_pixels(meta["batch"], arch.image_size, seed=meta["seed"])
    ids, lens = g["ids"], g["lens"]
    assert ids.shape == (12, 12) and {2, 12} <= set(lens.tolist()) and len(set(lens.tolist())) >= 4
    ref = blip2_score(sd, arch, px, ids, lens, meta["captions_per_image"], dtype)
    live = np.arange(11)[None, :] < (lens[:, None] - 1)
    assert np.array_equal(ref["live"], live)
    assert np.abs(ref["token_logprobs"] - g["token_logprobs"])[live].max() <= 1e-4
    sure = live & (g["margin"] > 1e-4)
    assert np.array_equal(ref["top_ids"][sure], g["top_ids"][sure])
    own = meta["own_caption_row"]                                  # HF's own greedy caption with its generation EOS
    n = int(lens[own]) - 1
    assert int(ids[own, n]) == arch.eos and np.array_equal(g["top_ids"][own, :n], ids[own, 1:n + 1])


def test_blip2_validation_takes_opt_ids():
    from embodied_captioning_amd.config import Blip2Arch
    from embodied_captioning_amd.engine import validate_score_ids
    arch = Blip2Arch.tiny()
    ids = random_captions(arch, 2, 5, None, seed=0)
    ids[0, 4] = arch.eos
    t, ln = validate_score_ids(ids, [5, 3], arch, 2, limit=5)
    assert ln.tolist() == [5, 3]
    ids[1, 1] = arch.eos
    with pytest.raises(ValueError, match="EOS"):
        validate_score_ids(ids, [5, 3], arch, 2)


def test_validate_score_ids_names_every_fault():
    from embodied_captioning_amd.config import BlipArch, CocaArch
    from embodied_captioning_amd.engine import validate_score_ids
    arch = BlipArch.tiny()
    L = 6
    ids = random_captions(arch, 6, L, None, seed=0)
    lens = np.array([6, 2, 4, 6, 3, 5])
    ids[3, 5] = arch.eos                                           # EOS as the last token is allowed
    ids[4, 3:] = [arch.pad, arch.eos, arch.bos]                    # anything behind a caption's end is padding
    t, ln = validate_score_ids(ids, lens, arch, 6)
    assert t.dtype == torch.int32 and ln.dtype == torch.int32 and tuple(t.shape) == (6, L) and ln.tolist() == lens.tolist()
    t, ln = validate_score_ids(ids.tolist(), [6, 0, 4, 6, 0, 5], arch, 2, captions_per_image=3)     # absent slots with C > 1
    assert ln.tolist() == [6, 0, 4, 6, 0, 5]

    def bad(match, ids_=ids, lens_=lens, arch_=arch, n=6, C=1, **kw):
        with pytest.raises(ValueError, match=match):
            validate_score_ids(ids_, lens_, arch_, n, C, **kw)

    bad("CoCa", arch_=CocaArch.tiny())
    bad("captions_per_image", C=0)
    bad("integers", ids_=ids.astype(np.float32))
    bad("integers", lens_=lens.astype(np.float64))
    bad(r"ids must be \[N, L\]", n=5)
    bad(r"ids must be \[N, L\]", ids_=ids[0])
    bad(r"lens must be \[N\]", lens_=lens[:5])
    bad("L >= 2", ids_=ids[:, :1], lens_=np.full(6, 2))
    bad("nothing to score", ids_=ids[:0], lens_=lens[:0], n=0)
    bad("too long", limit=5)
    bad("absent slot", lens_=np.array([6, 0, 4, 6, 3, 5]))
    bad("outside", lens_=np.array([6, 1, 4, 6, 3, 5]))
    bad("outside", lens_=np.array([6, 2, 4, 7, 3, 5]))
    bad("outside", lens_=np.array([6, 2, -1, 6, 3, 5]))
    for v in (-1, arch.vocab):
        x = ids.copy()
        x[4, 5] = v                                                # in the padding too: nothing out of range is ever gathered
        bad("out of range", ids_=x)
    x = ids.copy()
    x[2, 0] = 7
    bad("BOS", ids_=x)
    x = ids.copy()
    x[0, 2] = arch.pad
    bad("pad", ids_=x)
    x = ids.copy()
    x[0, 2] = arch.eos
    bad("EOS", ids_=x)
    x = ids.copy()
    x[1, 1] = arch.eos                                             # [BOS, EOS]: the empty caption, its end scored - allowed
    validate_score_ids(x, lens, arch, 6)


def test_score_summary_is_float64_on_the_returned_logprobs():
    from embodied_captioning_amd.engine import score_summary
    g = torch.Generator().manual_seed(3)
    lp = -torch.rand((4, 7), generator=g)
    top = lp * 0.5
    n = torch.tensor([7, 3, 0, 1], dtype=torch.int32)
    s = score_summary(lp, top, n)
    for r in range(4):
        k = int(n[r])
        if k == 0:
            assert all(torch.isnan(s[key][r]) for key in ("logprob_mean", "perplexity", "top_perplexity")) and float(s["logprob_sum"][r]) == 0.0
            continue
        tot = float(lp[r, :k].double().sum())
        assert abs(float(s["logprob_sum"][r]) - tot) < 1e-12 and abs(float(s["logprob_mean"][r]) - tot / k) < 1e-12
        assert abs(float(s["perplexity"][r]) - np.exp(-tot / k)) < 1e-12
        assert abs(float(s["top_perplexity"][r]) - np.exp(-float(top[r, :k].double().sum()) / k)) < 1e-12
    assert s["n_tokens"].tolist() == [7, 3, 0, 1] and s["perplexity"].dtype == torch.float64


class _StubScorer:
    """score_matrix from a table: value of (crop, caption) = table[caption] + 0.01 * crop index within the call."""
    def __init__(self, table):
        self.table, self.calls = table, []

    def score_matrix(self, images, captions):
        self.calls.append((len(images), list(captions)))
        return np.array([[self.table[c] + 0.01 * i for c in captions] for i in range(len(images))])


def _grouped():
    frame_a, frame_b = np.zeros((64, 64, 3), np.uint8), np.ones((64, 64, 3), np.uint8)
    box = np.array([8, 8, 40, 40], np.float32)
    mk = lambda f, c: {"image": f, "pred_box": box, "caption": c}      # noqa: E731
    return {(0, 1): [mk(frame_a, "a chair"), mk(frame_b, "a sofa"), mk(frame_a, "a chair"), mk(frame_b, "a stool")],
            (0, 2): [mk(frame_b, "a lamp")], (0, 3): []}


def test_likelihood_pseudo_captions_ordering_deduplication_and_stability():
    from embodied_captioning_amd.pseudocaptioner import likelihood_pseudo_captions
    crop = lambda frames, rects: [(fi, j) for fi, rs in enumerate(rects) for j in range(len(rs))]      # noqa: E731 - frame-major crops
    sc = _StubScorer({"a chair": -1.5, "a sofa": -0.5, "a stool": -1.5, "a lamp": -2.0})
    out = likelihood_pseudo_captions(_grouped(), sc, crop=crop)
    assert set(out) == {"(0, 1)", "(0, 2)"}                        # an empty group has no entry
    # every distinct caption once (first-occurrence order), against every crop of the group, in one call per group
    assert sc.calls == [(4, ["a chair", "a sofa", "a stool"]), (1, ["a lamp"])]
    mean = 0.01 * (0 + 1 + 2 + 3) / 4
    lst = out["(0, 1)"]["captions_list"]
    assert [c for _, c in lst] == ["a sofa", "a chair", "a stool"]  # descending; the tie keeps first-occurrence order
    assert np.allclose([s for s, _ in lst], [-0.5 + mean, -1.5 + mean, -1.5 + mean], atol=1e-12)
    assert out["(0, 1)"]["pseudocaption"] == lst[0] and out["(0, 2)"]["pseudocaption"] == [-2.0, "a lamp"]
    assert likelihood_pseudo_captions({(1, 1): []}, sc, crop=crop) == {}


def test_cli_routes_blip_ll_and_blip2_ll(tmp_path, monkeypatch):
    from embodied_captioning_amd import pseudocaptioner as P
    from embodied_captioning_amd.captioner import likelihood_scorer as S
    made, seen = [], []

    class Fake:
        def __init__(self, name, device, dtype, batch_size, family):
            made.append((name, device, dtype, batch_size, family))

        def close(self):
            made.append("closed")

    monkeypatch.setattr(S, "CaptionLikelihoodScorer", Fake)
    monkeypatch.setattr(P, "group_records", lambda paths: {"g": []})
    monkeypatch.setattr(P, "likelihood_pseudo_captions", lambda grouped, scorer: seen.append(list(grouped)) or {"k": {"captions_list": [], "pseudocaption": []}})
    out = tmp_path / "o.json"
    assert P.main(["--file_path", str(tmp_path), "--output_csv_path", str(out), "--method", "blip_ll", "--dtype", "bf16"]) == 0
    assert made == [(P.DEFAULT_MODELS["blip_ll"], "cuda:0", "bf16", 32, "blip"), "closed"] and seen == [["g"]]
    assert P.main(["--file_path", str(tmp_path), "--output_csv_path", str(out), "--method", "blip2_ll", "--model", "/some/dir"]) == 0
    assert made[2:] == [("/some/dir", "cuda:0", "f32s", 32, "blip2"), "closed"]
    assert json.loads(out.read_text()) == {"k": {"captions_list": [], "pseudocaption": []}}
    for m in P.REFUSED_METHODS:                                    # unchanged
        with pytest.raises(SystemExit, match=m):
            P.main(["--file_path", str(tmp_path), "--output_csv_path", str(out), "--method", m])
    with pytest.raises(SystemExit, match="unknown"):
        P.main(["--file_path", str(tmp_path), "--output_csv_path", str(out), "--method", "blip_lll"])


def test_coca_wrapper_refuses_by_name():
    from embodied_captioning_amd.captioner.models.coca.coca import CoCa
    with pytest.raises(ValueError, match="CoCa"):
        CoCa.score_captions(object.__new__(CoCa), [], [])


def test_score_matrix_leaves_an_overlong_caption_out_and_copies_duplicates():
    import types
    from embodied_captioning_amd.captioner.likelihood_scorer import CaptionLikelihoodScorer
    calls = []

    class Model:
        arch, device = "arch", "dev"
        engine = types.SimpleNamespace(score_limit=4)

        def caption_ids(self, c):
            return [510] + list(c)

        def score_captions(self, images, groups):
            calls.append([list(g) for g in groups])
            n, C = len(images), len(groups[0])
            return {"logprob_mean": torch.arange(n * C, dtype=torch.float64) * -1.0, "captions_per_image": C}

    sc = CaptionLikelihoodScorer(model=Model())
    m = sc.score_matrix(["i0", "i1"], [(1, 2), (1, 2, 3, 4), (7,), (1, 2)])        # the second is 5 tokens with BOS: beyond the limit
    assert calls == [[[(1, 2), (7,)], [(1, 2), (7,)]]]                              # distinct, scorable captions once per image
    assert m.tolist() == [[-0.0, float("-inf"), -1.0, -0.0], [-2.0, float("-inf"), -3.0, -2.0]]
    assert sc.score_matrix(["i0"], [(1, 2, 3, 4)]).tolist() == [[float("-inf")]] and len(calls) == 1
