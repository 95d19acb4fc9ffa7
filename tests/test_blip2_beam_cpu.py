"""CPU: the beam search over the BLIP-2 restatement (tests/_blip2_beam_ref.py) against the HF golden (tests/golden/blip2_tiny_beam.npz,
tools/make_goldens_blip2_beam.py).  This pins the numbering the device loop uses - token columns [BOS, new tokens ...], the prompt of
33 positions taken off every length HF computes - before anything runs on a GPU."""
import json
import os

import numpy as np
import pytest

import _blip2_beam_ref as BR

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "blip2_tiny_beam.npz")
_CACHE = {}


def load_beam_golden():
    """-> (npz, meta).  meta["cases"][key] = {K, lp, seed}; arrays ids_/scores_/top2_/gap_/omit_ + key."""
    g = np.load(GOLD)
    return g, json.loads(str(g["meta"]))


def case_inputs(meta, key):
    from embodied_captioning_amd.config import Blip2Arch
    from embodied_captioning_amd.weights import procedural_blip2_state_dict, synthetic_pixels
    c = meta["cases"][key]
    a = Blip2Arch.tiny()
    sd = procedural_blip2_state_dict(a, c["seed"], eos_boost=meta["eos_boost"])
    return a, sd, synthetic_pixels(meta["batch"], a.image_size, seed=c["seed"]), c["K"], c["lp"]


def restatements(key):
    """(fp32, fp64) restatement of a golden case: computed once, shared, never modified."""
    if key not in _CACHE:
        _, meta = load_beam_golden()
        a, sd, px, K, lp = case_inputs(meta, key)
        _CACHE[key] = tuple(BR.beam_search(sd, a, px, K, lp, dtype=dt) for dt in (np.float32, np.float64))
    return _CACHE[key]


KEYS = ["k3_lp1", "k3_lp2", "k5_lp1"]


def test_golden_file_covers_the_cases():
    g, meta = load_beam_golden()
    assert sorted(meta["cases"]) == sorted(KEYS)
    assert [(meta["cases"][k]["K"], meta["cases"][k]["lp"]) for k in KEYS] == [(3, 1.0), (3, 2.0), (5, 1.0)]
    for k in KEYS:
        assert g[f"ids_{k}"].shape == (4, 20) and g[f"scores_{k}"].shape == (4,) and g[f"top2_{k}"].shape == (4,)
        assert len(g[f"omit_{k}"]) <= 1
        # the omitted images are exactly those below the bar, as the tool decided them
        assert np.array_equal(np.nonzero(g[f"gap_{k}"] < meta["gap_bar"])[0], g[f"omit_{k}"])


@pytest.mark.parametrize("key", KEYS)
def test_fp32_restatement_reproduces_hf(key):
    """Tokens identical on the images the file keeps; scores within 1e-4 (SURVEY section 7 step 1's bar for beam scores) on every
    image that returns HF's hypothesis - the kept ones and an omitted one whose near-tie fell as HF's did (another hypothesis has
    another score)."""
    g, meta = load_beam_golden()
    r32, _ = restatements(key)
    keep = np.setdiff1d(np.arange(meta["batch"]), g[f"omit_{key}"])
    assert np.array_equal(r32["ids"][keep], g[f"ids_{key}"][keep])
    a = case_inputs(meta, key)[0]
    want_len = np.array([int(np.argmax(r == a.eos)) + 1 if (r == a.eos).any() else r.size for r in g[f"ids_{key}"]])
    assert np.array_equal(r32["lens"][keep], want_len[keep])
    scored = np.array([b for b in range(meta["batch"]) if np.array_equal(r32["ids"][b], g[f"ids_{key}"][b])])
    assert set(keep) <= set(scored)
    assert np.abs(r32["scores"][scored] - g[f"scores_{key}"][scored]).max() < 1e-4


@pytest.mark.parametrize("key", KEYS)
def test_fp32_and_fp64_restatements_decide_alike(key):
    """Every golden image (the omitted ones included: their near-ties are below 1e-3, far above fp32's error on these scores)."""
    g, _ = load_beam_golden()
    r32, r64 = restatements(key)
    assert np.array_equal(r32["ids"], r64["ids"]) and np.array_equal(r32["lens"], r64["lens"])
    assert r32["steps"] == r64["steps"] and r32["reorders"] == r64["reorders"]
    assert np.abs(r32["scores"].astype(np.float64) - r64["scores"]).max() < 1e-4
    assert np.allclose(r64["gap"], g[f"gap_{key}"], rtol=0, atol=1e-9)
    assert r64["reorders"] >= 3          # the cases are worth pinning: steps that read a cache through another row's history
