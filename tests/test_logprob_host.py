"""CPU: the host half of the batched per-caption perplexity - `perplexity_from_logprobs`, the new ABI symbols, and the pool's
split of a merged pass carrying the two new per-row outputs."""
import json
import os

import pytest
import torch


def _kats(golden_dir):
    return [k for k in json.load(open(os.path.join(golden_dir, "perplexity_kat.json"))) if k["target_is_argmax"]]


def test_perplexity_from_logprobs_equals_compute_perplexity_on_the_kats(golden_dir):
    """Per-step log max softmax in float64 -> helper == CaptioningPredictor.compute_perplexity on the same float64 logits."""
    from embodied_captioning_amd.captioner.captioning_predictor import CaptioningPredictor
    from embodied_captioning_amd.engine import perplexity_from_logprobs
    m = CaptioningPredictor()
    kats = _kats(golden_dir)
    assert len(kats) == 3
    for k in kats:
        x = torch.tensor(k["input"], dtype=torch.float64).permute(1, 0, 2)          # [1, T, V]
        lp = torch.log_softmax(x, dim=-1).max(dim=-1).values                         # [1, T]
        got = perplexity_from_logprobs(lp, torch.tensor([lp.shape[1]], dtype=torch.int32))
        want = m.compute_perplexity(x)
        assert got.dtype == torch.float64 and got.shape == (1,) and want.dtype == torch.float64
        assert abs(float(got[0]) - float(want)) <= 1e-12 * abs(float(want))
        assert abs(float(got[0]) - k["expected"]) <= 1e-3 * k["expected"]


def test_perplexity_from_logprobs_counts_scored_steps_only():
    from embodied_captioning_amd.engine import perplexity_from_logprobs
    g = torch.Generator().manual_seed(3)
    steps = 7
    lp = -torch.rand((4, steps), generator=g, dtype=torch.float64).to(torch.float32) * 5.0
    scored = torch.tensor([1, steps, 3, 5], dtype=torch.int32)
    want = torch.stack([torch.exp(-lp[r, :n].double().sum() / n) for r, n in enumerate(scored.tolist())])
    clean = lp.clone()
    for r, n in enumerate(scored.tolist()):
        clean[r, n:] = 0.0                                         # what the library leaves after a caption's end
    got = perplexity_from_logprobs(clean, scored)
    assert got.dtype == torch.float64 and torch.allclose(got, want, rtol=1e-15, atol=0.0)
    # whatever sits beyond `scored` does not enter
    assert torch.equal(perplexity_from_logprobs(lp, scored), got)
    assert float(got[0]) == float(torch.exp(-lp[0, 0].double()))
    with pytest.raises(ValueError):
        perplexity_from_logprobs(lp, torch.tensor([1, steps + 1, 3, 5]))
    with pytest.raises(ValueError):
        perplexity_from_logprobs(lp[0], scored)


def test_library_exports_the_scored_entry_points():
    from embodied_captioning_amd import _native, build
    build.build(verbose=False)
    lib = _native.load_library()
    for name in ("cap_generate_scored", "cap_op_select_logprob"):
        assert hasattr(lib, name) and name in _native.EXPORTS
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "captioner_hip.h")).read()
    assert "cap_generate_scored(" in text and "cap_op_select_logprob(" in text


def test_pool_splits_the_new_per_row_outputs_of_a_merged_pass():
    from embodied_captioning_amd._native import CaptionerHipError
    from embodied_captioning_amd.engine import EnginePool
    assert {"token_logprobs", "scored_steps"} <= set(EnginePool._PER_ROW_OUTPUTS)
    rows = [8, 8, 5, 3]
    plan = EnginePool.coalesce_plan(rows, 2, 16)
    assert plan == [[0, 1], [2, 3]]
    outs_m, r0 = [], 0
    for g in plan:
        n = sum(rows[j] for j in g)
        idx = torch.arange(r0, r0 + n)
        outs_m.append({"sequences": idx[:, None].repeat(1, 4).int(), "lengths": idx.int(),
                       "token_logprobs": -idx[:, None].float() - torch.arange(3)[None, :] / 8.0, "scored_steps": (idx % 4).int()})
        r0 += n
    outs = EnginePool.split_merged_outputs(plan, rows, outs_m)
    r0 = 0
    for j, n in enumerate(rows):
        idx = torch.arange(r0, r0 + n)
        assert set(outs[j]) == {"sequences", "lengths", "token_logprobs", "scored_steps"}
        assert torch.equal(outs[j]["token_logprobs"], -idx[:, None].float() - torch.arange(3)[None, :] / 8.0)
        assert torch.equal(outs[j]["scored_steps"], (idx % 4).int()) and torch.equal(outs[j]["lengths"], idx.int())
        r0 += n
    with pytest.raises(CaptionerHipError):
        EnginePool.split_merged_outputs(plan, rows, [dict(o, logits=torch.zeros(1)) for o in outs_m])
