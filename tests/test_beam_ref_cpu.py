"""CPU: the host beam-search reference (tests/_beam_ref.py) held to HF's own `generate` (tests/golden/beam_scripted.npz, recorded by
oracle/beam_scripted_ref.py on the scripted model of tests/_beam_script.py), and the margins of the committed cases - so that
tests/test_beam_search_gpu.py measures the HIP kernels against something that is not only ours, and never against a decision that
a last-bit difference in the kernel's log-softmax sum could turn.

Score bar (the rule of tests/test_attention_kernels_gpu.py): 8 x max |fp32 host reference - fp64 host reference| over the case's
unmasked final and running scores, plus one fp32 spacing of the score."""
import os

import numpy as np
import pytest

from _beam_ref import bar, beam_search, min_gaps, refs, same_decisions
from _beam_script import BY_NAME, CASES, LEGACY, V5, elements_at_or_above_the_bound, logits_row

GAP_FACTOR = 64.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "beam_scripted.npz")


@pytest.fixture(scope="module")
def hf():
    return np.load(GOLDEN)


def test_record_covers_every_v5_case_hf_can_run(hf):
    want = [c.name for c in CASES if c.mode == V5 and not c.tie and c.K > 1]
    assert list(hf["names"]) == want
    assert str(hf["transformers_version"]).startswith("5.")
    for name in want:
        c = BY_NAME[name]
        assert hf[name + "/params"].tolist() == [c.seed, c.B, c.K, c.V, c.max_len, c.eos, c.bos], name
        assert float(hf[name + "/lp"]) == c.lp


@pytest.mark.parametrize("name", [c.name for c in CASES if c.mode == V5 and not c.tie and c.K > 1])
def test_fp32_reference_reproduces_hf_generate(hf, name):
    case = BY_NAME[name]
    r32, _, err = refs(case)
    assert np.array_equal(r32["ids"], hf[name + "/sequences"]), (r32["ids"], hf[name + "/sequences"])
    for b in range(case.B):
        got, want = float(r32["scores"][b]), float(hf[name + "/scores"][b])
        assert abs(got - want) <= bar(err, want), (b, got, want, bar(err, want))
        # the sequence ends where the reference says it does: EOS (or max_len) at lens - 1, fill after
        n = int(r32["lens"][b])
        assert (r32["ids"][b, n:] == case.fill).all() and (n == case.max_len or r32["ids"][b, n - 1] == case.eos)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_case_margins(case):
    """fp32 and fp64 agree on every decision, and every deciding comparison is either an exact tie (tie cases only, equal in
    both formats) or wider than 64 x the case's own fp32-vs-fp64 score error."""
    r32, r64, err = refs(case)
    assert same_decisions(r32, r64)
    g64 = min_gaps(r64, positive_only=case.tie)
    for kind, g in g64.items():
        assert g > 0.0 and g >= GAP_FACTOR * err, (kind, g, err)
    zero = min(min_gaps(r64).values()) == 0.0
    assert zero == case.tie, "a tie case has exact ties, the others none"
    if case.tie:
        assert min(min_gaps(r32).values()) == 0.0


def _stops(r):
    """Per item, the cur_len of the step at which its early-stop flag dropped (None: never)."""
    n = r["ids"].shape[0]
    out = [None] * n
    for s in r["steps"]:
        for b in range(n):
            if out[b] is None and not s["open"][b]:
                out[b] = s["cur_len"]
    return out


def test_cases_have_the_shapes_their_names_promise():
    for mode in ("v5", "legacy"):
        never = refs(BY_NAME[mode + "_never_ends"])[1]
        L = BY_NAME[mode + "_never_ends"].max_len
        assert never["stop_cur_len"] == L - 1 and (never["lens"] == L).all()
        assert all(s["open"].all() for s in never["steps"][:-1])
        eos2 = BY_NAME[mode + "_all_eos_step2"]
        r = refs(eos2)[1]
        assert (r["lens"] == 3).all() and (r["ids"][:, 2] == eos2.eos).all() and r["stop_cur_len"] <= 3
        assert any(s["displaced"].any() for s in refs(BY_NAME[mode + "_late_displaces"])[1]["steps"])
        d = _stops(refs(BY_NAME[mode + "_items_differ"])[1])
        assert len(set(d)) == 3, d
    # both early stops and max_len ends occur in both modes
    for mode in (V5, LEGACY):
        ends = [refs(c)[1]["stop_cur_len"] == c.max_len - 1 for c in CASES if c.mode == mode]
        assert any(ends) and not all(ends)
    assert {c.K for c in CASES} >= {1, 2, 3, 4, 5, 8}
    assert {c.min_len for c in CASES if c.mode == LEGACY} == {0, 3}
    assert {c.lp for c in CASES if not c.tie} >= {0.0, 0.6, 1.0, 2.0}
    # MinLength bites: with the mask off, the masked legacy cases end differently
    import dataclasses
    for c in CASES:
        if c.min_len and not c.tie:
            off = beam_search(dataclasses.replace(c, min_len=0), np.float64)
            assert not np.array_equal(off["ids"], refs(c)[1]["ids"]), c.name


def test_every_launch_branch_and_template_width_is_among_the_cases():
    """launch_beam_rows: row in LDS (lds <= 148 KiB, ld % 4 == 0, V > 2K), candidate lists only (row too large), plain kernel
    (ld % 4 != 0 or V <= 2K); list widths <4> (2K <= 4), <8> (2K <= 8), <16>.  The width matters only in the kernel's fallback
    (more than 1024 elements at its bound): the comb cases reach it, once per width, and from both row sources at <16>."""
    seen, per_mode = set(), set()
    for c in CASES:
        lds = (c.V + 3) // 4 * 16 + 2 * c.K * 256 * 8
        width = 4 if 2 * c.K <= 4 else 8 if 2 * c.K <= 8 else 16
        fast = c.row_ld % 4 == 0 and c.V > 2 * c.K
        branch = ("lds" if lds <= 148 * 1024 else "lists") if fast else "plain"
        seen.add((branch, width if fast else 0))
        per_mode.add((branch, c.mode))
    assert seen >= {("lds", 4), ("lds", 8), ("lds", 16), ("lists", 16), ("plain", 0)}
    assert per_mode == {(b, m) for b in ("lds", "lists", "plain") for m in (V5, LEGACY)}
    assert any(c.row_ld % 4 for c in CASES) and any(c.V == 2 * c.K for c in CASES)
    assert {c.V for c in CASES} >= {64, 1000, 30524, 49408} and {c.B for c in CASES} == {1, 3} and max(c.max_len for c in CASES) <= 12
    fallback = set()
    for c in CASES:
        lds = (c.V + 3) // 4 * 16 + 2 * c.K * 256 * 8
        n = elements_at_or_above_the_bound(logits_row(c, 0, (c.bos,)), c.K)
        if c.kind == "comb":
            assert n > 1024, (c.name, n)
            fallback.add(("lds" if lds <= 148 * 1024 else "lists", 4 if 2 * c.K <= 4 else 8 if 2 * c.K <= 8 else 16))
        elif c.row_ld % 4 == 0 and c.V > 2 * c.K and not c.tie:
            assert n <= 1024, (c.name, n)
    assert fallback == {("lds", 16), ("lists", 16), ("lists", 8), ("lists", 4)}
