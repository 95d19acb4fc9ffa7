"""A scripted "language model" with no weights, for the beam-search tests (tests/_beam_ref.py, tests/test_beam_ref_cpu.py,
tests/test_beam_search_gpu.py, oracle/beam_scripted_ref.py): the fp32 logits row of a beam is a function of (case seed, item index,
the beam's token prefix) only, so the HIP kernels, the host reference and HF's generate all see bit-identical rows whatever order
they ask in.

  normal rows   numpy.random.default_rng([seed, item, *prefix]).standard_normal(V) * scale, cast to fp32
  dyadic rows   integers in [0, levels) * 0.25: exact ties inside a row, and sums that tie across beams (raw-logit scoring)
  comb rows     normal rows with +20 on the elements whose float4 index mod 256 is below 2K - 1: the row's leaders all belong to
                2K - 1 threads of the candidate kernel, so the 2K-th best per-thread maximum is low, more than 1024 elements reach
                that bound and the kernel takes its fallback (per-thread sorted lists of the template's width)
  EOS schedule  eos_boost[item][len(prefix)] is added (in fp32) to the EOS logit: hypotheses finish early, late, all at once or never

CASES is the committed list.  Every non-tie case was checked when it was written (and is checked again by
tests/test_beam_ref_cpu.py) to decide every comparison by at least 64 x its own fp32-vs-fp64 score error; a seed that did not was
replaced here, none is filtered at run time."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

V5, LEGACY = 0, 1           # the `mode` of cap_op_beam_init / cap_op_beam_step
PAD = 0


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    seed: int
    mode: int
    B: int
    K: int
    V: int
    max_len: int
    lp: float
    boost: tuple                 # per position (len max_len), or per item a tuple of those
    min_len: int = 0
    kind: str = "normal"         # "normal" | "dyadic" | "comb"
    scale: float = 2.0
    levels: int = 4
    eos: int = 1
    ld: int = 0                  # 0: V rounded up to a multiple of 4, plus 4
    tie: bool = False            # exact ties by construction (no HF record: torch.topk's tie order is not specified)
    what: str = ""

    @property
    def bos(self):
        return 2 if self.V > 2 and self.eos != 2 else 0

    @property
    def row_ld(self):
        return self.ld or (self.V + 3) // 4 * 4 + 4

    @property
    def fill(self):
        """What unwritten positions of the output hold: HF v5 `pad_token_id or eos_token_id`, the legacy scorer the pad id."""
        return PAD if self.mode == LEGACY else (PAD or self.eos)

    def boost_at(self, item, pos):
        b = self.boost[item] if isinstance(self.boost[0], tuple) else self.boost
        return b[pos]


def ramp(L, start, step, first=2):
    """EOS boost `start` at position `first`, growing by `step` per position; -30 (never) before."""
    return tuple(-30.0 if p < first else start + step * (p - first) for p in range(L))


def flat(L, v):
    return tuple(float(v) for _ in range(L))


def spike(L, pos, v, other=-30.0):
    return tuple(float(v) if p == pos else float(other) for p in range(L))


def comb_mask(V, K):
    return (np.arange(V) // 4) % 256 < 2 * K - 1


def elements_at_or_above_the_bound(row, K):
    """What beam_rows_lds_kernel's threshold selection collects for a row of scores (any monotone function of them): thread t
    owns the float4 chunks t, t + 256, ...; tau is the 2K-th best of the 256 per-thread maxima (value, then lower index);
    returns the number of elements at or above tau - more than 1024 sends the kernel to its fallback."""
    V = row.shape[0]
    owner = (np.arange(V) // 4) % 256
    best = []
    for t in range(256):
        idx = np.nonzero(owner == t)[0]
        if idx.size:
            i = idx[np.argmax(row[idx])]            # first maximal: the lower index
            best.append((-float(row[i]), int(i)))
    best.sort()
    if len(best) < 2 * K:
        return V
    tv, ti = -best[2 * K - 1][0], best[2 * K - 1][1]
    return int(np.sum((row > tv) | ((row == tv) & (np.arange(V) <= ti))))


@functools.lru_cache(maxsize=200000)
def _row(case, item, prefix):
    rng = np.random.default_rng([case.seed, item, *prefix])
    if case.kind == "dyadic":
        row = rng.integers(0, case.levels, case.V).astype(np.float32) * np.float32(0.25)
    else:
        row = (rng.standard_normal(case.V) * case.scale).astype(np.float32)
        if case.kind == "comb":
            row[comb_mask(case.V, case.K)] += np.float32(20.0)
    row[case.eos] = row[case.eos] + np.float32(case.boost_at(item, len(prefix)))
    row.setflags(write=False)
    return row


def logits_row(case, item, prefix):
    """fp32 [V], read-only.  prefix: the beam's tokens so far, BOS included."""
    return _row(case, int(item), tuple(int(t) for t in prefix))


def _c(name, seed, mode, B, K, V, L, lp, boost, **kw):
    return Case(name=name, seed=seed, mode=mode, B=B, K=K, V=V, max_len=L, lp=lp, boost=boost, **kw)


CASES = (
    # ---- HF v5 scoring: random rows, every length penalty, every launch branch and template width
    _c("v5_k3_v64_lp1", 101, V5, 3, 3, 64, 10, 1.0, ramp(10, 0.0, 1.5), what="row in LDS, <8>"),
    _c("v5_k2_v1000_lp06", 102, V5, 3, 2, 1000, 12, 0.6, ramp(12, 2.0, 1.0), what="row in LDS, <4>"),
    _c("v5_k4_v1000_lp0", 103, V5, 1, 4, 1000, 9, 0.0, ramp(9, 3.0, 1.0), what="row in LDS, <8>, no length penalty"),
    _c("v5_k5_v30524_lp2", 104, V5, 3, 5, 30524, 8, 2.0, ramp(8, 6.0, 1.5), what="BLIP vocabulary, row in LDS, <16>"),
    _c("v5_k8_v49408_lp1", 105, V5, 1, 8, 49408, 7, 1.0, ramp(7, 8.0, 1.5), eos=49407,
       what="CoCa vocabulary, candidate lists only, <16>, EOS the last id"),
    _c("v5_k1_v2_lp1", 106, V5, 3, 1, 2, 12, 1.0, ramp(12, -3.0, 0.5), scale=1.0, what="K = 1, V = 2K: plain kernel"),
    _c("v5_k1_v64_lp06", 107, V5, 3, 1, 64, 11, 0.6, ramp(11, 0.0, 1.0), what="K = 1"),
    _c("v5_k3_v6_lp1", 108, V5, 3, 3, 6, 9, 1.0, ramp(9, -1.0, 0.5), scale=1.0, what="V = 2K: plain kernel"),
    _c("v5_k8_v16_lp2", 109, V5, 1, 8, 16, 8, 2.0, ramp(8, 0.0, 0.5), scale=1.0, what="V = 2K, K = 8: plain kernel"),
    _c("v5_k3_v1000_ld1003", 110, V5, 3, 3, 1000, 9, 1.0, ramp(9, 2.0, 1.5), ld=1003, what="ld % 4 != 0: plain kernel"),
    _c("v5_k5_v64_lp06", 111, V5, 3, 5, 64, 12, 0.6, ramp(12, 0.0, 1.0), what="<16> on a small row"),
    # ---- HF v5: the shapes of a search
    _c("v5_never_ends", 120, V5, 3, 3, 64, 7, 1.0, flat(7, -30.0), what="max_len reached with open beams"),
    _c("v5_all_eos_step2", 121, V5, 3, 4, 64, 8, 1.0, spike(8, 2, 25.0, other=0.0),
       what="second step: EOS is every beam's best continuation - the K best of the 2K candidates are all EOS"),
    _c("v5_late_displaces", 122, V5, 1, 3, 64, 12, 2.0, (-30.0, -30.0, 4.0, -30.0, -30.0, -30.0, 3.0, 5.0, 7.0, 9.0, 11.0, 13.0),
       what="a late, better hypothesis (length penalty 2) displaces a pool entry"),
    _c("v5_items_differ", 123, V5, 3, 3, 64, 12, 1.0,
       (spike(12, 2, 25.0, other=0.0), ramp(12, 0.0, 1.5, first=5), flat(12, -30.0)),
       what="item 0 stops at once, item 1 late, item 2 never"),
    # ---- legacy CoCa scorer (raw logits, start token in the denominator, is_done on the best candidate)
    _c("legacy_k3_v64_min0_lp06", 201, LEGACY, 3, 3, 64, 10, 0.6, ramp(10, 1.0, 1.0), what="row in LDS, <8>"),
    _c("legacy_k2_v1000_min3_lp2", 202, LEGACY, 3, 2, 1000, 12, 2.0, ramp(12, 6.0, 0.5, first=1), min_len=3,
       what="EOS leads from the first step: MinLength masks it while cur_len < 3"),
    _c("legacy_k5_v49408_min3_lp2", 2040, LEGACY, 3, 5, 49408, 8, 2.0, ramp(8, 8.0, 0.5, first=1), min_len=3, eos=49407,
       what="CoCa's own shape: candidate lists only, <16>"),
    _c("legacy_k1_v64_min0_lp1", 204, LEGACY, 3, 1, 64, 10, 1.0, ramp(10, 2.0, 1.0), what="K = 1"),
    _c("legacy_k4_v8_min3_lp2", 208, LEGACY, 1, 4, 8, 9, 2.0, ramp(9, 1.0, 0.5, first=1), min_len=3, scale=1.0,
       what="V = 2K with a masked EOS: plain kernel, -inf candidates"),
    _c("legacy_k3_v30524_ld30527", 206, LEGACY, 1, 3, 30524, 7, 1.0, ramp(7, 8.0, 1.0), ld=30527, what="ld % 4 != 0: plain kernel"),
    _c("legacy_never_ends", 220, LEGACY, 3, 3, 64, 7, 0.0, flat(7, -30.0), what="max_len reached with open beams"),
    _c("legacy_all_eos_step2", 221, LEGACY, 3, 4, 64, 8, 1.0, spike(8, 2, 25.0, other=0.0), what="as v5_all_eos_step2"),
    _c("legacy_late_displaces", 222, LEGACY, 1, 3, 64, 12, 0.6, (-30.0, -30.0, 6.0, -30.0, -30.0, -30.0, 5.0, 6.0, 7.0, 8.0, 9.0, 10.0),
       what="a late, better hypothesis displaces a pool entry"),
    _c("legacy_items_differ", 223, LEGACY, 3, 3, 64, 12, 2.0,
       (spike(12, 2, 25.0, other=0.0), ramp(12, 4.0, 1.0, first=5), flat(12, -30.0)), what="as v5_items_differ"),
    # ---- the candidate kernel's fallback (more than 1024 elements at its bound), once per list width and row source; raw-logit
    # scoring only: on such rows torch's own fp32 log-softmax is further from fp64 than 8 x this reference's error
    _c("legacy_comb_k5_v30524", 401, LEGACY, 1, 5, 30524, 5, 0.6, ramp(5, 22.0, 1.0), kind="comb", what="fallback, row in LDS, <16>"),
    _c("legacy_comb_k8_v30524", 402, LEGACY, 1, 8, 30524, 5, 1.0, ramp(5, 22.0, 1.0), kind="comb", what="fallback, candidate lists only, <16>"),
    _c("legacy_comb_k4_v49408", 403, LEGACY, 1, 4, 49408, 5, 1.0, ramp(5, 22.0, 1.0), kind="comb", what="fallback, candidate lists only, <8>"),
    _c("legacy_comb_k2_v100000", 404, LEGACY, 1, 2, 100000, 5, 2.0, ramp(5, 22.0, 1.0), kind="comb", what="fallback, candidate lists only, <4>"),
    # ---- exact ties: the order must be the flat-index order (beam-major, then token id)
    _c("v5_tie_rows_k3_v64", 301, V5, 3, 3, 64, 9, 1.0, ramp(9, 0.0, 0.25), kind="dyadic", tie=True,
       what="equal logits inside a row"),
    _c("v5_tie_rows_k4_v1000", 302, V5, 1, 4, 1000, 7, 0.6, ramp(7, 0.0, 0.25), kind="dyadic", tie=True,
       what="equal logits inside a row, hundreds of them"),
    _c("legacy_tie_sums_k4_v64", 303, LEGACY, 3, 4, 64, 9, 1.0, ramp(9, 0.0, 0.25), kind="dyadic", tie=True,
       what="dyadic logits: running sums tie across beams"),
    _c("legacy_tie_sums_k2_v1000_min3", 304, LEGACY, 3, 2, 1000, 8, 2.0, ramp(8, 0.5, 0.25, first=1), kind="dyadic", min_len=3, tie=True,
       what="dyadic logits, MinLength mask, two beams"),
)

BY_NAME = {c.name: c for c in CASES}
