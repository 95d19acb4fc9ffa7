"""Cosine similarity of caption embeddings on the device (csrc/similarity.hip through cap_cosine_matrix / cap_group_similarity).

What the reference computes with torch / sentence-transformers `util.cos_sim`, one object at a time:

    _cosine_distance(embeddings)                 experimenting_env/utils/projection_utils.py   -> group_similarity(...).disagreement
    mean pairwise cosine over i < j per group    scripts/compute_cosine_sim.py                 -> .pair_mean
    its mean and standard deviation              captioner/test_cosine_similarity.py           -> .pair_mean, sqrt(.pair_var)
    diag(cos_sim(proposed, reference))           scripts/compute_performance_measures.py       -> cosine_matrix(a, b, paired=True)

Two deliberate departures from the reference: a zero row has cosine 0 with everything (rows are normalised as F.normalize does, by
max(norm, 1e-12); the reference divides by zero), and duplicates are handled by caption string and count (`weights`), not by
`unique(dim=0)` on the embeddings.  Tensors in, tensors out, all on the device; fp32 arithmetic whatever the encoder's dtype was.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Sequence

import numpy as np
import torch

from . import _native as N

MAX_DIM = 1024


class GroupSimilarity(NamedTuple):
    disagreement: torch.Tensor   # fp32 [G]  mean of 1 - cos over the expanded group's full matrix, diagonal included
    pair_mean: torch.Tensor      # fp32 [G]  mean cosine over the unordered pairs of the expanded group
    pair_var: torch.Tensor       # fp32 [G]  its population variance
    pairs: torch.Tensor          # int64 [G] W (W - 1) / 2
    medoid: torch.Tensor         # int32 [G] row with the largest row_mean (first on ties), -1 for an empty group
    row_mean: torch.Tensor       # fp32 [N]  mean cosine of row i to the other members of its expanded group


def _rows(x: torch.Tensor, what: str) -> torch.Tensor:
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise ValueError(f"{what} must be a [rows, D] tensor")
    if not x.is_cuda:
        raise N.CaptionerHipError(f"{what} is not on the device: the similarity kernels have no host path")
    return x.detach().to(torch.float32).contiguous()


def _call(device, entry: str, *args) -> None:
    lib = N.load_library()
    with torch.cuda.device(device):
        argv = [C.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else a for a in args]
        N.check(getattr(lib, entry)(*argv, C.c_void_p(torch.cuda.current_stream(device).cuda_stream)), entry)


def cosine_matrix(a: torch.Tensor, b: torch.Tensor, paired: bool = False) -> torch.Tensor:
    """cos(a_i, b_j) -> fp32 [Na, Nb]; paired: cos(a_i, b_i) -> fp32 [N], bit for bit the matrix's diagonal."""
    a, b = _rows(a, "a"), _rows(b, "b")
    if a.shape[1] != b.shape[1]:
        raise ValueError(f"a and b differ in width ({a.shape[1]} / {b.shape[1]})")
    if paired and a.shape[0] != b.shape[0]:
        raise ValueError(f"paired similarity needs as many rows in a as in b ({a.shape[0]} / {b.shape[0]})")
    Na, Nb, D = a.shape[0], b.shape[0], a.shape[1]
    out = torch.empty((Na,) if paired else (Na, Nb), dtype=torch.float32, device=a.device)
    ws = torch.empty((max(Na + Nb, 4),), dtype=torch.float32, device=a.device)
    _call(a.device, "cap_cosine_matrix", a, b, Na, Nb, D, int(bool(paired)), out, ws, C.c_size_t(ws.numel() * 4))
    return out


def group_similarity(embeddings: torch.Tensor, offsets: Sequence[int], weights: torch.Tensor | None = None) -> GroupSimilarity:
    """embeddings [N, D] on the device; group g = rows offsets[g] .. offsets[g + 1] (host sequence of G + 1 ints: 0 first, N last,
    non-decreasing); weights [N] positive integer counts (None = ones): every statistic is that of the group with row i repeated
    weights[i] times."""
    e = _rows(embeddings, "embeddings")
    off = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64))
    if off.ndim != 1 or off.size < 1:
        raise ValueError("offsets must hold G + 1 row bounds")
    if off.size and (off.min() < -2 ** 31 or off.max() >= 2 ** 31):
        raise ValueError("offsets do not fit 32 bits")
    off = off.astype(np.int32)
    N_, D, G = e.shape[0], e.shape[1], off.size - 1
    w = None
    if weights is not None:
        w = torch.as_tensor(weights).detach().to(device=e.device, dtype=torch.float32).contiguous()
        if w.shape != (N_,):
            raise ValueError(f"weights must be [{N_}], got {tuple(w.shape)}")
    lib = N.load_library()
    off_p = off.ctypes.data_as(C.c_void_p)
    need = lib.cap_group_similarity_workspace(N_, G, D, off_p)
    if need == 0:
        raise N.CaptionerHipError(f"cap_group_similarity_workspace failed: {N.last_error()}")
    dev = e.device
    ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    f32 = lambda n: torch.empty((n,), dtype=torch.float32, device=dev)  # noqa: E731
    out = GroupSimilarity(f32(G), f32(G), f32(G), torch.empty((G,), dtype=torch.int64, device=dev),
                          torch.empty((G,), dtype=torch.int32, device=dev), f32(N_))
    _call(dev, "cap_group_similarity", e, off_p, w, N_, G, D, out.disagreement, out.pair_mean, out.pair_var, out.pairs, out.medoid,
          out.row_mean, ws, C.c_size_t(need))
    return out


def caption_groups(freq: dict):
    """The output of `distributed.captions_frequency` ({key: [[count, caption], ...]}) -> (keys, sentences, offsets, weights): every
    DISTINCT caption of every group once, in first-seen order, groups in the dict's order; offsets has len(keys) + 1 entries and an
    empty group is an empty range; weights are the counts.  Pure host work."""
    keys, sentences, offsets, weights = [], [], [0], []
    for key, lst in freq.items():
        seen = {}
        for n, cap in lst:
            n = int(n)
            if n < 1:
                raise ValueError(f"caption {cap!r} of {key!r} has count {n}")
            if cap in seen:
                weights[seen[cap]] += n
            else:
                seen[cap] = len(sentences)
                sentences.append(cap)
                weights.append(n)
        keys.append(key)
        offsets.append(len(sentences))
    return keys, sentences, offsets, weights
