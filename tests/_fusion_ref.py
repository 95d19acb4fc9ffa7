"""float64 restatement of the probability fusion, written from its definition, for the vocab-fusion tests:

    p_t(i)  = softmax(z_t)(i)                         per decode step t of a caption (a masked / -inf entry gives 0)
    m(i)    = max_t p_t(i)                            per caption
    mean(i) = sum over the group's captions of m(i) / n
    kept    = { i : mean(i) > th }, ascending

and the bars the tests use: for a probability, the larger of 8 x torch-fp32-CPU softmax's own error against float64 on the same
rows and 4 fp32 spacings at the value; for the threshold, a band of 4 fp32 spacings of th around th in which a float64 mean decides
nothing (the inputs are built so that no mean falls inside it)."""
import numpy as np
import torch


def softmax64(rows32: torch.Tensor) -> np.ndarray:
    """fp32 [n, V] host rows -> float64 softmax per row (rows may hold -inf, never only -inf)."""
    x = rows32.double().numpy()
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def spacing32(v) -> np.ndarray:
    """fp32 spacing at |v| (float64 array); at 0 the smallest normal's spacing does not matter: callers take a max with it."""
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def prob_bar(rows32: torch.Tensor, want: np.ndarray):
    """-> (bar per value, shaped like want [n, V] or broadcastable; ref_err): 8 x the maximal error of torch float32 softmax on the
    CPU against float64 over these rows, or 4 fp32 spacings at the value, whichever is larger."""
    ref32 = torch.softmax(rows32, dim=-1).double().numpy()
    ref_err = float(np.abs(ref32 - softmax64(rows32)).max())
    return np.maximum(8.0 * ref_err, 4.0 * spacing32(want)), ref_err


def group_mean64(acc64: np.ndarray, members) -> np.ndarray:
    return acc64[list(members)].sum(axis=0) / float(len(members))


def threshold_band(th: float) -> float:
    return 4.0 * float(spacing32(np.float32(th)))


def kept64(mean64: np.ndarray, th: float) -> np.ndarray:
    return np.nonzero(mean64 > float(np.float32(th)))[0]


def assert_no_mean_in_band(mean64: np.ndarray, th: float) -> float:
    """The threshold condition: no float64 mean within 4 fp32 spacings of th (th as the fp32 the kernel receives).  -> the margin."""
    margin = float(np.abs(mean64 - float(np.float32(th))).min())
    assert margin > threshold_band(th), (margin, threshold_band(th))
    return margin
