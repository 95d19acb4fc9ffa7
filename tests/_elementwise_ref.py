"""Host references of the helper kernels in csrc/elementwise.hip (tests/test_elementwise_kernels_gpu.py): plain numpy / torch,
float64 where the kernel rounds, bit patterns where it only moves or encodes values.  tests/test_elementwise_ref_cpu.py pins
these against torch.nn.functional and numpy where there is no GPU.  Never imported by the product package."""
import numpy as np
import torch

from _util import g8_encode

U = 2.0 ** -24                        # fp32 unit roundoff
NAN32, NAN16 = 0x7FC00000, 0x7FC0     # the NaN sentinels of fp32 / bf16 outputs as bit patterns
ODD = 0x5A5A5A5B                      # the sentinel of int32 outputs and G8 containers (an odd word; halves 0x5A5B | 0x5A5A)
KIND = {"f32": "f32", "bf16": "bf16", "f32s": "g8"}      # test dtype name -> storage kind of the operand output


def sentinel(kind):
    return {"f32": NAN32, "bf16": NAN16, "g8": ODD, "i32": ODD}[kind]


def np_int(kind):
    return np.int16 if kind == "bf16" else np.int32


def _as_signed(v, dt):
    return np.array(v, dtype=np.uint16 if dt == np.int16 else np.uint32).astype(dt)


def encode(kind, x, ld=None):
    """fp32 values [rows, cols] -> the bit image of a [rows, ld] buffer of `kind` that held sentinels and had its first `cols`
    columns of every row stored (int32 words, int16 for bf16).  G8: ld % 8 == 0; a group cut by `cols` keeps sentinel halves."""
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float32))
    rows, cols = x.shape
    ld = cols if ld is None else ld
    dt = np_int(kind)
    out = np.full((rows, ld), _as_signed(sentinel(kind), dt), dtype=dt)
    if kind == "f32":
        out[:, :cols] = x.view(np.int32)
    elif kind == "bf16":
        out[:, :cols] = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy()
    else:
        assert ld % 8 == 0
        full = np.zeros((rows, ld), dtype=np.float32)
        full[:, :cols] = x
        img = g8_encode(full).view(np.int16).reshape(rows, ld // 8, 2, 8)
        keep = (np.arange(ld) < cols).reshape(1, ld // 8, 1, 8)
        halves = out.view(np.int16).reshape(rows, ld // 8, 2, 8)
        out = np.ascontiguousarray(np.where(keep, img, halves)).view(np.int32).reshape(rows, ld)
    return out


def layernorm64(y, gamma, beta, eps):
    """two-pass LayerNorm of fp32 rows in float64 (biased variance, eps inside the root)"""
    y = np.asarray(y, dtype=np.float64)
    mu = y.mean(-1, keepdims=True)
    var = ((y - mu) ** 2).mean(-1, keepdims=True)
    return (y - mu) / np.sqrt(var + eps) * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64)


def embed_sum32(word, pos, tok, t):
    """word[tok] + pos[t] as one fp32 add per element; tok int [R]"""
    return (word[np.asarray(tok)] + pos[t][None, :]).astype(np.float32)


def embed_tokens_sum32(word, pos, type0, ids, L):
    """(word[clamp(id)] + type0) + pos[r % L] in fp32, in that order"""
    V = word.shape[0]
    tok = np.clip(np.asarray(ids, dtype=np.int64), 0, V - 1)
    l = np.arange(len(tok)) % L
    return ((word[tok] + type0[None, :]).astype(np.float32) + pos[l]).astype(np.float32)


def init_prompt_seq(R, L, prompt, V, pad):
    """prompt int [rows, P], rows 1 or R -> (seq [R, L], finished [R], lengths [R])"""
    prompt = np.asarray(prompt)
    P = prompt.shape[1]
    seq = np.full((R, L), pad, dtype=np.int32)
    seq[:, :P] = np.clip(np.broadcast_to(prompt, (R, P)).astype(np.int64), 0, V - 1)
    return seq, np.zeros(R, np.int32), np.full(R, L, np.int32)


def reduce_bias_act32(part, bias, act):
    """((part[0] + part[1]) + ...) + bias in fp32, then ReLU for act 2"""
    s = part[0].astype(np.float32).copy()
    for z in range(1, part.shape[0]):
        s = (s + part[z]).astype(np.float32)
    if bias is not None:
        s = (s + bias[None, :]).astype(np.float32)
    return np.maximum(s, np.float32(0)) if act == 2 else s


# c of the bound below: a mean over n rows is n - 1 additions, the rounding of 1 / n and one multiplication = n + 1 roundings; one
# more covers every second-order term (n <= 128: (1 + u)^(n + 1) - 1 - (n + 1) u < 1e-4 u)
MEAN_POOL_C = 2
# the normalisation after it: the squares (1 rounding), their sum (3 additions in the thread, 6 wave steps, 3 across the waves;
# non-negative terms, so the relative errors do not amplify) = 13 roundings, halved by the root, + the root + the division < 9 u;
# 16 u with the second-order terms and a contracted multiply-add either way
MEAN_POOL_NORM_U = 16


def mean_pool_normalize64(x, lens):
    """x fp32 [B, L, D], lens int [B] (clamped to [1, L]) -> (float64 [B, D] normalised means, the bound on an fp32 kernel's
    absolute error [B, D]).  The fp32 sequential sum of n terms then the scaling by 1 / n is within
    e_c = (n + MEAN_POOL_C) 2^-24 sum_l |x_lc| / n of the mean m_c; dividing by the norm of the computed vector carries that to
    (e_c + |o_c| ||e||_2) / ||m||  (o = m / ||m||: the first term is the numerator's error, the second the norm's, which moves by
    at most ||e||_2), plus MEAN_POOL_NORM_U 2^-24 |o_c| for the norm's own arithmetic and the division."""
    x = np.asarray(x, dtype=np.float64)
    B, L, D = x.shape
    out, bound = np.zeros((B, D)), np.zeros((B, D))
    for b in range(B):
        n = min(max(int(lens[b]), 1), L)
        m = x[b, :n].sum(0) / n
        e = (n + MEAN_POOL_C) * U * np.abs(x[b, :n]).sum(0) / n
        nrm = max(np.sqrt((m * m).sum()), 1e-12)
        out[b] = m / nrm
        bound[b] = (e + np.abs(out[b]) * np.sqrt((e * e).sum())) / nrm + MEAN_POOL_NORM_U * U * np.abs(out[b])
    return out, bound


def patch_gather(x, ps):
    """[B, 3, img, img] -> [B * G * G, 3 ps^2]: row b G^2 + py G + px, column c ps^2 + dy ps + dx (a pure rearrangement)"""
    B, C3, img, _ = x.shape
    G = img // ps
    return np.ascontiguousarray(x.reshape(B, C3, G, ps, G, ps).transpose(0, 2, 4, 1, 3, 5)).reshape(B * G * G, C3 * ps * ps)


def normalise_u8_64(u8, mean, std):
    """uint8 [B, img, img, 3] -> (float64 [B, 3, img, img] = (u / 255 - mean[c]) / std[c] with the fp32 mean / std as given, the
    bound on an fp32 kernel's absolute error).  t = u / 255 <= 1 reaches the subtraction through the rounded constant 1 / 255 and
    the product (2 u t <= 2 u, one rounding fewer if the compiler contracts the multiply-subtract), the subtraction rounds once
    (u |t - mean| <= u for a mean inside [0, 1]): three roundings of size u in front of the division, which scales them by 1 / std
    and adds its own u |v|."""
    mean, std = np.asarray(mean, np.float32).astype(np.float64), np.asarray(std, np.float32).astype(np.float64)
    v = (u8.astype(np.float64) / 255.0 - mean) / std
    bound = 3 * U / std + U * np.abs(v)
    return np.ascontiguousarray(v.transpose(0, 3, 1, 2)), np.ascontiguousarray(np.broadcast_to(bound, v.shape).transpose(0, 3, 1, 2))


def store_error(kind, v):
    """what a store in the operand type adds to a value v: nothing, bf16's half ulp 2^-8 |v| (8 significant bits), or G8's: lo = rn16(v - hi) keeps 11
    bits of a residue <= 2^-11 |v| (2^-22 |v|), or sits in fp16's subnormal grid (spacing 2^-24: 2^-25)."""
    v = np.abs(v)
    return {"f32": 0.0 * v, "bf16": 2.0 ** -8 * v, "g8": 2.0 ** -22 * v + 2.0 ** -25}[kind]


def compact_rows(finished):
    return np.flatnonzero(np.asarray(finished) == 0).astype(np.int32)


def absmax_bits(x):
    """bit pattern of max |x| (fp32); any NaN -> None (the kernel then returns a pattern above +inf's)"""
    x = np.asarray(x, dtype=np.float32)
    if np.isnan(x).any():
        return None
    return int(np.abs(x).max().view(np.uint32))


def greedy_expected(logits, V, eos, mask_eos):
    """the documented selection (csrc/ops.h): torch.argmax of the row's first V entries with EOS at -inf while masked and every
    NaN standing as -inf - first maximal index, 0 when nothing is above -inf"""
    z = torch.as_tensor(np.asarray(logits, dtype=np.float32))[:, :V].clone()
    if mask_eos:
        z[:, eos] = float("-inf")
    z[torch.isnan(z)] = float("-inf")
    return torch.argmax(z, dim=-1).numpy().astype(np.int32)
