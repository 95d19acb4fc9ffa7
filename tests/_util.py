"""Shared helpers for the GPU parity tests (never imported by the product package)."""
import ctypes as C
import json
import os

import numpy as np
import torch

from embodied_captioning_amd.config import BlipArch
from embodied_captioning_amd.weights import procedural_blip_state_dict, synthetic_pixels

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    meta = json.loads(str(g["meta"]))
    arch = BlipArch(**meta["arch"])
    return g, meta, arch


_SD_CACHE = {}


def golden_inputs(name):
    """(golden, meta, arch, state_dict, pixels) - the state dict is cached per fixture."""
    g, meta, arch = load_golden(name)
    key = (name, meta["seed"], meta["eos_boost"])
    if key not in _SD_CACHE:
        _SD_CACHE[key] = procedural_blip_state_dict(arch, meta["seed"], eos_boost=meta["eos_boost"])
    px = synthetic_pixels(meta["batch"], arch.image_size, seed=meta["seed"])
    return g, meta, arch, _SD_CACHE[key], px


_COCA_SD_CACHE = {}


def coca_golden(name, part=""):
    """A CoCa fixture of tools/make_goldens_coca.py -> (values with the `part` prefix stripped, meta, arch, state dict,
    pixels).  The state dict is the one the library loads (coca_library_state_dict: derived tensors added, the position
    table resized from `weights_image_size` to the arch's input size); it is cached per fixture."""
    import dataclasses
    from embodied_captioning_amd.coca_weights import coca_library_state_dict
    from embodied_captioning_amd.config import CocaArch
    from embodied_captioning_amd.weights import procedural_coca_state_dict
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    vals = {k[len(part):]: g[k] for k in g.files if k.startswith(part)}
    meta = json.loads(str(vals["meta"]))
    arch = CocaArch(**meta["arch"])
    key = (name, meta["seed"], meta["eos_boost"])
    if key not in _COCA_SD_CACHE:
        _COCA_SD_CACHE.clear()                          # full-size dicts are GBs: keep one
        wa = dataclasses.replace(arch, image_size=meta["weights_image_size"])
        _COCA_SD_CACHE[key] = coca_library_state_dict(procedural_coca_state_dict(wa, meta["seed"], eos_boost=meta["eos_boost"]), arch)
    px = synthetic_pixels(meta["batch"], arch.image_size, seed=meta["seed"])
    return vals, meta, arch, _COCA_SD_CACHE[key], px


def strided(x, stride):
    """[B, ...] -> every `stride`-th value of each row, the layout of the fixtures' *_sample arrays."""
    x = np.asarray(x)
    return x.reshape(x.shape[0], -1)[:, ::int(stride)]


def pad_to(seq, L, fill):
    """HF crops generated sequences at the longest row; our ABI returns [B, max_len]."""
    seq = np.asarray(seq)
    if seq.shape[1] == L:
        return seq
    out = np.full((seq.shape[0], L), fill, dtype=seq.dtype)
    out[:, : seq.shape[1]] = seq
    return out


def token_parity(ours, ref, margins, tau):
    """Greedy-token comparison that knows about near-ties.

    ours/ref: int [B, L] incl. BOS.  margins: fp32 [L-1, B] oracle top1-top2 logit gap at each step.
    A row may leave the oracle's path only at a step whose oracle margin is below `tau`; after that step
    the row is on a different (equally valid) prefix and is not compared further.
    Returns (n_exact_rows, n_diverged_rows, first_bad) - first_bad is None when every divergence was at a near-tie.
    """
    B, L = ref.shape
    exact = diverged = 0
    first_bad = None
    for b in range(B):
        row_ok = True
        for s in range(1, L):
            if ours[b, s] != ref[b, s]:
                row_ok = False
                m = margins[s - 1, b] if s - 1 < margins.shape[0] else 0.0
                if not (m < tau) and first_bad is None:
                    first_bad = (b, s, int(ours[b, s]), int(ref[b, s]), float(m))
                break
        exact += row_ok
        diverged += (not row_ok)
    return exact, diverged, first_bad


# ---- G8: the GEMM-operand layout of the split-fp16 mode (embodied_captioning_amd/csrc/common.h) ----------------------
G8_WSCALE = 4096.0


def g8_encode(x, scale=1.0):
    """fp32 [..., K] (K % 8 == 0) -> float32-typed container of the same shape whose bytes are the G8 image: every 8
    consecutive elements of a row = [8 fp16 hi | 8 fp16 lo], hi = rn16(s x), lo = rn16(s x - hi)."""
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float32)) * np.float32(scale)
    x = np.clip(x, -65000.0, 65000.0).astype(np.float32)     # G8_AMAX: the device clamps to fp16's range the same way
    assert x.shape[-1] % 8 == 0
    hi = x.astype(np.float16)
    lo = (x - hi.astype(np.float32)).astype(np.float16)
    g = np.stack([hi.reshape(*x.shape[:-1], -1, 8), lo.reshape(*x.shape[:-1], -1, 8)], axis=-2)   # [..., K/8, 2, 8]
    return np.ascontiguousarray(g).view(np.float32).reshape(x.shape)


def g8_decode(c, scale=1.0):
    """Inverse of g8_encode: container (float32-typed, [..., K]) -> the fp32 values hi + lo (divided by scale)."""
    c = np.ascontiguousarray(np.asarray(c, dtype=np.float32))
    h = c.view(np.float16).reshape(*c.shape[:-1], -1, 2, 8).astype(np.float32)
    return ((h[..., 0, :] + h[..., 1, :]) / np.float32(scale)).reshape(c.shape)


# ---- operands of the single-kernel entry points (cap_op_*): dt is "f32", "bf16" or "f32s" (split mode: fp32 values, G8 operands) ----
NAN = float("nan")


def ptr(t):
    return t.data_ptr() if t is not None else None


def cur_stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def check_rc(lib, rc):
    assert rc == 0, lib.cap_last_error().decode()


def att_dtype(dt):
    """element type of q / k / v and the caches of the attention kernels (split mode: fp32)"""
    return torch.bfloat16 if dt == "bf16" else torch.float32


def nan_buf(dt, *shape):
    """NaN words of the operand's width (a G8 container is 4 bytes per element: a NaN word decodes to NaN)"""
    return torch.full(shape, NAN, dtype=att_dtype(dt), device="cuda")


def nan_f32(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device="cuda")


def same_bits(a, b):
    """torch.equal on the bytes (a G8 container's words are not numbers)"""
    it = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return a.shape == b.shape and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def finish32(part, bias):
    """Part8::finish / the cross kernel's q: the slices in order, then the bias, in fp32"""
    s = part[0].clone()
    for z in range(1, part.shape[0]):
        s = s + part[z]
    return s + bias


def operand_values(dt, t, scale=1.0):
    """device operand -> its float64 values (a NaN container decodes to NaN)"""
    if dt != "f32s":
        return t.cpu().double()
    return torch.from_numpy(g8_decode(t.cpu().contiguous().numpy(), scale)).double()


# ---- int8 weights (csrc/gemm_skinny.hip): row-quantised signed bytes in MFMA fragment order + fp32 row scales -------------------------
def i8_pack(lib, N, w):
    """fp32 device matrix -> (packed bytes, row scales) through cap_op_quant_i8_pack"""
    rows, cols = w.shape
    packed = torch.empty(rows * cols, dtype=torch.uint8, device="cuda")
    scale = torch.empty(rows, dtype=torch.float32, device="cuda")
    N.check(lib.cap_op_quant_i8_pack(C.c_void_p(w.data_ptr()), C.c_void_p(packed.data_ptr()), C.c_void_p(scale.data_ptr()), rows, cols, cur_stream()),
            "cap_op_quant_i8_pack")
    return packed, scale


def i8_unpack(packed, rows, cols):
    """fragment order -> [rows, cols] int8: block (t, s) of 1 KiB, lane r + 16 g owns 16 bytes = k-step 0 (8) then k-step 1 (8)"""
    b = packed.view(torch.int8).cpu().view(rows // 16, cols // 64, 4, 16, 2, 8)           # t, s, g, r, ks, e
    return b.permute(0, 3, 1, 4, 2, 5).reshape(rows, cols)                               # (t, r), (s, ks, g, e)


def i8_pack_host(q):
    """the inverse of i8_unpack on the host: int8 [rows, cols] -> the fragment-ordered bytes (uint8 [rows * cols])"""
    rows, cols = q.shape
    b = q.reshape(rows // 16, 16, cols // 64, 2, 4, 8).permute(0, 2, 4, 1, 3, 5)          # (t, r), (s, ks, g, e) -> t, s, g, r, ks, e
    return b.contiguous().view(torch.uint8).reshape(-1)


# ---- KV16: the split mode's cross-attention K/V cache layout (embodied_captioning_amd/csrc/common.h) ------------------
def kv16_unpack(raw, rows):
    """bytes of a KV16 block -> (int16 [rows, 64], fp32 scales [rows]); groups of 32 rows = 32 x 128 B then 32 scales."""
    g = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 4224)
    q = g[:, :4096].reshape(-1, 128).view(np.int16)[:rows]
    sc = g[:, 4096:].reshape(-1, 128).view(np.float32).reshape(-1)[:rows]
    return q.copy(), sc.copy()
