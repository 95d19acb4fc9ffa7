#!/usr/bin/env python
"""A/B of the MFMA ViT attention kernels between two builds of the library (GPU box only): the in-tree one and
embodied_captioning_amd/lib/libcaptioner_old.so (a copy of an earlier build), both loaded into this process.  Walks a table of
cases that reaches every instantiation of the seven kernels; the outputs of every case are compared bit for bit.  The timed cases
(the workloads' shapes) run in interleaved rounds, so both sides see the same clocks; median and min per side, and the spread of
the old side's own rounds - the yardstick for "level".    python tools/ab_vit_attention.py [> profiles/<name>.txt]"""
import ctypes as C, os, statistics, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from embodied_captioning_amd import _native
new = _native.load_library()
OLD = os.path.join(ROOT, "embodied_captioning_amd", "lib", "libcaptioner_old.so")
if not os.path.exists(OLD):
    sys.exit(f"{OLD} is missing: build the earlier revision and copy its libcaptioner_hip.so there first")
old = C.CDLL(OLD)
for lib in (old, new):
    lib.cap_last_error.restype = C.c_char_p
    for f, n_int in ((lib.cap_op_vit_attention, 4), (lib.cap_op_vit_attention_hd, 5)):
        f.restype = C.c_int
        f.argtypes = [C.c_int, C.c_void_p, C.c_void_p] + [C.c_int] * n_int + [C.c_void_p]
s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
F32, BF16, SPLIT = 0, 1, 2

# (kernel reached, dtype, q|k|v as "f32" / "bf16" / "g8", B, N, H, head_dim, impl)     impl: 2 = MFMA, 3 = G8 in, 5 = G8 in and the
# per-unit kernel, + 8 = causal
BITS = [("mfma<1>", BF16, "bf16", 2, 32, 2, 64, 2), ("mfma<2>", BF16, "bf16", 2, 33, 2, 64, 2), ("mfma<2>", BF16, "bf16", 2, 64, 2, 64, 2),
        ("mfma<7>", BF16, "bf16", 2, 193, 2, 64, 2), ("mfma<7>", BF16, "bf16", 2, 224, 2, 64, 2), ("mfma<9>", BF16, "bf16", 2, 288, 2, 64, 2),
        ("mfma<9>", BF16, "bf16", 2, 257, 2, 64, 2), ("flash<19,5>", BF16, "bf16", 2, 608, 2, 64, 2), ("flash<19,5>", BF16, "bf16", 2, 577, 2, 64, 2),
        ("flash_wide<9,5>", BF16, "bf16", 2, 288, 2, 88, 0), ("flash_wide<9,5>", BF16, "bf16", 2, 257, 2, 128, 0),
        ("flash_wide<9,5> causal", BF16, "bf16", 2, 257, 2, 88, 8), ("flash_wide<2,2>", BF16, "bf16", 2, 64, 2, 88, 0),
        ("flash_wide<2,2> causal", BF16, "bf16", 2, 32, 2, 80, 8), ("flash_wide<2,2> causal", BF16, "bf16", 2, 33, 2, 80, 8)]
for dt, to in ((F32, "float"), (SPLIT, "g8")):
    BITS += [(f"f32_mfma<{kb},{to}>", dt, "f32", 2, n, 2, 64, 0) for kb, n in ((1, 32), (1, 17), (7, 224), (7, 197), (9, 288), (9, 257))]
    BITS += [(f"f32_mfma_wide<3,{ndb},{to}>", dt, "f32", 2, n, 2, hd, 0) for ndb, n, hd in ((1, 96, 32), (2, 97, 48), (3, 97, 72), (3, 96, 88),
                                                                                            (3, 192, 96), (3, 257, 88))]
BITS += [("split<2,1>", SPLIT, "g8", 2, 64, 2, 64, 3), ("split<2,1>", SPLIT, "g8", 2, 17, 2, 64, 3), ("split<7,1>", SPLIT, "g8", 2, 65, 2, 64, 3),
         ("split<7,1>", SPLIT, "g8", 2, 192, 2, 64, 3), ("split<7,1,1>", SPLIT, "g8", 2, 197, 2, 64, 3), ("split<7,1,1>", SPLIT, "g8", 2, 224, 2, 64, 3),
         ("split<4,0>", SPLIT, "g8", 2, 256, 2, 64, 3), ("split<4,0>", SPLIT, "g8", 2, 384, 2, 64, 3), ("split<4,0>", SPLIT, "g8", 2, 385, 2, 64, 3),
         ("split<4,0>", SPLIT, "g8", 2, 577, 2, 64, 3), ("split_pw<7>", SPLIT, "g8", 43, 197, 6, 64, 3), ("split_pw<7>", SPLIT, "g8", 300, 193, 1, 64, 3),
         ("split_pw<7>", SPLIT, "g8", 65, 224, 4, 64, 3)]
TIMED = [("split_pw<7>", SPLIT, "g8", 256, 197, 12, 64, 3), ("split<7,1,1>", SPLIT, "g8", 256, 197, 12, 64, 5),
         ("mfma<7>", BF16, "bf16", 256, 197, 12, 64, 2), ("mfma<9>", BF16, "bf16", 64, 257, 16, 64, 2),
         ("flash_wide<9,5>", BF16, "bf16", 32, 257, 16, 88, 0), ("f32_mfma_wide<3,3,float>", F32, "f32", 32, 257, 16, 88, 0),
         ("f32_mfma_wide<3,3,g8>", SPLIT, "f32", 32, 257, 16, 88, 0), ("flash<19,5>", BF16, "bf16", 64, 577, 16, 64, 2),
         ("f32_mfma<7,float>", F32, "f32", 64, 197, 12, 64, 0), ("f32_mfma<7,g8>", SPLIT, "f32", 64, 197, 12, 64, 0),
         ("f32_mfma<9,float>", F32, "f32", 32, 257, 16, 64, 0), ("split<7,1>", SPLIT, "g8", 64, 160, 12, 64, 3),
         ("split<4,0>", SPLIT, "g8", 64, 577, 16, 64, 3), ("split<2,1>", SPLIT, "g8", 256, 50, 12, 64, 3),
         ("mfma<2>", BF16, "bf16", 256, 50, 12, 64, 2), ("flash_wide<2,2> causal", BF16, "bf16", 64, 33, 32, 80, 8)]


def inputs(case):
    _, dt, form, B, N, H, hd, impl = case
    g = torch.Generator().manual_seed(N * 131 + hd + B)
    x = (torch.randn(B * N, 3 * H * hd, generator=g) * 1.5).cuda()
    if form == "bf16":
        return x.to(torch.bfloat16)
    if form == "g8":
        g8 = torch.empty_like(x)
        assert new.cap_op_convert(SPLIT, C.c_void_p(x.data_ptr()), C.c_void_p(g8.data_ptr()), x.numel(), s) == 0
        return g8
    return x


def launch(lib, case, qkv, ctx):
    _, dt, form, B, N, H, hd, impl = case
    if form == "g8":        # G8 q|k|v go through the entry point that knows impl 3 / 5
        return lib.cap_op_vit_attention(dt, C.c_void_p(qkv.data_ptr()), C.c_void_p(ctx.data_ptr()), B, N, H, impl, s)
    return lib.cap_op_vit_attention_hd(dt, qkv.data_ptr(), ctx.data_ptr(), B, N, H, hd, impl, s)


def outputs(case, qkv):
    _, dt, form, B, N, H, hd, impl = case
    outs = []
    for lib in (old, new):
        ctx = torch.full((B * N, H * hd), float("nan"), dtype=torch.bfloat16 if form == "bf16" else torch.float32, device="cuda")
        assert launch(lib, case, qkv, ctx) == 0, (case, lib.cap_last_error())
        torch.cuda.synchronize()
        outs.append(ctx)
    return outs


bad = 0
for case in BITS + TIMED:
    a, b = outputs(case, inputs(case))
    raw = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
    same = torch.equal(a.view(raw), b.view(raw))         # raw bits: a G8 word is no number, and NaN left in a buffer must match too
    bad += not same
    print("%-26s dtype %d B %3d N %3d H %2d hd %3d impl %d   %s" % (case[0], case[1], *case[3:], "bit-equal" if same else "DIFFERENT"))
print("cases: %d, different: %d" % (len(BITS) + len(TIMED), bad))

ROUNDS, ITERS = 9, 20
print("\ntimed, %d interleaved rounds of %d launches after one untimed round (clocks, caches), us per launch: median (min) per side; "
      "spread = (max - min) / median of the old side's rounds" % (ROUNDS, ITERS))
for case in TIMED:
    qkv = inputs(case)
    ctxs = outputs(case, qkv)
    t = {0: [], 1: []}
    for rep in range(-1, ROUNDS):
        for side, lib in enumerate((old, new)):
            for _ in range(3): launch(lib, case, qkv, ctxs[side])
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(ITERS): launch(lib, case, qkv, ctxs[side])
            e1.record(); torch.cuda.synchronize()
            if rep >= 0: t[side].append(e0.elapsed_time(e1) * 1e3 / ITERS)
    mo, mn = statistics.median(t[0]), statistics.median(t[1])
    print("%-26s B %3d N %3d H %2d hd %3d   old %8.1f (%8.1f)   new %8.1f (%8.1f)   new/old %.3f   old spread %.1f %%"
          % (case[0], *case[3:7], mo, min(t[0]), mn, min(t[1]), mn / mo, 100 * (max(t[0]) - min(t[0])) / mo))
sys.exit(1 if bad else 0)
