"""Build-time ISA check of the lane = query attention kernels (csrc/attention.hip, csrc/blip2_itm.hip).  They keep a query's `qv[HDP]`
and `o[HDP]` rows in registers by design (252 VGPRs for itm_self_attention_kernel); a toolchain bump that spills them turns
every key's fma chain into scratch traffic without failing any numerical test.  So the generated code is read: no instantiation may
have a private segment - except the ones named in SPILLS, asserted with their byte counts so that they cannot grow unnoticed.
The same for the seven MFMA ViT attention kernels, which keep a query tile's scores and context in accumulators (several of them
within a few registers of their limit) and are assembled from the shared steps of csrc/vit_attn_frag.h.
No GPU needed (hipcc cross-compiles)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("itm_self_attention_kernel", "generic_attention_kp_kernel", "generic_attention_kernel", "text_attention_kernel",
           "pool_attention_kernel")
VIT_KERNELS = ("vit_attention_mfma", "vit_attention_flash", "vit_attention_flash_wide", "vit_attention_f32_mfma",
               "vit_attention_f32_mfma_wide", "vit_attention_split", "vit_attention_split_pw")
# mangled-name fragment -> private_segment_fixed_size in bytes, for instantiations that are known to spill
SPILLS = {"24vit_attention_flash_wideILi9ELi5EE": 148}      # BLIP-2's ViT-g (88-wide heads, 257 tokens): 512 registers and 36 more


@pytest.fixture(scope="module")
def attention_asm(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    from embodied_captioning_amd.build import FLAGS
    flags = [f for f in FLAGS if f != "-fPIC"]
    text = ""
    for src in ("attention.hip", "blip2_itm.hip"):
        out = tmp_path_factory.mktemp("isa") / (src + ".s")
        r = subprocess.run([hipcc, *flags, "-S", "--cuda-device-only", os.path.join(ROOT, "embodied_captioning_amd", "csrc", src), "-o", str(out)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        text += out.read_text()
    return text


def _private_segments(asm):
    """mangled kernel name -> private_segment_fixed_size, from the .amdhsa_kernel blocks."""
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm, flags=re.S):
        seg = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2))
        assert seg, m.group(1)
        out[m.group(1)] = int(seg.group(1))
    return out


def _is(name, kernel):
    return re.search(r"\d+" + kernel + r"I", name) is not None       # Itanium mangling: <length><name>I<template args>


def _count_and_check(segs, kernels, what):
    """instantiations seen per kernel; every one without a private segment, or with exactly its recorded one"""
    seen = {k: 0 for k in kernels}
    unused = {frag: size for frag, size in SPILLS.items() if any(_is(frag, k) for k in kernels)}
    for name, size in sorted(segs.items()):
        for k in kernels:
            if not _is(name, k):
                continue
            seen[k] += 1
            hit = [frag for frag in SPILLS if frag in name]
            if hit:
                assert size == SPILLS[hit[0]], (name, size, "the recorded spill changed")
                unused.pop(hit[0], None)
            else:
                assert size == 0, (name, size, what)
    assert not unused, ("recorded spills that no longer exist", unused)
    return seen


def test_lane_per_query_attention_kernels_keep_their_rows_in_registers(attention_asm):
    seen = _count_and_check(_private_segments(attention_asm), KERNELS, "spills its query / output rows to scratch")
    # bf16, fp32 and G8-output forms: 3 of the scorer's kernel, 6 four-wave (HDP 32, 64), 12 lane = query (HDP 32..128), 4 text, 6 pooler
    assert seen == {"itm_self_attention_kernel": 3, "generic_attention_kp_kernel": 6, "generic_attention_kernel": 12,
                    "text_attention_kernel": 4, "pool_attention_kernel": 6}, seen


def test_mfma_vit_attention_kernels_keep_their_tiles_in_registers(attention_asm):
    seen = _count_and_check(_private_segments(attention_asm), VIT_KERNELS, "spills its score / context accumulators to scratch")
    # mfma<1, 2, 7, 9>; flash<19, 5>; flash_wide<9, 5>, <2, 2>; f32_mfma<1, 7, 9> x {fp32, G8}; f32_mfma_wide<3, 1..3> x {fp32, G8};
    # split<2, 1>, <7, 1>, <7, 1, 1>, <4, 0>; split_pw<7>
    assert seen == {"vit_attention_mfma": 4, "vit_attention_flash": 1, "vit_attention_flash_wide": 2, "vit_attention_f32_mfma": 6,
                    "vit_attention_f32_mfma_wide": 6, "vit_attention_split": 4, "vit_attention_split_pw": 1}, seen
