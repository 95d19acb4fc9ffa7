"""GPU: the beam form of the OPT decode-step attention (cap_op_opt_beam_decode_attention) alone.

Rows r = image * K + beam over caches [B * K][Lmax][T].  A row's history: the P prompt keys from the cache of row image * K (stored
once per image), key P + g from the cache of row anc[r][g], its own new key from the fused q|k|v row.  The kernel keeps the greedy
kernel's sums in the greedy kernel's order, so the tests are exact: the same history laid out contiguously per row and given to
cap_op_opt_decode_attention must produce the same bits.  The float64 bar is the one tests/test_attention_kernels_gpu.py derives
(8 x the error of the same formula in torch float32 against float64 on the same inputs; bf16: after the final rounding's half ulp);
run with -s for the maxima (appended to profiles/attention_kernels_gpu_tolerances.txt).

Shapes: T = H * hd with H = 2, hd 16 (the runtime-width form) and 80 (OPT-2.7b's, HD8 = 10), P = 9, Lmax = 80; generated positions
0 / 1 (nothing / one key read through the table), 3 / 5 (the P.V tail loop) and 60 (70 keys: the lanes' second trip over the keys and
the 16-key unrolled P.V loop)."""
import math

import pytest
import torch

from test_attention_kernels_gpu import BF16, DT_NAME, F32, SPLIT, _check, _in_t, _judge, _out_t, _p, _refused, _stream

pytestmark = pytest.mark.gpu

H, P, LMAX, SENTINEL = 2, 9, 80, 77.0
DTYPES = [F32, BF16, SPLIT]


@pytest.fixture(scope="module")
def lib():
    from embodied_captioning_amd import _native
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _native.load_library()


def _case(B, K, g, hd, dtype, seed, identity=False):
    """Host tensors of one call, in the kernel's input type: qkv [R, 3T], caches [R, LMAX, T] (sentinel wherever nothing is stored),
    anc int32 [R, LMAX - P], and the same histories contiguous per row (gk, gv) for the greedy kernel."""
    gen = torch.Generator().manual_seed(seed)
    it = _in_t(dtype)
    R, T, past = B * K, H * hd, P + g
    rn = lambda *s: (torch.randn(*s, generator=gen) * 1.5).to(it)      # noqa: E731
    qkv = rn(R, 3 * T)
    kc, vc = torch.full((R, LMAX, T), SENTINEL, dtype=it), torch.full((R, LMAX, T), SENTINEL, dtype=it)
    kc[::K, :P], vc[::K, :P] = rn(B, P, T), rn(B, P, T)                  # the prompt: the image's first row only
    kc[:, P:past], vc[:, P:past] = rn(R, g, T), rn(R, g, T)             # every row generated something at every position
    first = (torch.arange(R) // K * K)[:, None]
    if identity:
        anc = torch.arange(R)[:, None].expand(R, LMAX - P).contiguous()
    else:
        anc = first + torch.randint(0, K, (R, LMAX - P), generator=gen)
    src = torch.cat([first.expand(R, P), anc[:, :g]], 1)                # [R, past]: the row that holds key j of row r
    jj = torch.arange(past)[None, :]
    gk, gv = torch.full_like(kc, SENTINEL), torch.full_like(vc, SENTINEL)
    gk[:, :past], gv[:, :past] = kc[src, jj], vc[src, jj]
    return {"qkv": qkv, "kc": kc, "vc": vc, "anc": anc.to(torch.int32), "gk": gk, "gv": gv, "R": R, "T": T, "past": past, "K": K, "B": B}


def _out(R, T, dtype):
    return torch.full((R, T), float("nan"), dtype=_out_t(dtype), device="cuda")


def _run_beam(lib, dtype, c, anc="table"):
    qd, kd, vd, od = c["qkv"].cuda(), c["kc"].cuda(), c["vc"].cuda(), _out(c["R"], c["T"], dtype)
    ad = c["anc"].cuda() if anc == "table" else None
    _check(lib, lib.cap_op_opt_beam_decode_attention(dtype, _p(qd), _p(kd), _p(vd), _p(od), c["B"], c["K"], c["T"], H, LMAX, P, c["past"],
                                                     _p(ad), LMAX - P, _stream()))
    torch.cuda.synchronize()
    return od.cpu(), kd.cpu(), vd.cpu()


def _run_greedy(lib, dtype, c, k, v):
    qd, kd, vd, od = c["qkv"].cuda(), k.cuda(), v.cuda(), _out(c["R"], c["T"], dtype)
    _check(lib, lib.cap_op_opt_decode_attention(dtype, _p(qd), _p(kd), _p(vd), _p(od), c["R"], c["T"], H, LMAX, c["past"], _stream()))
    torch.cuda.synchronize()
    return od.cpu(), kd.cpu(), vd.cpu()


def _same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(a.view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32),
                                              b.view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32))


def _assert_only_the_new_slot_written(c, kd, vd):
    """Exactly slot `past` of each row's OWN cache holds the row's k / v; the prompt region and every other slot are as they were."""
    T, past = c["T"], c["past"]
    for name, got, before, col in (("k", kd, c["kc"], 1), ("v", vd, c["vc"], 2)):
        want = before.clone()
        want[:, past] = c["qkv"][:, col * T:(col + 1) * T]
        assert _same_bits(got, want), f"{name} cache: something other than slot `past` of the row's own cache changed"


@pytest.mark.parametrize("g", [0, 3, 60])
@pytest.mark.parametrize("hd", [16, 80])
@pytest.mark.parametrize("dtype", DTYPES)
def test_one_beam_with_identity_ancestry_is_the_greedy_kernel(lib, dtype, hd, g):
    c = _case(3, 1, g, hd, dtype, 100 * hd + g, identity=True)
    ob, kb, vb = _run_beam(lib, dtype, c)
    og, kg, vg = _run_greedy(lib, dtype, c, c["kc"], c["vc"])
    assert not torch.isnan(og.float()).any()
    assert _same_bits(ob, og) and _same_bits(kb, kg) and _same_bits(vb, vg)
    on, kn, vn = _run_beam(lib, dtype, c, anc=None)          # no table at one beam: every key the row's own
    assert _same_bits(on, og) and _same_bits(kn, kg) and _same_bits(vn, vg)


@pytest.mark.parametrize("g", [1, 5, 60])
@pytest.mark.parametrize("hd", [16, 80])
@pytest.mark.parametrize("dtype", DTYPES)
def test_random_ancestry_and_a_prompt_stored_once_per_image(lib, dtype, hd, g):
    B, K = 2, 3
    c = _case(B, K, g, hd, dtype, 7 + 100 * hd + g)
    ob, kb, vb = _run_beam(lib, dtype, c)
    _assert_only_the_new_slot_written(c, kb, vb)
    og, _, _ = _run_greedy(lib, dtype, c, c["gk"], c["gv"])  # the same histories, contiguous per row
    assert not torch.isnan(og.float()).any()
    assert _same_bits(ob, og)
    # float64: softmax(q k^T / sqrt(hd)) v over each row's history and its new key
    R, T, past = c["R"], c["T"], c["past"]
    heads = lambda x: x.float().view(R, -1, H, hd).permute(0, 2, 1, 3)          # noqa: E731  [R, L, T] -> [R, H, L, hd]
    knew, vnew = c["qkv"][:, None, T:2 * T], c["qkv"][:, None, 2 * T:]
    prob = {"q": heads(c["qkv"][:, None, :T]), "k": heads(torch.cat([c["gk"][:, :past], knew], 1)),
            "v": heads(torch.cat([c["gv"][:, :past], vnew], 1)), "mask": torch.ones(1, 1, 1, past + 1, dtype=torch.bool),
            "scale": 1.0 / math.sqrt(hd)}
    if dtype == SPLIT:
        from _util import g8_decode
        out = torch.from_numpy(g8_decode(ob.numpy()))
    else:
        out = ob.float()
    _judge(f"opt_beam_decode {DT_NAME[dtype]} hd {hd} B {B} K {K} generated {g}", "opt", (hd, past), "randn", dtype, out.view(R, 1, T), prob)


def test_refusals_by_name(lib):
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device="cuda")      # noqa: E731
    anc = z(6, 1100, dt=torch.int32)

    def call(T, Lmax, past, K=3, table=anc):
        qkv, kc, out = z(6, 3 * T), z(6 * Lmax * T), z(6, T)
        return lib.cap_op_opt_beam_decode_attention(F32, _p(qkv), _p(kc), _p(kc), _p(out), 2, K, T, H, Lmax, P, past, _p(table), 1100, _stream())

    _refused(lib, call(24, LMAX, 12), "T=24")                # head_dim 12
    _refused(lib, call(272, LMAX, 12), "T=272")              # head_dim 136
    _refused(lib, call(32, 1030, 1024), "past=1024")         # past + 1 > 1024
    _refused(lib, call(32, LMAX, 12, table=None), "ancestry")
    _refused(lib, call(32, LMAX, 12, K=9), "beams=9")
    _refused(lib, call(32, LMAX, P - 1), "prompt keys")
