"""GPU: the small-batch decode kernels (csrc/decode_small.hip) one launch at a time, through cap_op_small_gemm /
cap_op_small_cross, and the fused-producer form of the batch path's decode attention (cap_op_decode_attention_fused).

Every case makes two comparisons:
  (a) against a float64 reference built from the already-rounded operands, which rounds every intermediate (the LayerNorm row,
      the attention context, q through the attention's value type) to the type the kernel stores it in;
  (b) bit for bit against the batch-path chain on the same inputs - cap_op_reduce_layernorm, cap_op_gemm_partial (tile 6),
      cap_op_gemm, cap_op_decode_attention(_fused), cap_op_pack_kv16: decode_small.hip promises the same bits by construction.
Every output buffer starts as NaN and is larger than what the kernel owns: what it owns must be finite afterwards, the rest
still NaN (x_out rows from R on, out columns N..ldc, out_part slabs from S on, skipped rows, every cache position but the appended).

Tolerances of (a).
Operands straight from memory (PRO_GLOBAL): the bounds of test_split_gpu.py::test_decode_rows_kernel_split_k_slices_and_row_invariance,
2e-4 sqrt(K / 64) for bf16 against the product of the rounded operands, 1e-5 sqrt(max(K, 256) / 256) for the split mode against
the original fp32 operands.
Quantised intermediates: an fp32 value next to a rounding boundary may land on the neighbouring bf16 number, and that is not
derivable in advance; so the BATCH chain of (b) - code independent of the kernels under test, pinned by the HF goldens - was run
on every case of this file and its worst absolute error against the same float64 reference taken per dtype and kind.  The bound
is twice that maximum, rounded up to one significant digit (flips are rare and input dependent; the small path is allowed none
the batch path does not have, which (b) enforces exactly anyway).  Measured on the MI355X (docs/experiments.md has the same table):

    kind (prologue -> epilogue)        bf16: batch max  bound     split: batch max  bound
    ln_partial    LN -> slabs          6.619e-07        2e-6      7.665e-07         2e-6
    ln_act_t      LN -> GELU, operand  7.778e-03        2e-2      8.473e-07         2e-6
    ln_act_f32    LN -> act, fp32      2.363e-06        5e-6      2.762e-06         6e-6
    sa_partial    self-attn -> slabs   1.326e-04        3e-4      9.726e-07         2e-6
    cross         cross kernel         3.084e-02        7e-2      4.762e-06         1e-5

(bf16 slabs and fp32 outputs stay at fp32 rounding because the reference rounds the LayerNorm row exactly where the kernel does and no
value of these inputs sat on a bf16 boundary; an operand-type output adds its own rounding, the attention context and q theirs.)
The tests assert the constants (TOL); they print both chains' errors before asserting and never re-measure.
x_out is fp32 arithmetic on exact inputs: LayerNorm 3e-5 and the plain sum 1e-5, the bounds of test_kernels_gpu.py::test_reduce_layernorm.
The fused decode attention with an exactly known q: 1e-5 (fp32 / G8 context) and 2e-2 (bf16 context), the bounds of
test_kernels_gpu.py::test_decode_attention_with_ancestry_and_shared_kv.
Cache values, x_out against the batch kernels and every comparison (b): torch.equal.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from _util import G8_WSCALE, NAN, g8_decode, g8_encode, kv16_unpack
from _util import att_dtype as _att_dtype, check_rc as _check, cur_stream as _stream, finish32 as _finish32, nan_buf as _nan, nan_f32 as _nanf
from _util import operand_values as _val, ptr as _p, same_bits as _same_bits

pytestmark = pytest.mark.gpu

SPLIT = 2
TAG = {"bf16": 1, "f32s": SPLIT}
SLAB = {"bf16": 64, "f32s": 32}
DTYPES = ["bf16", "f32s"]
EPS = 1e-5
PRO_GLOBAL, PRO_LN, PRO_SA = 0, 1, 2
EPI_PARTIAL, EPI_ACT_T, EPI_ACT_F32 = 0, 1, 2
KV_F32, KV_BF16, KV_KV16 = 0, 1, 2

# twice the batch chain's worst error against float64, one significant digit, rounded up (module docstring)
TOL = {
    ("ln_partial", "bf16"): 2e-6, ("ln_partial", "f32s"): 2e-6,
    ("ln_act_t", "bf16"): 2e-2, ("ln_act_t", "f32s"): 2e-6,
    ("ln_act_f32", "bf16"): 5e-6, ("ln_act_f32", "f32s"): 6e-6,
    ("sa_partial", "bf16"): 3e-4, ("sa_partial", "f32s"): 2e-6,
    ("cross", "bf16"): 7e-2, ("cross", "f32s"): 1e-5,
}
TOL_X_LN, TOL_X_SUM = 3e-5, 1e-5
TOL_ATT = {"bf16": 2e-2, "f32s": 1e-5}


@pytest.fixture(scope="module")
def lib():
    from embodied_captioning_amd import _native
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _native.load_library()


def _report(kind, dt, batch_err, small_err):
    print(f"MEASURE {kind} {dt} batch {batch_err:.3e} small {small_err:.3e}")


# ---- operands --------------------------------------------------------------------------------------------------------
def _op(dt, x):
    """fp32 host tensor -> GEMM operand on the device (bf16, or the G8 container as float32 words)"""
    if dt == "bf16":
        return x.to(torch.bfloat16).cuda()
    return torch.from_numpy(g8_encode(x.contiguous().numpy())).cuda()


def _wop(lib, dt, W):
    if dt == "bf16":
        return W.to(torch.bfloat16).cuda()
    src, d = W.cuda(), torch.empty(W.shape, dtype=torch.float32, device="cuda")
    _check(lib, lib.cap_op_convert_weight(SPLIT, C.c_void_p(_p(src)), C.c_void_p(_p(d)), W.shape[0], W.shape[1], _stream()))
    torch.cuda.synchronize()
    return d


def _round_op(dt, x64):
    """what a store in the operand type keeps of a value"""
    if dt == "bf16":
        return x64.float().to(torch.bfloat16).double()
    return torch.from_numpy(g8_decode(g8_encode(x64.float().contiguous().numpy()))).double()


def _act64(x, act):
    if act == 1:
        return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))
    return x.clamp_min(0.0) if act == 2 else x


# ---- LayerNorm prologue ------------------------------------------------------------------------------------------------
class LnIn:
    """inputs of a SmallLN on the host and the device, its float64 results, the batch kernel's"""

    def __init__(self, g, S, R, D, bias=True, resid=True, x_is_sum=0, x_out=True):
        self.S, self.R, self.D, self.x_is_sum = S, R, D, x_is_sum
        self.part = torch.randn(S, R, D, generator=g)
        self.bias = torch.randn(D, generator=g) if bias else None
        self.resid = torch.randn(R, D, generator=g) * 2 if resid else None
        self.gamma, self.beta = torch.rand(D, generator=g) + 0.5, torch.randn(D, generator=g) * 0.5
        self.d = {k: (getattr(self, k).cuda() if getattr(self, k) is not None else None) for k in ("part", "bias", "resid", "gamma", "beta")}
        self.x_out = _nanf(R + 2, D) if x_out else None
        y = self.part.double().sum(0)
        if bias:
            y = y + self.bias.double()
        if resid:
            y = y + self.resid.double()
        self.y64 = y
        self.x64 = torch.nn.functional.layer_norm(y, (D,), self.gamma.double(), self.beta.double(), EPS)

    def rows(self, r0, r1):
        """the same inputs for rows r0..r1 alone"""
        o = object.__new__(LnIn)
        o.S, o.R, o.D, o.x_is_sum = self.S, r1 - r0, self.D, self.x_is_sum
        o.d = dict(self.d)
        o.d["part"] = self.d["part"][:, r0:r1].contiguous()
        o.d["resid"] = self.d["resid"][r0:r1].contiguous() if self.d["resid"] is not None else None
        o.x_out = _nanf(r1 - r0 + 2, self.D) if self.x_out is not None else None
        return o

    def fill(self, ln):
        ln.part, ln.S, ln.bias, ln.resid = _p(self.d["part"]), self.S, _p(self.d["bias"]), _p(self.d["resid"])
        ln.gamma, ln.beta, ln.eps, ln.x_out, ln.x_is_sum = _p(self.d["gamma"]), _p(self.d["beta"]), EPS, _p(self.x_out), self.x_is_sum

    def batch(self, lib, dt):
        """cap_op_reduce_layernorm on the same inputs -> (operand row, fp32 LayerNorm, fp32 sum)"""
        R, D = self.R, self.D
        xt, xf, y = _nan(dt, R, D), _nanf(R, D), _nanf(R, D)
        _check(lib, lib.cap_op_reduce_layernorm(TAG[dt], C.c_void_p(_p(self.d["part"])), self.S, C.c_void_p(_p(self.d["bias"])),
                                                C.c_void_p(_p(self.d["resid"])), C.c_void_p(_p(self.d["gamma"])), C.c_void_p(_p(self.d["beta"])),
                                                C.c_float(EPS), C.c_void_p(_p(xt)), C.c_void_p(_p(xf)), C.c_void_p(_p(y)), R, D, 1, _stream()))
        torch.cuda.synchronize()
        return xt, xf, y

    def check_x_out(self, batch_xf, batch_y, live=None):
        """x_out: the rows < R that were computed against float64 and the batch kernel's bits; skipped rows and rows from R on untouched"""
        if self.x_out is None:
            return
        R = self.R
        live = torch.ones(R, dtype=torch.bool) if live is None else live
        got, want, bat = self.x_out[:R].cpu(), (self.y64 if self.x_is_sum else self.x64), (batch_y if self.x_is_sum else batch_xf).cpu()
        assert torch.isfinite(got[live]).all() and torch.isnan(got[~live]).all() and torch.isnan(self.x_out[R:]).all()
        assert (got[live].double() - want[live]).abs().max().item() < (TOL_X_SUM if self.x_is_sum else TOL_X_LN)
        assert torch.equal(got[live], bat[live])


def _small_gemm(lib, dt, W, R, N, K, S, pro, epi, nchain, A=None, ln=None, sa=None, out_part=None, bias=None, act=0, out=None, ldc=0,
                tag=None):
    from embodied_captioning_amd._native import CapSmallGemm
    a = CapSmallGemm()
    a.W, a.A, a.R, a.N, a.K, a.S, a.pro, a.epi, a.nchain = _p(W), _p(A), R, N, K, S, pro, epi, nchain
    if ln is not None:
        ln.fill(a.ln)
    if sa is not None:
        sa(a.sa)
    a.out_part, a.bias, a.act, a.out, a.ldc = _p(out_part), _p(bias), act, _p(out), ldc
    rc = lib.cap_op_small_gemm(TAG[dt] if tag is None else tag, C.byref(a), _stream())
    torch.cuda.synchronize()
    return rc


def _batch_partial(lib, dt, A, W, R, N, K, S):
    part = _nanf(S, R, N)
    _check(lib, lib.cap_op_gemm_partial(TAG[dt], C.c_void_p(_p(A)), C.c_void_p(_p(W)), C.c_void_p(_p(part)), R, N, K, S, 6, _stream()))
    torch.cuda.synchronize()
    return part


def _slab_refs(A64, W64, S):
    Ks = A64.shape[1] // S
    return torch.stack([A64[:, z * Ks:(z + 1) * Ks] @ W64[:, z * Ks:(z + 1) * Ks].T for z in range(S)])


# ---- GEMM, operands from memory ------------------------------------------------------------------------------------------
GLOBAL_SLABS = [1, 3, 24, 25, 48, 49, 72, 73, 97]      # S = 1: waves without a slab; n = 6 | 7; 12 | 13; 18 | 19; 25 slabs on wave 0


def _global_case(lib, dt, R, N, K, S, seed):
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(R, K, generator=g)
    W = torch.randn(N, K, generator=g) / math.sqrt(K)
    Ad, Wd = _op(dt, A), _wop(lib, dt, W)
    if dt == "bf16":
        ref, tol = _slab_refs(Ad.cpu().double(), Wd.cpu().double(), S), 2e-4 * math.sqrt(K / 64)
    else:
        ref, tol = _slab_refs(A.double(), W.double(), S), 1e-5 * math.sqrt(max(K, 256) / 256)
    part = _nanf(S + 1, R, N)
    _check(lib, _small_gemm(lib, dt, Wd, R, N, K, S, PRO_GLOBAL, EPI_PARTIAL, 4, A=Ad, out_part=part))
    assert torch.isfinite(part[:S]).all() and torch.isnan(part[S:]).all()
    err = (part[:S].cpu().double() - ref).abs().max().item()
    print(f"global {dt} R={R} N={N} K={K} S={S}: err {err:.3e} (bound {tol:.3e})")
    assert err < tol
    assert (part[:S].cpu().double().sum(0) - ref.sum(0)).abs().max().item() < tol
    assert torch.equal(part[:S], _batch_partial(lib, dt, Ad, Wd, R, N, K, S))


@pytest.mark.parametrize("slabs", GLOBAL_SLABS)
@pytest.mark.parametrize("dt", DTYPES)
def test_gemm_global_slabs_per_chain_against_the_register_batches(lib, dt, slabs):
    """PRO_GLOBAL -> EPI_PARTIAL on 4 chains, one K slice: the two-deep register pipeline of NF = 6 slab batches at every count of
    slabs per chain where a batch boundary or a reload (b + 2, b + 3, the second trip round the pair loop) comes into play."""
    for N in (16, 48):
        for R in (1, 5, 16):
            _global_case(lib, dt, R, N, slabs * SLAB[dt], 1, 1000 * slabs + 10 * N + R)


@pytest.mark.parametrize("S", [2, 3, 4])
@pytest.mark.parametrize("dt", DTYPES)
def test_gemm_global_k_slices(lib, dt, S):
    for N, R in ((16, 5), (48, 16), (48, 1)):
        _global_case(lib, dt, R, N, 48 * SLAB[dt], S, 77 * S + N + R)


# ---- GEMM, LayerNorm prologue ----------------------------------------------------------------------------------------------
LN_K = {"bf16": [128, 768, 832, 1024], "f32s": [384, 416, 768, 800, 1024]}
LN_R = [1, 4, 5, 8, 9, 16]
FORMS = [("ln_partial", EPI_PARTIAL, 4, 0), ("ln_act_t", EPI_ACT_T, 4, 1), ("ln_act_f32", EPI_ACT_F32, 1, 0), ("ln_act_f32", EPI_ACT_F32, 1, 2),
         ("ln_act_f32", EPI_ACT_F32, 1, 1)]


def _ln_cases():
    """A fixed list: every K of the dtype under every form; S in {1, 2, 4} wherever K divides, on EPI_PARTIAL (with more than one
    slice an activation epilogue has two workgroups storing one element: the engine never asks, there is no result to check);
    R, N, ln.S, bias / resid, x_is_sum, x_out cycle with periods that do not share a factor with each other's."""
    cases, i = [], 0
    for dt in DTYPES:
        for kind, epi, nchain, act in FORMS:
            for K in LN_K[dt]:
                for S in ((1, 2, 4) if epi == EPI_PARTIAL else (1,)):
                    if K % (SLAB[dt] * S):
                        continue
                    R = LN_R[i % 6]
                    N = (4, 60, 68, 1020)[i % 4] if nchain == 1 else (48, 16, 64)[i % 3]
                    cases.append(dict(dt=dt, kind=kind, epi=epi, nchain=nchain, act=act, K=K, S=S, R=R, N=N, lnS=(1, 2, 4)[(i // 2) % 3],
                                      bias=i % 5 != 2, resid=i % 7 != 3, x_is_sum=(i // 3) % 2, x_out=i % 4 != 1, seed=i))
                    i += 1
    return cases


LN_CASES = _ln_cases()


def _ln_id(c):
    return f"{c['dt']}-{c['kind']}{c['act']}-K{c['K']}-S{c['S']}-R{c['R']}-N{c['N']}-ln{c['lnS']}{'b' if c['bias'] else ''}{'r' if c['resid'] else ''}" \
           f"{'y' if c['x_is_sum'] else ''}{'x' if c['x_out'] else ''}"


def test_ln_case_list_covers_every_listed_value():
    for dt in DTYPES:
        cs = [c for c in LN_CASES if c["dt"] == dt]
        assert {c["K"] for c in cs} == set(LN_K[dt]) and {c["R"] for c in cs} == set(LN_R)
        assert {c["S"] for c in cs if c["nchain"] == 4} == {1, 2, 4}
        assert {c["N"] for c in cs if c["nchain"] == 1} == {4, 60, 68, 1020}
        assert {c["lnS"] for c in cs} == {1, 2, 4} and {c["act"] for c in cs if c["nchain"] == 1} == {0, 1, 2}
        for key in ("bias", "resid", "x_is_sum", "x_out"):
            assert {bool(c[key]) for c in cs} == {False, True}
        # the one-chain kernel's 12 | 13 and 24 | 25 slabs against both of its batch sizes (NF = 12 up to 8 rows, 6 beyond)
        one = [c for c in cs if c["nchain"] == 1]
        assert {c["R"] <= 8 for c in one} == {False, True}
        # every RPW (rows per wave of the prologue: 1, 2, 4) on both kernels
        for nchain in (1, 4):
            assert {min((c["R"] + 3) // 4, 3) for c in cs if c["nchain"] == nchain} == {1, 2, 3}


def _ln_gemm(lib, c, ln, Wd, bd, R):
    """one launch of the case on `ln` (R rows) -> (out_part or None, out or None)"""
    dt, N, K, S, ldc = c["dt"], c["N"], c["K"], c["S"], c["N"] + (12 if c["epi"] == EPI_ACT_F32 else 16)
    part = out = None
    if c["epi"] == EPI_PARTIAL:
        part = _nanf(S + 1, R, N)
    elif c["epi"] == EPI_ACT_T:
        out = _nan(dt, R + 1, ldc)
    else:
        out = _nanf(R + 1, ldc)
    _check(lib, _small_gemm(lib, dt, Wd, R, N, K, S, PRO_LN, c["epi"], c["nchain"], ln=ln, out_part=part, bias=bd, act=c["act"], out=out, ldc=ldc))
    return part, out


def _ln_batch(lib, c, xt, Wd, bd, R):
    dt, N, K = c["dt"], c["N"], c["K"]
    if c["epi"] == EPI_PARTIAL:
        return _batch_partial(lib, dt, xt, Wd, R, N, K, c["S"])
    f32 = c["epi"] == EPI_ACT_F32
    o = _nanf(R, N) if f32 else _nan(dt, R, N)
    # fc1 runs on the rows kernel (tile 6), the transform / vocabulary GEMMs on the register-staged tile the launcher picks (tile 0);
    # cap_op_gemm has GELU only: ReLU is taken of the plain output, bit for bit what fmaxf(v, 0) gives
    _check(lib, lib.cap_op_gemm(TAG[dt], C.c_void_p(_p(xt)), C.c_void_p(_p(Wd)), C.c_void_p(_p(bd)), None, C.c_void_p(_p(o)), R, N, K,
                                1 if c["act"] == 1 else 0, 1 if f32 else 0, 0 if f32 else 6, _stream()))
    torch.cuda.synchronize()
    return o.clamp_min(0.0) if c["act"] == 2 else o


@pytest.mark.parametrize("c", LN_CASES, ids=_ln_id)
def test_gemm_layernorm_prologue(lib, c):
    dt, R, N, K, S = c["dt"], c["R"], c["N"], c["K"], c["S"]
    g = torch.Generator().manual_seed(4000 + c["seed"])
    ln = LnIn(g, c["lnS"], R, K, c["bias"], c["resid"], c["x_is_sum"], c["x_out"])
    W = torch.randn(N, K, generator=g) / math.sqrt(K)
    b = torch.randn(N, generator=g) if c["epi"] != EPI_PARTIAL else None
    Wd, bd = _wop(lib, dt, W), (b.cuda() if b is not None else None)
    W64 = _val(dt, Wd, G8_WSCALE if dt == "f32s" else 1.0)
    part, out = _ln_gemm(lib, c, ln, Wd, bd, R)
    xt, xf, y = ln.batch(lib, dt)
    bat = _ln_batch(lib, c, xt, Wd, bd, R)
    A64 = _round_op(dt, ln.x64)
    if c["epi"] == EPI_PARTIAL:
        ref = _slab_refs(A64, W64, S)
        assert torch.isfinite(part[:S]).all() and torch.isnan(part[S:]).all()
        got, got_b, bits, bits_b = part[:S].cpu().double(), bat.cpu().double(), part[:S], bat
    else:
        ref = _act64(A64 @ W64.T + b.double(), c["act"])
        vdt = dt if c["epi"] == EPI_ACT_T else "bf16"          # (a float32 tensor decodes as itself through the bf16 branch)
        assert torch.isnan(out[R:]).all() and torch.isnan(out[:, N:]).all()
        bits, bits_b = out[:R, :N], bat
        got, got_b = _val(vdt, bits.contiguous()), _val(vdt, bat)
        assert torch.isfinite(got).all()
    eb, es = (got_b - ref).abs().max().item(), (got - ref).abs().max().item()
    _report(c["kind"], dt, eb, es)
    ln.check_x_out(xf, y)
    assert _same_bits(bits, bits_b) if c["epi"] == EPI_ACT_T else torch.equal(bits, bits_b)
    assert es < TOL[(c["kind"], dt)]


# ---- GEMM, self-attention prologue -------------------------------------------------------------------------------------
SA_KEYS = [1, 8, 9, 16, 17, 32]
SA_HS = [(2, 1), (2, 2), (4, 2), (4, 1)]                  # (H, S): all heads in one slice; one head per slice; two; all


def _sa_cases():
    cases, i = [], 0
    for dt in DTYPES:
        for nk in SA_KEYS:
            for H, S in SA_HS:
                R = (1, 6, 16)[i % 3]
                cases.append(dict(dt=dt, n_keys=nk, H=H, S=S, R=R, anc=R == 6 and (i // 3) % 2 == 0, qkv_S=(1, 2, 4)[(i // 2) % 3], seed=i))
                i += 1
    return cases


SA_CASES = _sa_cases()


def test_sa_case_list_covers_every_listed_value():
    for dt in DTYPES:
        cs = [c for c in SA_CASES if c["dt"] == dt]
        assert {c["R"] for c in cs} == {1, 6, 16} and {c["qkv_S"] for c in cs} == {1, 2, 4}
        assert {c["anc"] for c in cs if c["R"] == 6} == {False, True}
        assert {(c["n_keys"], c["H"], c["S"]) for c in cs} == {(k, h, s) for k in SA_KEYS for h, s in SA_HS}


class SaIn:
    KV_LD, N = 40, 48

    def __init__(self, dt, c):
        g = torch.Generator().manual_seed(9000 + c["seed"])
        self.dt, self.c = dt, c
        R, H, nk = c["R"], c["H"], c["n_keys"]
        self.R, self.H, self.K = R, H, 64 * H
        ta = _att_dtype(dt)
        self.part = torch.randn(c["qkv_S"], R, 3 * H * 64, generator=g)
        self.bias = torch.randn(3 * H * 64, generator=g) * 0.5
        self.kc = torch.randn(R, H, self.KV_LD, 64, generator=g).to(ta)
        self.vc = torch.randn(R, H, self.KV_LD, 64, generator=g).to(ta)
        self.anc = None
        if c["anc"]:      # 2 images x 3 beams: position j of row r was written by a beam of r's image
            self.anc = ((torch.arange(R) // 3 * 3)[:, None] + torch.randint(0, 3, (R, self.KV_LD), generator=g)).to(torch.int32)
        self.W = torch.randn(self.N, self.K, generator=g) / math.sqrt(self.K)
        self.part_d, self.bias_d = self.part.cuda(), self.bias.cuda()
        self.anc_d = self.anc.cuda() if self.anc is not None else None
        # float64 reference: the newest position's q | k | v are the fp32 sums through the attention's value type, exactly
        fin = _finish32(self.part, self.bias).to(ta)
        self.q, self.kn, self.vn = (fin[:, i * self.K:(i + 1) * self.K].reshape(R, H, 64) for i in range(3))
        src = self.anc[:, :nk].long() if self.anc is not None else torch.arange(R)[:, None].expand(R, nk)
        hh, jj = torch.arange(H)[None, :, None], torch.arange(nk)[None, None, :]
        Kg, Vg = self.kc[src[:, None, :], hh, jj].double(), self.vc[src[:, None, :], hh, jj].double()
        Kg[:, :, nk - 1], Vg[:, :, nk - 1] = self.kn.double(), self.vn.double()
        p = torch.softmax(torch.einsum("rhd,rhjd->rhj", self.q.double(), Kg) * 0.125, -1)
        self.ctx64 = torch.einsum("rhj,rhjd->rhd", p, Vg).reshape(R, self.K)

    def rows(self, r0, r1):
        """the device inputs of rows r0..r1 alone (no ancestry)"""
        return self.part_d[:, r0:r1].contiguous(), self.kc[r0:r1].cuda(), self.vc[r0:r1].cuda()

    def check_caches(self, kd, vd, r0=0):
        nk, R = self.c["n_keys"], kd.shape[0]
        want_k, want_v = self.kc[r0:r0 + R].clone(), self.vc[r0:r0 + R].clone()
        want_k[:, :, nk - 1], want_v[:, :, nk - 1] = self.kn[r0:r0 + R], self.vn[r0:r0 + R]
        assert torch.equal(kd.cpu(), want_k) and torch.equal(vd.cpu(), want_v)


def _sa_launch(lib, s, Wd, part_d, kd, vd, R, anc_d=None):
    c = s.c
    out = _nanf(c["S"] + 1, R, s.N)

    def fill(sa):
        sa.qkv_part, sa.qkv_bias, sa.qkv_S, sa.kc, sa.vc = _p(part_d), _p(s.bias_d), c["qkv_S"], _p(kd), _p(vd)
        sa.anc, sa.anc_ld, sa.kv_ld, sa.n_keys, sa.H, sa.skip = _p(anc_d), s.KV_LD, s.KV_LD, c["n_keys"], s.H, None
    _check(lib, _small_gemm(lib, s.dt, Wd, R, s.N, s.K, c["S"], PRO_SA, EPI_PARTIAL, 4, sa=fill, out_part=out))
    assert torch.isfinite(out[:c["S"]]).all() and torch.isnan(out[c["S"]:]).all()
    return out[:c["S"]]


def _fused_attention(lib, dt, part, S, bias, q_ld, col0, append, k, v, anc, anc_ld, rpk, kv_ld, n_keys, out, R, H, impl=0):
    rc = lib.cap_op_decode_attention_fused(TAG[dt], C.c_void_p(_p(part)), S, C.c_void_p(_p(bias)), q_ld, col0, append, C.c_void_p(k),
                                           C.c_void_p(v), C.c_void_p(_p(anc)), anc_ld, rpk, kv_ld, n_keys, C.c_void_p(_p(out)), R, H, impl,
                                           _stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("c", SA_CASES, ids=lambda c: f"{c['dt']}-keys{c['n_keys']}-H{c['H']}-S{c['S']}-R{c['R']}-qkv{c['qkv_S']}{'-anc' if c['anc'] else ''}")
def test_gemm_self_attention_prologue(lib, c):
    dt, R, S = c["dt"], c["R"], c["S"]
    s = SaIn(dt, c)
    Wd = _wop(lib, dt, s.W)
    W64 = _val(dt, Wd, G8_WSCALE if dt == "f32s" else 1.0)
    kd, vd = s.kc.cuda(), s.vc.cuda()
    part = _sa_launch(lib, s, Wd, s.part_d, kd, vd, R, s.anc_d)
    s.check_caches(kd, vd)                      # position n_keys - 1 exactly the rounded sums, everything else unchanged
    # the batch chain: the attention kernel with the fused producer, then the rows GEMM
    kb, vb, ctx = s.kc.cuda(), s.vc.cuda(), _nan(dt, R, s.K)
    _check(lib, _fused_attention(lib, dt, s.part_d, c["qkv_S"], s.bias_d, 3 * s.K, 0, 1, _p(kb), _p(vb), s.anc_d, s.KV_LD, 1, s.KV_LD, c["n_keys"],
                                 ctx, R, s.H))
    bat = _batch_partial(lib, dt, ctx, Wd, R, s.N, s.K, S)
    ref = _slab_refs(_round_op(dt, s.ctx64), W64, S)
    eb, es = (bat.cpu().double() - ref).abs().max().item(), (part.cpu().double() - ref).abs().max().item()
    _report("sa_partial", dt, eb, es)
    assert torch.equal(kb, kd) and torch.equal(vb, vd)
    assert torch.equal(part, bat)
    assert es < TOL[("sa_partial", dt)]


# ---- the cross kernel ------------------------------------------------------------------------------------------------------
CROSS_GEOM = [(128, 2), (768, 12), (1024, 16)]
CROSS_KINDS = [("bf16", KV_BF16), ("f32s", KV_F32), ("f32s", KV_KV16)]
# 1, 20, 32: the wave-unit branch and its last key (KV16: read from global memory); 33: the first LDS copy; 50; 197: the production
# block; 577: over the `fits` threshold for fp32 rows and KV16, and for bf16 rows the largest block that still fits (at D = 1024
# exactly the 150 KiB limit); 600: over it for bf16
CROSS_KEYS = {KV_BF16: [1, 20, 32, 33, 50, 197, 577, 600], KV_F32: [1, 20, 32, 33, 50, 197, 577], KV_KV16: [1, 20, 32, 33, 50, 197, 577]}


def _cross_cases():
    cases = []
    for dt, kind in CROSS_KINDS:
        geoms = [(D, H, S) for D, H in CROSS_GEOM for S in (1, 2, 3, 4) if D % (SLAB[dt] * S) == 0]
        keys = CROSS_KEYS[kind]
        for i in range(2 * len(keys)):       # every key count twice (the second time with the other kv_row0), the geometries in turn
            D, H, S = geoms[i % len(geoms)]
            nk = keys[i % len(keys)]
            R, rpk = ((1, 1), (16, 1), (6, 3))[i % 3]
            cases.append(dict(dt=dt, kind=kind, D=D, H=H, S=S, n_keys=nk, row0=(0, 37)[(i // len(keys) + i) % 2], pad=(0, 3)[(i // 2) % 2], R=R, rpk=rpk,
                              skip=R > 1 and i % 2 == 1, lnS=(1, 4)[(i // 3) % 2], x_is_sum=(i // 2) % 2, x_out=i % 5 != 4, seed=i))
        for j, (D, H, S) in enumerate(geoms):      # and every geometry at the production block
            i = 100 + j
            R, rpk = ((16, 1), (6, 3), (1, 1))[j % 3]
            cases.append(dict(dt=dt, kind=kind, D=D, H=H, S=S, n_keys=(197, 50)[j % 2], row0=(37, 0)[(j // 2) % 2], pad=(3, 0)[j % 2], R=R, rpk=rpk,
                              skip=R > 1 and j % 3 == 0, lnS=(4, 1)[j % 2], x_is_sum=j % 2, x_out=True, seed=i))
    return cases


CROSS_CASES = _cross_cases()


def _cross_id(c):
    return f"{c['dt']}-kv{c['kind']}-D{c['D']}-S{c['S']}-keys{c['n_keys']}-row{c['row0']}-pad{c['pad']}-R{c['R']}x{c['rpk']}" \
           f"{'-skip' if c['skip'] else ''}-ln{c['lnS']}{'y' if c['x_is_sum'] else ''}{'x' if c['x_out'] else ''}"


def test_cross_case_list_covers_every_listed_value():
    for dt, kind in CROSS_KINDS:
        cs = [c for c in CROSS_CASES if c["kind"] == kind]
        assert {(c["D"], c["H"], c["S"]) for c in cs} == {(D, H, S) for D, H in CROSS_GEOM for S in (1, 2, 3, 4) if D % (SLAB[dt] * S) == 0}
        assert {c["n_keys"] for c in cs} == set(CROSS_KEYS[kind])
        assert {c["row0"] for c in cs} == {0, 37} and {c["pad"] for c in cs} == {0, 3}
        assert {(c["R"], c["rpk"]) for c in cs} == {(1, 1), (16, 1), (6, 3)}
        assert {c["skip"] for c in cs} == {False, True} and {c["lnS"] for c in cs} == {1, 4}
        assert {c["x_is_sum"] for c in cs} == {0, 1} and any(c["x_out"] for c in cs)
        slabs = {c["D"] // SLAB[dt] // c["S"] for c in cs}         # per slice: one, exactly the register batch, the tail loop, a long tail
        assert {1, 6, 8, 16}.issubset(slabs) and (dt == "bf16" or 32 in slabs)
    # KV16 blocks copied to LDS (33..197 keys) that start on a 32-row group and inside one
    starts = {(c["row0"] + (c["n_keys"] + c["pad"]) * h) % 32 != 0 for c in CROSS_CASES if c["kind"] == KV_KV16 and 32 < c["n_keys"] <= 197
              for h in range(c["H"])}
    assert starts == {False, True}


class CrossIn:
    def __init__(self, lib, c):
        g = torch.Generator().manual_seed(20000 + 1000 * c["kind"] + c["seed"])
        self.c, dt = c, c["dt"]
        R, D, H, nk, rpk = c["R"], c["D"], c["H"], c["n_keys"], c["rpk"]
        self.kv_ld = nk + c["pad"]
        self.n_img = (R + rpk - 1) // rpk
        self.rows = c["row0"] + self.n_img * H * self.kv_ld
        self.ln = LnIn(g, c["lnS"], R, D, True, True, c["x_is_sum"], c["x_out"])
        self.W = torch.randn(D, D, generator=g) / math.sqrt(D)
        self.bias = torch.randn(D, generator=g) * 0.5
        Kf = torch.randn(self.rows, 64, generator=g)
        Vf = torch.randn(self.rows, 64, generator=g) * torch.logspace(-1, 1, 64)
        self.Wd, self.bias_d = _wop(lib, dt, self.W), self.bias.cuda()
        self.W64 = _val(dt, self.Wd, G8_WSCALE if dt == "f32s" else 1.0)
        self.skip = None
        if c["skip"]:
            self.skip = torch.zeros(R, dtype=torch.int32)
            self.skip[1::3] = 1
        self.skip_d = self.skip.cuda() if self.skip is not None else None
        self.live = torch.ones(R, dtype=torch.bool) if self.skip is None else self.skip == 0
        # the block as the kernel addresses it (by row index from its base) and as the batch kernels do (from the launch's first row)
        r0 = c["row0"]
        if c["kind"] == KV_KV16:
            self.kd, self.vd = self._pack(lib, Kf, self.rows), self._pack(lib, Vf, self.rows)
            self.kb, self.vb = self._pack(lib, Kf[r0:], self.rows - r0), self._pack(lib, Vf[r0:], self.rows - r0)
            self.kb_p, self.vb_p = _p(self.kb), _p(self.vb)
            K64, V64 = self._unpack(self.kd, self.rows), self._unpack(self.vd, self.rows)
            assert torch.equal(K64[r0:], self._unpack(self.kb, self.rows - r0))      # per-row quantisation: the same values either way
        else:
            tk = torch.bfloat16 if c["kind"] == KV_BF16 else torch.float32
            self.kd, self.vd = Kf.to(tk).cuda(), Vf.to(tk).cuda()
            esz = 2 if c["kind"] == KV_BF16 else 4
            self.kb_p, self.vb_p = _p(self.kd) + r0 * 64 * esz, _p(self.vd) + r0 * 64 * esz
            K64, V64 = self.kd.cpu().double(), self.vd.cpu().double()
        # float64 reference
        img = torch.arange(R) // rpk
        Kr = K64[r0:].view(self.n_img, H, self.kv_ld, 64)[img][:, :, :nk]
        Vr = V64[r0:].view(self.n_img, H, self.kv_ld, 64)[img][:, :, :nk]
        q = (_round_op(dt, self.ln.x64) @ self.W64.T + self.bias.double()).float().to(_att_dtype(dt)).double().view(R, H, 64)
        p = torch.softmax(torch.einsum("rhd,rhjd->rhj", q, Kr) * 0.125, -1)
        self.ctx64 = torch.einsum("rhj,rhjd->rhd", p, Vr).reshape(R, D)

    @staticmethod
    def _pack(lib, x, rows):
        src, d = x.contiguous().cuda(), torch.zeros((rows + 31) // 32 * 4224, dtype=torch.uint8, device="cuda")
        _check(lib, lib.cap_op_pack_kv16(C.c_void_p(_p(src)), C.c_void_p(_p(d)), rows, _stream()))
        torch.cuda.synchronize()
        return d

    @staticmethod
    def _unpack(d, rows):
        q, sc = kv16_unpack(d.cpu().numpy().tobytes(), rows)
        return torch.from_numpy(q.astype(np.float64) * sc.astype(np.float64)[:, None])

    def launch(self, lib, ln=None, R=None, row0=None, skip=True, tag=None, **over):
        """cap_op_small_cross -> (rc, out [R + 1, D])"""
        from embodied_captioning_amd._native import CapSmallCross
        c = self.c
        R = c["R"] if R is None else R
        out = _nan(c["dt"], R + 1, c["D"])
        a = CapSmallCross()
        a.W, a.bias, a.R, a.D, a.H, a.S = _p(self.Wd), _p(self.bias_d), R, c["D"], c["H"], c["S"]
        (self.ln if ln is None else ln).fill(a.ln)
        a.kbase, a.vbase, a.kv_row0 = _p(self.kd), _p(self.vd), c["row0"] if row0 is None else row0
        a.rows_per_kv, a.kv_ld, a.n_keys, a.kv_kind = c["rpk"], self.kv_ld, c["n_keys"], c["kind"]
        a.skip, a.out = (_p(self.skip_d) if skip else None), _p(out)
        for k, v in over.items():
            setattr(a, k, v)
        rc = lib.cap_op_small_cross(TAG[c["dt"]] if tag is None else tag, C.byref(a), _stream())
        torch.cuda.synchronize()
        return rc, out

    def batch(self, lib):
        """reduce + LayerNorm -> rows GEMM in S slices -> decode attention with the fused producer; None where the batch launcher
        refuses the shape by design (a KV16 cache with 32 keys or fewer)"""
        c, dt = self.c, self.c["dt"]
        R, D = c["R"], c["D"]
        xt, xf, y = self.ln.batch(lib, dt)
        qp = _batch_partial(lib, dt, xt, self.Wd, R, D, D, c["S"])
        out = _nan(dt, R, D)
        rc = _fused_attention(lib, dt, qp, c["S"], self.bias_d, D, 0, 0, self.kb_p, self.vb_p, None, 0, c["rpk"], self.kv_ld, c["n_keys"], out, R,
                              c["H"], 16 if c["kind"] == KV_KV16 else 0)
        if c["kind"] == KV_KV16 and c["n_keys"] <= 32:
            assert rc != 0 and b"KV16" in lib.cap_last_error()
            return xf, y, None
        _check(lib, rc)
        return xf, y, out


@pytest.mark.parametrize("c", CROSS_CASES, ids=_cross_id)
def test_cross_kernel(lib, c):
    dt, R = c["dt"], c["R"]
    x = CrossIn(lib, c)
    rc, out = x.launch(lib)
    _check(lib, rc)
    live = x.live
    assert torch.isnan(out[R:]).all() and torch.isnan(out[:R][~live]).all()          # skipped rows keep the sentinel
    got = _val(dt, out[:R].contiguous())
    assert torch.isfinite(got[live]).all()
    es = (got[live] - x.ctx64[live]).abs().max().item()
    xf, y, bat = x.batch(lib)
    x.ln.check_x_out(xf, y, live)    # (the head-0 workgroup of a skipped row returns before its LayerNorm)
    if bat is not None:
        eb = (_val(dt, bat)[live] - x.ctx64[live]).abs().max().item()
        _report("cross", dt, eb, es)
        assert _same_bits(out[:R][live.cuda()], bat[live.cuda()])
    else:
        print(f"MEASURE-small-only cross {dt} small {es:.3e}")
    assert es < TOL[("cross", dt)]


# ---- row invariance ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_row_alone_has_the_bits_it_has_among_sixteen(lib, dt):
    """One LayerNorm-prologue GEMM, one self-attention GEMM and one cross launch per cache kind: row r alone (R = 1) against row r of 16."""
    K = 768
    c = dict(dt=dt, kind="ln_partial", epi=EPI_PARTIAL, nchain=4, act=0, K=K, S=2, R=16, N=48)
    g = torch.Generator().manual_seed(31)
    ln = LnIn(g, 2, 16, K)
    Wd = _wop(lib, dt, torch.randn(48, K, generator=g) / math.sqrt(K))
    full, _ = _ln_gemm(lib, c, ln, Wd, None, 16)
    for r in (0, 7, 15):
        one = ln.rows(r, r + 1)
        alone, _ = _ln_gemm(lib, c, one, Wd, None, 1)
        assert torch.equal(alone[:2, 0], full[:2, r]) and torch.equal(one.x_out[0], ln.x_out[r])

    sc = dict(dt=dt, n_keys=17, H=4, S=2, R=16, anc=False, qkv_S=2, seed=77)
    s = SaIn(dt, sc)
    Wd = _wop(lib, dt, s.W)
    kd, vd = s.kc.cuda(), s.vc.cuda()
    full = _sa_launch(lib, s, Wd, s.part_d, kd, vd, 16)
    for r in (0, 7, 15):
        p1, k1, v1 = s.rows(r, r + 1)
        alone = _sa_launch(lib, s, Wd, p1, k1, v1, 1)
        assert torch.equal(alone[:, 0], full[:, r]) and torch.equal(k1[0], kd[r]) and torch.equal(v1[0], vd[r])

    for kdt, kind in CROSS_KINDS:
        if kdt != dt:
            continue
        cc = dict(dt=dt, kind=kind, D=768, H=12, S=4, n_keys=197, row0=0, pad=3, R=16, rpk=1, skip=False, lnS=4, x_is_sum=0, x_out=True, seed=5)
        x = CrossIn(lib, cc)
        rc, full = x.launch(lib)
        _check(lib, rc)
        for r in (0, 7, 15):      # row r's K/V block: the same cache, addressed from the row's first head row
            one = x.ln.rows(r, r + 1)
            rc, alone = x.launch(lib, ln=one, R=1, row0=r * 12 * x.kv_ld)
            _check(lib, rc)
            assert _same_bits(alone[0], full[r]) and torch.equal(one.x_out[0], x.ln.x_out[r])


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_small_gemm_refusals_name_the_launcher_and_write_nothing(lib):
    from embodied_captioning_amd._native import CapSmallGemm
    R, N, K, H = 4, 32, 128, 2
    Wd = torch.zeros(64, 2048, dtype=torch.float32, device="cuda")          # large enough for every shape tried, either type
    Ad = torch.zeros(16, 2048, dtype=torch.float32, device="cuda")
    f = torch.zeros(4 * 16 * 2048, dtype=torch.float32, device="cuda")     # slabs / q|k|v partial sums / bias / gamma / beta
    cache = torch.zeros(16 * H * 40 * 64, dtype=torch.float32, device="cuda")

    def attempt(dt, why, **kw):
        a = CapSmallGemm()
        a.W, a.A, a.R, a.N, a.K, a.S, a.pro, a.epi, a.nchain = _p(Wd), _p(Ad), R, N, K, 1, PRO_GLOBAL, EPI_PARTIAL, 4
        a.ln.part, a.ln.S, a.ln.gamma, a.ln.beta, a.ln.eps = _p(f), 1, _p(f), _p(f), EPS
        a.sa.qkv_part, a.sa.qkv_bias, a.sa.qkv_S, a.sa.kc, a.sa.vc = _p(f), _p(f), 1, _p(cache), _p(cache)
        a.sa.kv_ld, a.sa.n_keys, a.sa.H = 40, 5, H
        part, out, xo = _nanf(4, 16, 64), _nanf(17, 80), _nanf(18, 2048)
        a.out_part, a.bias, a.act, a.out, a.ldc, a.ln.x_out = _p(part), _p(f), 0, _p(out), 80, _p(xo)
        tag = TAG[dt] if isinstance(dt, str) else dt
        for k, v in kw.items():
            o, _, name = k.rpartition("__")
            setattr(getattr(a, o) if o else a, name, v)
        before = cache.clone()
        rc = lib.cap_op_small_gemm(tag, C.byref(a), _stream())
        torch.cuda.synchronize()
        err = lib.cap_last_error()
        assert rc != 0, why
        assert b"launch_small_gemm" in err, (why, err)
        assert torch.isnan(part).all() and torch.isnan(out).all() and torch.isnan(xo).all() and torch.equal(cache, before), why

    # the base shape is taken (so each refusal below is down to the one field it changes)
    for dt in DTYPES:
        a_part = _nanf(1, R, N)
        _check(lib, _small_gemm(lib, dt, Wd, R, N, K, 1, PRO_GLOBAL, EPI_PARTIAL, 4, A=Ad, out_part=a_part))
        assert (a_part == 0).all()
    attempt(0, "operand type CAP_F32")
    for dt in DTYPES:
        attempt(dt, "R = 0", R=0)
        attempt(dt, "R = 17", R=17)
        attempt(dt, "N % 4", N=18)
        attempt(dt, "N % 16 on 4 chains", N=20)
        attempt(dt, "K not whole slabs", K=K + 16)
        attempt(dt, "K not whole slabs per slice", K=3 * SLAB[dt], S=2)
        attempt(dt, "S = 0", S=0)
        attempt(dt, "LN prologue K = 1088", pro=PRO_LN, K=1088)
        attempt(dt, "LN prologue ln.S = 0", pro=PRO_LN, ln__S=0)
        attempt(dt, "self-attention n_keys = 0", pro=PRO_SA, sa__n_keys=0)
        attempt(dt, "self-attention n_keys = 33", pro=PRO_SA, sa__n_keys=33)
        attempt(dt, "self-attention qkv_S = 5", pro=PRO_SA, sa__qkv_S=5)
        attempt(dt, "self-attention qkv_S = 0", pro=PRO_SA, sa__qkv_S=0)
        attempt(dt, "global prologue with an activation epilogue", epi=EPI_ACT_T)
        attempt(dt, "fp32 epilogue on 4 chains", pro=PRO_LN, epi=EPI_ACT_F32)
        attempt(dt, "slabs on 1 chain", pro=PRO_LN, nchain=1)
        attempt(dt, "2 chains", nchain=2)
        attempt(dt, "self-attention prologue with an activation epilogue", pro=PRO_SA, epi=EPI_ACT_T)
    attempt("f32s", "a K slice of half a head", pro=PRO_SA, S=4)          # (a bf16 slab is a whole head already)


def test_small_cross_refusals_name_the_launcher_and_write_nothing(lib):
    for dt, kind in CROSS_KINDS:
        c = dict(dt=dt, kind=kind, D=128, H=2, S=1, n_keys=33, row0=0, pad=0, R=2, rpk=1, skip=False, lnS=1, x_is_sum=0, x_out=True, seed=1)
        x = CrossIn(lib, c)
        big = LnIn(torch.Generator().manual_seed(3), 1, 17, 1088)          # rows for the shapes beyond the base

        def attempt(why, **kw):
            rc, out = x.launch(lib, **kw)
            err = lib.cap_last_error()
            assert rc != 0, why
            assert b"launch_small_cross" in err, (why, err)
            ln = kw.get("ln", x.ln)
            assert torch.isnan(out).all() and torch.isnan(ln.x_out).all(), why

        attempt("operand type CAP_F32", tag=0)
        attempt("R = 0", R=0)
        attempt("R = 17", R=17, ln=big)
        attempt("D != 64 H", H=3)
        attempt("D = 1088", D=1088, H=17, ln=big)
        attempt("S = 5", S=5)
        attempt("S = 0", S=0)
        attempt("D not whole slabs per slice", S=3)
        attempt("n_keys = 0", n_keys=0)
        no_slabs = x.ln.rows(0, 2)
        no_slabs.S = 0
        attempt("ln.S = 0", ln=no_slabs)
        attempt("a cache kind of the other operand type", kv_kind=KV_F32 if kind == KV_BF16 else KV_BF16)
        rc, out = x.launch(lib)          # and the base shape is taken
        _check(lib, rc)
        assert torch.isfinite(_val(dt, out[:2].contiguous())).all()


# ---- the batch path's decode attention with the fused producer, on its own ------------------------------------------------
@pytest.mark.parametrize("n_keys,append", [(1, 1), (9, 1), (32, 1), (33, 0), (197, 0)])
@pytest.mark.parametrize("dt", DTYPES)
def test_decode_attention_fused_producer(lib, dt, n_keys, append):
    """q (and with append_kv the newest k / v) finished inside the attention unit from split-K partial sums: against float64,
    against the q-given kernel fed the finished q (and a cache that already holds the finished k / v), and the cache itself."""
    R, H, S = 5, 3, 3
    Dh, kv_ld, ta = H * 64, n_keys + 2, _att_dtype(dt)
    q_ld, col0 = (3 * Dh, 0) if append else (Dh + 64, 64)
    g = torch.Generator().manual_seed(100 * n_keys + append)
    part = torch.randn(S, R, q_ld, generator=g)
    bias = torch.randn(q_ld - col0, generator=g) * 0.5
    kc, vc = torch.randn(R, H, kv_ld, 64, generator=g).to(ta), torch.randn(R, H, kv_ld, 64, generator=g).to(ta)
    fin = _finish32(part[:, :, col0:], bias).to(ta)
    q = fin[:, :Dh].contiguous()
    want_k, want_v = kc.clone(), vc.clone()
    if append:
        want_k[:, :, n_keys - 1] = fin[:, Dh:2 * Dh].reshape(R, H, 64)
        want_v[:, :, n_keys - 1] = fin[:, 2 * Dh:].reshape(R, H, 64)
    p = torch.softmax(torch.einsum("rhd,rhjd->rhj", q.double().view(R, H, 64), want_k.double()[:, :, :n_keys]) * 0.125, -1)
    ref = torch.einsum("rhj,rhjd->rhd", p, want_v.double()[:, :, :n_keys]).reshape(R, Dh)
    # q_bias is indexed like a q_part row: the head's columns from col0 on
    bias_d = torch.cat([torch.zeros(col0), bias]).cuda()
    kd, vd, out = kc.cuda(), vc.cuda(), _nan(dt, R + 1, Dh)
    _check(lib, _fused_attention(lib, dt, part.cuda(), S, bias_d, q_ld, col0, append, _p(kd), _p(vd), None, 0, 1, kv_ld, n_keys, out, R, H))
    assert torch.isnan(out[R:]).all()
    got = _val(dt, out[:R].contiguous())
    err = (got - ref).abs().max().item()
    print(f"fused decode attention {dt} keys {n_keys}: err {err:.3e}")
    assert torch.isfinite(got).all() and err < TOL_ATT[dt]
    assert torch.equal(kd.cpu(), want_k) and torch.equal(vd.cpu(), want_v)
    plain, qd, kq, vq = _nan(dt, R, Dh), q.cuda(), want_k.cuda(), want_v.cuda()
    _check(lib, lib.cap_op_decode_attention(TAG[dt], C.c_void_p(_p(qd)), C.c_void_p(_p(kq)), C.c_void_p(_p(vq)), None, 0, 1,
                                            kv_ld, n_keys, C.c_void_p(_p(plain)), R, H, 0, _stream()))
    torch.cuda.synchronize()
    assert _same_bits(out[:R], plain)
