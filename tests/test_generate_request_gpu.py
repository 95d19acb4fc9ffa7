"""GPU: `cap_generate_request` (one `CapGenerateArgs`) against the five entry points that are conveniences over it.

1. Every legacy entry point and the request call with the equivalent struct write the same bits into every output buffer, the
   untouched tails included (both sides start from the same sentinel fill).
2. A refused request launches nothing: return code, sentinels intact, `cap_last_decode_steps` unchanged, and the message names the
   entry point that was called.  Every case is a host-side refusal.
3. A NULL struct is refused by name.

Tiny architectures, "f32s", max_len 12 (40 for the one case about positions)."""
import ctypes as C
import functools

import pytest
import torch

from embodied_captioning_amd import _native as N

pytestmark = pytest.mark.gpu

L = 12
I_FILL, F_FILL = -7, 123.5          # what every output buffer holds before a call


@functools.lru_cache(maxsize=None)
def _model(kind):
    from embodied_captioning_amd import weights as W
    from embodied_captioning_amd.config import Blip2Arch, BlipArch, CocaArch
    if kind == "blip":
        arch = BlipArch.tiny()
        return arch, W.procedural_blip_state_dict(arch, 3, eos_boost=2.0)
    if kind == "coca":
        arch = CocaArch.tiny()
        return arch, W.procedural_coca_state_dict(arch, 3, eos_boost=2.0)
    arch = Blip2Arch.tiny()
    return arch, W.procedural_blip2_state_dict(arch, 3, eos_boost=2.0)


def _engine(kind, B, K=1, max_len=L, path="auto", max_prompt=0):
    from embodied_captioning_amd.engine import CaptionerEngine
    arch, sd = _model(kind)
    eng = CaptionerEngine(arch, dtype="f32s", max_batch=B, max_beams=K, max_len=max_len, max_prompt=max_prompt)
    eng.load_state_dict(sd)
    eng.set_decode_path(path)
    return eng


def _pixels(eng, B):
    from embodied_captioning_amd.weights import synthetic_pixels
    return synthetic_pixels(B, eng.arch.image_size, seed=3).cuda()


def _prompt(eng, rows):
    return torch.tensor([[getattr(eng.arch, "bos", None) or eng.arch.sot, 11 + r, 12 + r] for r in range(rows)], dtype=torch.int32, device="cuda")


def _buffers(eng, B, rows, steps, cols, max_len=L, acc_ld=516):
    """Every output buffer a request can name, sentinel-filled.  rows = B x beams of a search, steps = recorded logit steps, cols =
    log-prob columns."""
    i32 = lambda *s: torch.full(s, I_FILL, dtype=torch.int32, device="cuda")          # noqa: E731
    f32 = lambda *s: torch.full(s, F_FILL, dtype=torch.float32, device="cuda")        # noqa: E731
    return {"out_ids": i32(B, max_len), "out_len": i32(B), "out_scores": f32(B), "out_step_logits": f32(steps, rows, eng.arch.vocab),
            "out_logprobs": f32(B, cols), "out_scored": i32(B), "out_vocab": f32(B, acc_ld)}


def _request(px, B, bufs, use, max_len=L, **fields):
    """A CapGenerateArgs over the buffers named in `use`; the other outputs stay absent (their buffers must keep the sentinel)."""
    a = N.CapGenerateArgs(pixels=px.data_ptr(), pixel_fmt=N.CAP_PIX_F32_NCHW, B=B, num_beams=1, max_len=max_len, length_penalty=1.0)
    for name in use:
        setattr(a, name, bufs[name].data_ptr())
    if "out_vocab" in use:
        a.acc_ld = bufs["out_vocab"].shape[1]
    for k, v in fields.items():
        setattr(a, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    return a


def _call(eng, symbol, a):
    """The request `a` through `symbol`: the request call itself, or the legacy entry point with the arguments it has."""
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    h, lp = eng._h, C.c_float(a.length_penalty)
    if symbol == "cap_generate_request":
        return eng.lib.cap_generate_request(h, C.byref(a), s)
    head = (h, a.pixels, a.pixel_fmt, a.B)
    greedy_outs = (a.out_step_logits, a.out_logprobs, a.out_scored, a.out_vocab, a.acc_ld)
    if symbol == "cap_generate":
        return eng.lib.cap_generate(*head, a.num_beams, a.max_len, lp, a.out_ids, a.out_len, a.out_scores, a.out_step_logits, s)
    if symbol == "cap_generate_scored":
        return eng.lib.cap_generate_scored(*head, a.num_beams, a.max_len, lp, a.out_ids, a.out_len, a.out_scores, a.out_step_logits,
                                           a.out_logprobs, a.out_scored, s)
    if symbol == "cap_generate_vocab":
        return eng.lib.cap_generate_vocab(*head, a.max_len, a.out_ids, a.out_len, *greedy_outs, s)
    if symbol == "cap_generate_prompted":
        return eng.lib.cap_generate_prompted(*head, a.max_len, a.prompt_ids, a.prompt_rows, a.prompt_len, a.out_ids, a.out_len,
                                             *greedy_outs, s)
    assert symbol == "cap_generate_groups"
    return eng.lib.cap_generate_groups(*head, a.num_beams, a.num_beam_groups, a.max_len, lp, a.out_ids, a.out_len, a.out_scores, s)


BASE = ("out_ids", "out_len")
GREEDY = BASE + ("out_step_logits", "out_logprobs", "out_scored", "out_vocab")
# id: (model, B, beams of the handle, legacy symbol, buffers in use, request fields, prompt rows)
EQUAL_CASES = {
    "blip_greedy": ("blip", 3, 1, "cap_generate", BASE + ("out_scores", "out_step_logits"), {}, 0),
    "blip_beams": ("blip", 2, 3, "cap_generate", BASE + ("out_scores", "out_step_logits"), {"num_beams": 3}, 0),
    "blip_scored": ("blip", 3, 1, "cap_generate_scored", BASE + ("out_logprobs", "out_scored"), {}, 0),
    "blip_vocab": ("blip", 3, 1, "cap_generate_vocab", GREEDY, {}, 0),
    "blip_prompt_shared": ("blip", 3, 1, "cap_generate_prompted", GREEDY, {}, 1),
    "blip_prompt_rows": ("blip", 3, 1, "cap_generate_prompted", GREEDY, {}, 3),
    "coca_groups_6_3": ("coca", 2, 6, "cap_generate_groups", BASE + ("out_scores",), {"num_beams": 6, "num_beam_groups": 3}, 0),
    "coca_groups_3_3": ("coca", 2, 3, "cap_generate_groups", BASE + ("out_scores",), {"num_beams": 3, "num_beam_groups": 3}, 0),
    "coca_scored": ("coca", 3, 1, "cap_generate_scored", BASE + ("out_logprobs", "out_scored"), {}, 0),
    "blip2_vocab": ("blip2", 3, 1, "cap_generate_vocab", GREEDY, {}, 0),
    "blip_17_rows": ("blip", 17, 1, "cap_generate", BASE, {}, 0),
}


@pytest.mark.parametrize("case", sorted(EQUAL_CASES))
def test_each_legacy_entry_point_equals_the_request_call(case):
    kind, B, K, symbol, use, fields, prompt_rows = EQUAL_CASES[case]
    eng = _engine(kind, B, K, max_prompt=3 if prompt_rows else 0)
    px = _pixels(eng, B)
    fields = dict(fields)
    P = 0
    if prompt_rows:
        prompt = _prompt(eng, prompt_rows)
        P = prompt.shape[1]
        fields.update(prompt_ids=prompt, prompt_rows=prompt_rows, prompt_len=P)
    beams = fields.get("num_beams", 1) // fields.get("num_beam_groups", 1)
    greedy = beams == 1 and "num_beam_groups" not in fields          # the greedy loop leaves out_scores alone
    cols = L if kind == "blip2" else L - 1
    sides = {}
    for sym in (symbol, "cap_generate_request"):
        bufs = _buffers(eng, B, B * beams, cols - max(P - 1, 0), cols)
        rc = _call(eng, sym, _request(px, B, bufs, use, **fields))
        torch.cuda.synchronize()
        assert rc == 0, N.last_error()
        sides[sym] = (bufs, eng.last_decode_steps, eng.last_decode_path, eng.last_row_compaction, eng.last_prefill_passes)
    (old, *old_state), (new, *new_state) = sides[symbol], sides["cap_generate_request"]
    assert old_state == new_state
    for name in old:
        assert torch.equal(old[name], new[name]), name
        touched = bool((old[name] != (I_FILL if old[name].dtype == torch.int32 else F_FILL)).any())
        assert touched == (name in use and not (name == "out_scores" and greedy)), name      # an absent buffer is never written
    if case == "blip_17_rows":          # the batch kernels and row compaction behind the request call (3 rows take the small path)
        assert new_state[1:3] == ["batch", True]
    if case == "blip_greedy":
        assert new_state[1] == "small"
    if case == "coca_groups_3_3":       # a group of one beam is a 1-beam BEAM search: it returns scores, the greedy loop does not
        assert bool((new["out_scores"] != F_FILL).all())
    eng.close()


# id: (model, handle (B, beams, max_len, path), legacy symbol, buffers in use, request fields, prompt rows [0 = none])
REFUSED = {
    "logprobs_without_scored": ("blip", (3, 1, L, "auto"), "cap_generate_scored", BASE + ("out_logprobs",), {}, 0),
    "logprobs_with_two_beams": ("blip", (3, 2, L, "auto"), "cap_generate_scored", BASE + ("out_logprobs", "out_scored"), {"num_beams": 2}, 0),
    "vocab_acc_ld_below_vocab": ("blip", (3, 1, L, "auto"), "cap_generate_vocab", GREEDY, {"acc_ld": 508}, 0),
    "vocab_acc_ld_not_multiple_of_4": ("blip", (3, 1, L, "auto"), "cap_generate_vocab", GREEDY, {"acc_ld": 514}, 0),
    "vocab_misaligned_pointer": ("blip", (3, 1, L, "auto"), "cap_generate_vocab", GREEDY, {"misalign": True}, 0),
    "prompted_acc_ld_below_vocab": ("blip", (3, 1, L, "auto"), "cap_generate_prompted", GREEDY, {"acc_ld": 508}, 1),
    "prompt_on_coca": ("coca", (3, 1, L, "auto"), "cap_generate_prompted", BASE, {}, 1),
    "prompt_on_blip2": ("blip2", (3, 1, L, "auto"), "cap_generate_prompted", BASE, {}, 1),
    "prompt_rows_2_at_B_3": ("blip", (3, 1, L, "auto"), "cap_generate_prompted", BASE, {}, 2),
    "prompt_len_1": ("blip", (3, 1, L, "auto"), "cap_generate_prompted", BASE, {"prompt_len": 1}, 1),
    "prompt_len_max_len": ("blip", (3, 1, L, "auto"), "cap_generate_prompted", BASE, {"prompt_len": L}, 1),
    "groups_on_blip": ("blip", (2, 6, L, "auto"), "cap_generate_groups", BASE + ("out_scores",), {"num_beams": 6, "num_beam_groups": 3}, 0),
    "six_beams_in_four_groups": ("coca", (2, 6, L, "auto"), "cap_generate_groups", BASE + ("out_scores",), {"num_beams": 6, "num_beam_groups": 4}, 0),
    "blip2_with_two_beams": ("blip2", (3, 1, L, "auto"), "cap_generate", BASE, {"num_beams": 2}, 0),
    "forced_small_path_at_17_rows": ("blip", (17, 1, L, "small"), "cap_generate", BASE, {}, 0),
    "forced_small_path_with_max_len_40": ("blip", (3, 1, 40, "small"), "cap_generate", BASE, {"max_len": 40}, 0),
}


@pytest.mark.parametrize("through", ["legacy", "request"])
@pytest.mark.parametrize("case", sorted(REFUSED))
def test_a_refused_request_launches_nothing(case, through):
    """Every row is refused on the host, before the zero fill of the outputs and before the image side: all sentinels survive and the
    handle's step count stays.  The two forced-small-path rows are the one intended change of behaviour of the request refactor:
    before it they failed after the encoder had run (the outputs were already zero-filled and the sequence state initialised).
    A BLIP-2 handle cannot be created with max_beams 2, so for `blip2_with_two_beams` the capacity rule is the one that fires."""
    kind, (B, K, max_len, path), symbol, use, fields, prompt_rows = REFUSED[case]
    eng = _engine(kind, B, K, max_len, path, max_prompt=3 if prompt_rows and kind == "blip" else 0)
    px = _pixels(eng, B)
    fields = dict(fields)
    bufs = _buffers(eng, B, B * K, 1, max_len, max_len=max_len)
    if prompt_rows:
        prompt = _prompt(eng, prompt_rows)
        fields = dict({"prompt_ids": prompt, "prompt_rows": prompt_rows, "prompt_len": prompt.shape[1]}, **fields)
    misalign = fields.pop("misalign", False)
    a = _request(px, B, bufs, use, **fields)
    if misalign:
        a.out_vocab = bufs["out_vocab"].data_ptr() + 4
        a.acc_ld = 512
    who = symbol if through == "legacy" else "cap_generate_request"
    steps_before = eng.last_decode_steps
    rc = _call(eng, who, a)
    msg = N.last_error()
    torch.cuda.synchronize()
    assert rc != 0 and who + ":" in msg, (rc, msg)
    assert eng.last_decode_steps == steps_before
    for name, t in bufs.items():
        assert bool((t == (I_FILL if t.dtype == torch.int32 else F_FILL)).all()), name
    if case.startswith("forced_small_path"):
        assert "small-batch decode path was forced" in msg
        eng.set_decode_path("auto")          # the same request is served once nothing is forced
        assert _call(eng, who, a) == 0, N.last_error()
        torch.cuda.synchronize()
    eng.close()


def test_the_request_call_refuses_a_null_struct_by_name():
    eng = _engine("blip", 2)
    before = eng.last_decode_steps
    rc = eng.lib.cap_generate_request(eng._h, None, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc != 0 and "cap_generate_request" in N.last_error() and "null request" in N.last_error()
    assert eng.last_decode_steps == before
    eng.close()
