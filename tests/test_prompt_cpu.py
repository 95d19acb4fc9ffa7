"""CPU: the host half of text-prompted captioning (`generate(prompt_ids=)`, `captioner.prompt` / `captioner.prompt_ids`): the
validation that runs before anything is uploaded, the prompt string's tokenization against HF's, the pool's merge plan for
prompted batches, and the premise of the GPU bit-identity test - forcing a caption's own prefix through the fp32 restatement gives
that caption - on the HF fixtures."""
import numpy as np
import pytest
import torch

from _prompt_ref import prompted_greedy
from _util import golden_inputs, pad_to

from embodied_captioning_amd.config import Blip2Arch, BlipArch, CocaArch
from embodied_captioning_amd.engine import EnginePool, prompt_token_limit, validate_prompt_ids

A = BlipArch.tiny()
GOOD = [A.bos, 11, 12, 13]


def _v(ids, arch=A, batch=3, max_length=12, **kw):
    return validate_prompt_ids(ids, arch, batch, max_length, **kw)


def test_valid_prompts_pass_in_all_three_shapes():
    for ids, rows in ((GOOD, 1), ([GOOD], 1), (torch.tensor([GOOD] * 3), 3), (np.asarray([GOOD] * 3), 3)):
        t = _v(ids)
        assert t.dtype == torch.int32 and tuple(t.shape) == (rows, 4) and not t.is_cuda and t.is_contiguous()
        assert t[0].tolist() == GOOD


@pytest.mark.parametrize("ids,kw,needle", [
    ([A.bos, 11, A.vocab], {}, "out of range"),
    ([A.bos, -1, 12], {}, "out of range"),
    ([A.bos, 11, A.eos, 13], {}, "EOS"),
    ([A.bos, A.pad, 12], {}, "pad"),
    ([11, 12, 13], {}, "column 0 must be BOS"),
    ([[A.bos, 11, 12], [12, 11, 12], [A.bos, 11, 12]], {}, "column 0 must be BOS"),
    ([A.bos] + [11] * 16, {"limit": 16, "max_length": 40}, "limit is 16"),
    ([A.bos] + [11] * 40, {"max_length": 60}, "limit is 32"),
    ([A.bos] + [11] * 11, {}, "max_length is 12"),
    ([A.bos] + [11] * 12, {}, "max_length is 12"),
    ([A.bos], {}, "P >= 2"),
    ([GOOD] * 2, {}, "row count must be 1"),
    ([GOOD] * 4, {}, "row count must be 1"),
    (GOOD, {"num_beams": 3}, "num_beams = 3"),
    (GOOD, {"num_beam_groups": 1}, "num_beam_groups = 1"),
    ([float(A.bos), 11.0], {}, "integer token ids"),
    ([[GOOD]], {}, "shape"),
])
def test_bad_prompts_raise_and_name_the_fault(ids, kw, needle):
    with pytest.raises(ValueError, match=needle):
        _v(ids, **kw)


def test_other_architectures_refuse_a_prompt_by_name():
    with pytest.raises(ValueError, match="CoCa"):
        validate_prompt_ids([CocaArch.tiny().sot, 11, 12], CocaArch.tiny(), 1, 12)
    with pytest.raises(ValueError, match="BLIP-2"):
        validate_prompt_ids([2, 11, 12], Blip2Arch.tiny(), 1, 12)
    # the wrappers of the other families refuse the configuration keys before anything is built
    from embodied_captioning_amd.captioner.generation_options import reject_prompt_keys
    from embodied_captioning_amd.captioner.utils.utils import Configuration
    for key, val in (("prompt", "a picture of"), ("prompt_ids", [2, 11])):
        cfg = Configuration(arch_name="blip2", model_name="procedural-blip2:1", height=224, width=224, **{key: val}).captioner
        with pytest.raises(ValueError, match=f"captioner.{key}.*blip"):
            reject_prompt_keys(cfg, "BLIP2(cfg)")
    reject_prompt_keys(Configuration(arch_name="coca", height=224, width=224).captioner, "CoCa(cfg)")
    # CoCa's `text=` stays a rejected generation option
    from embodied_captioning_amd.captioner.generation_options import _NEUTRAL, reject_unsupported_generation_options
    assert "text" in _NEUTRAL
    with pytest.raises(ValueError, match="text="):
        reject_unsupported_generation_options({"text": "a photo"}, "CoCa.generate")


def test_blip2_and_coca_wrappers_refuse_the_keys_before_the_library_is_touched():
    from embodied_captioning_amd.captioner.utils.utils import Configuration
    from embodied_captioning_amd.captioner.utils.utils_captioner import select_captioner
    for arch_name, model in (("blip2", "procedural-blip2:1"), ("coca", "procedural-tiny:1")):
        cfg = Configuration(arch_name=arch_name, model_name=model, height=224, width=224, prompt_ids=[2, 11, 12]).captioner
        with pytest.raises(ValueError, match="captioner.prompt_ids"):
            select_captioner(cfg)


def test_prompt_limit_follows_the_workspace_rows():
    assert prompt_token_limit(1, 1, 0) == 2                 # one decode row: one prefill position
    assert prompt_token_limit(8, 1, 0) == 9
    assert prompt_token_limit(1, 1, 16) == 16               # capacity reserved at creation
    assert prompt_token_limit(256, 1, 0) == 32              # the library's CAP_MAX_PROMPT
    assert prompt_token_limit(2, 3, 4) == 7


def test_prompt_and_prompt_ids_both_given_and_string_without_tokenizer():
    from embodied_captioning_amd.captioner.models.blip.blip import resolve_prompt
    with pytest.raises(ValueError, match="both given"):
        resolve_prompt("a picture of", GOOD, None, A)
    with pytest.raises(ValueError, match="no tokenizer"):
        resolve_prompt("a picture of", None, None, A)
    assert resolve_prompt(None, None, None, A) is None
    assert resolve_prompt(None, GOOD, None, A) == GOOD
    assert resolve_prompt(None, torch.tensor([GOOD, GOOD]), None, A) == [GOOD, GOOD]
    # the wrapper resolves the configured keys before it creates an engine: both errors need no GPU
    from embodied_captioning_amd.captioner.utils.utils import Configuration
    from embodied_captioning_amd.captioner.utils.utils_captioner import select_captioner
    for kw, needle in (({"prompt": "a picture of"}, "no tokenizer"), ({"prompt": "a", "prompt_ids": GOOD}, "both given"),
                       ({"prompt_ids": [A.bos, 11, A.eos]}, "EOS"), ({"prompt_ids": GOOD, "num_beams": 3}, "num_beams = 3"),
                       ({"prompt_ids": [GOOD, GOOD]}, "ONE prompt for every caption")):
        cfg = Configuration(arch_name="blip", model_name="procedural-tiny:3:2.0", height=224, width=224, max_length=12, **kw).captioner
        with pytest.raises(ValueError, match=needle):
            select_captioner(cfg)


def test_prompt_string_is_tokenized_as_hf_does(tmp_path):
    """HF: `processor(images, text)` -> BertTokenizer ids [CLS] words [SEP]; `generate` sets column 0 to BOS and passes
    input_ids[:, :-1] to the decoder (modeling_blip.py:858-932)."""
    transformers = pytest.importorskip("transformers")
    from embodied_captioning_amd.captioner.models.blip.blip import resolve_prompt
    words = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", "a", "picture", "of", "the", "dog", "##s", "play", "##ing", ",", "red"]
    vocab = tmp_path / "vocab.txt"
    vocab.write_text("\n".join(words) + "\n")
    tok = transformers.BertTokenizer(str(vocab), do_lower_case=True)
    arch = BlipArch()
    for text in ("a picture of", "A Picture of the dogs playing, red", "the zebra"):
        hf = torch.tensor([tok(text).input_ids])
        hf[:, 0] = arch.bos                      # what BlipForConditionalGeneration.generate does to its input_ids ...
        want = hf[:, :-1][0].tolist()            # ... before the text decoder sees them
        got = resolve_prompt(text, None, tok, arch)
        assert got == want and got[0] == arch.bos and tok.sep_token_id not in got, (text, got, want)
    assert resolve_prompt("a picture of", None, tok, arch) == [arch.bos, 5, 6, 7]
    with pytest.raises(ValueError, match="no word"):
        resolve_prompt("", None, tok, arch)


def test_pool_plan_never_merges_unequal_prompt_lengths_and_keeps_row_order():
    rows = [8, 8, 8, 4, 4, 8, 8]
    plens = [4, 4, 4, 6, 6, 4, 4]
    for n_eng in (1, 2, 3):
        plan = EnginePool.coalesce_plan_prompted(rows, n_eng, 24, plens)
        assert [j for g in plan for j in g] == list(range(len(rows)))            # every batch once, in order
        for g in plan:
            assert len({plens[j] for j in g}) == 1, (plan, plens)                # one prompt length per pass
            assert sum(rows[j] for j in g) <= 24
    plan = EnginePool.coalesce_plan_prompted(rows, 1, 24, plens)
    assert plan == [[0, 1, 2], [3, 4], [5, 6]]
    assert EnginePool.coalesce_plan_prompted(rows, 1, 24, [4] * 7) == EnginePool.coalesce_plan(rows, 1, 24)
    # per-row prompts are concatenated in plan order; a shared row is expanded only where a pass mixes prompts
    mk = lambda j, r, P: torch.arange(r * P, dtype=torch.int32).reshape(r, P) + 1000 * j      # noqa: E731
    prompts = [mk(0, 8, 4), mk(1, 1, 4), mk(2, 8, 4), mk(3, 1, 6), mk(3, 1, 6), mk(5, 8, 4), mk(6, 8, 4)]
    merged = EnginePool.merge_prompts(plan, rows, prompts)
    assert [tuple(m.shape) for m in merged] == [(24, 4), (1, 6), (16, 4)]
    assert torch.equal(merged[0], torch.cat([prompts[0], prompts[1].expand(8, 4), prompts[2]]))
    assert torch.equal(merged[1], prompts[3]) and torch.equal(merged[2], torch.cat([prompts[5], prompts[6]]))
    with pytest.raises(ValueError, match="different lengths"):
        EnginePool.merge_prompts([[0, 3]], rows, prompts)
    # the split restores the per-batch outputs of prompted passes (sequences start with each batch's own prompt)
    outs_m = [{"sequences": torch.cat([m.expand(sum(rows[j] for j in g), m.shape[1]) if m.shape[0] == 1 else m,
                                       torch.zeros((sum(rows[j] for j in g), 2), dtype=torch.int32)], dim=1),
               "lengths": torch.arange(sum(rows[j] for j in g), dtype=torch.int32)} for g, m in zip(plan, merged)]
    outs = EnginePool.split_merged_outputs(plan, rows, outs_m)
    for j, o in enumerate(outs):
        assert o["sequences"].shape[0] == rows[j] == o["lengths"].shape[0]
        assert torch.equal(o["sequences"][:, :-2], prompts[j].expand(rows[j], prompts[j].shape[1]))
    # one shared prompt, or one per batch
    assert EnginePool._per_batch_prompts(GOOD, 3) == [GOOD] * 3
    assert EnginePool._per_batch_prompts([GOOD, [GOOD] * 8, torch.tensor(GOOD)], 3)[1] == [GOOD] * 8
    with pytest.raises(ValueError, match="2 prompts for 3 batches"):
        EnginePool._per_batch_prompts([GOOD, GOOD], 3)
    with pytest.raises(ValueError, match="flat list of ints or a tensor"):
        EnginePool._per_batch_prompts([GOOD], 3)                           # a shared prompt is never a nested list
    assert EnginePool._per_batch_prompts(torch.tensor([GOOD]), 3)[2].tolist() == [GOOD]


def test_forced_tokens_reproduce_hf_on_the_prompt_golden():
    g, meta, arch, sd, px = golden_inputs("blip_tiny_prompt")
    L = meta["max_length"]
    prompt = g["prompt_ids"]
    assert prompt.tolist() == meta["prompt_ids"] and prompt[0] == arch.bos and len(prompt) == 4
    ref = prompted_greedy(sd, arch, px, prompt, L)
    assert np.array_equal(ref["sequences"].numpy(), g["greedy_sequences"])
    assert np.array_equal(ref["lengths"].numpy(), g["greedy_lengths"]) and len(set(g["greedy_lengths"].tolist())) > 1
    T = ref["logits"].shape[0]
    live = g["greedy_live"][:T]
    assert float(g["greedy_margin"][g["greedy_live"]].min()) >= 5e-3
    np.testing.assert_allclose(ref["logits"].numpy()[live], g["greedy_logits_full"][:T][live], rtol=0, atol=1.1e-5)


@pytest.mark.parametrize("P", [2, 4, 6])
def test_own_prefix_as_the_prompt_gives_the_unprompted_caption(P):
    """The premise of the GPU bit-identity test, on HF's unprompted tiny fixture: a row prompted with its own first P tokens decodes to
    its own caption, with the logits of the steps from P - 1 on."""
    from oracle import blip_ref
    g, meta, arch, sd, px = golden_inputs("blip_tiny")
    L = meta["max_length"]
    hf = pad_to(g["greedy_sequences"], L, arch.pad)
    own = blip_ref.greedy_generate(sd, arch, px, max_length=L)
    assert np.array_equal(pad_to(own["sequences"].numpy(), L, arch.pad), hf)
    rows = [b for b in range(hf.shape[0]) if arch.eos not in hf[b, :P + 1] and arch.pad not in hf[b, :P + 1]]
    assert rows, "no caption of the fixture is longer than the prompt"
    ref = prompted_greedy(sd, arch, px[rows], hf[rows, :P], L)
    assert np.array_equal(ref["sequences"].numpy(), hf[rows])
    for j in range(ref["logits"].shape[0]):
        if P - 1 + j < len(own["logits"]):
            np.testing.assert_allclose(ref["logits"][j].numpy(), own["logits"][P - 1 + j][rows].numpy(), rtol=0, atol=1.1e-5)
