"""CPU: the host half of the probability-fusion pseudo-captions (captioner/pseudo_caption_fusion.py): hand-derived known answers
for the three functions with the reference's names, the CSR builder and the capacity bound behind `fuse_vocab_groups`, special
ids skipped in decoding, `fused_pseudo_captions` and the CLI on a fake captioner, beams refused by name, the new ABI symbols."""
import csv
import math
import os
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class FakeTokenizer:
    """ids -> "w<id>" words; 0 (pad), 1 (bos) and 2 (eos) are special."""
    all_special_ids = [0, 1, 2]

    def decode(self, ids, skip_special_tokens=False):
        return " ".join(f"w{int(i)}" for i in ids if not (skip_special_tokens and int(i) in self.all_special_ids))


def _probs():
    """Two captions over 6 tokens, dyadic so every mean is exact.  Per-caption maxima over the steps:
         caption A (3 steps): [1/2, 1/4, 1/2, 0,   1/8, 1/2]
         caption B (2 steps): [1/2, 1/4, 0,   1,   1/8, 0  ]
       mean:                  [1/2, 1/4, 1/4, 1/2, 1/8, 1/4]"""
    A = torch.tensor([[0.5, 0.25, 0.125, 0.0, 0.125, 0.0],
                      [0.25, 0.125, 0.5, 0.0, 0.0, 0.125],
                      [0.125, 0.0, 0.25, 0.0, 0.125, 0.5]], dtype=torch.float64)
    B = torch.tensor([[0.5, 0.25, 0.0, 0.125, 0.125, 0.0],
                      [0.0, 0.0, 0.0, 1.0, 0.0, 0.0]], dtype=torch.float64)
    return [A, B]


def test_host_functions_known_answers():
    from embodied_captioning_amd.captioner import pseudo_caption_fusion as F
    A, B = _probs()
    mA, mB = F.compute_max_tokens_probability(A), F.compute_max_tokens_probability(B)
    assert mA.tolist() == [0.5, 0.25, 0.5, 0.0, 0.125, 0.5] and mB.tolist() == [0.5, 0.25, 0.0, 1.0, 0.125, 0.0]
    mean = F.compute_average_tokens_probability(torch.stack([mA, mB]))
    assert mean.tolist() == [0.5, 0.25, 0.25, 0.5, 0.125, 0.25]
    # th 0.25: tokens 1, 2 and 5 sit exactly AT the threshold and are excluded (strict >); token 3 is high in caption B only
    ids, p = F.pseudo_caption_tokens([A, B], 0.25)
    assert ids.tolist() == [0, 3] and p.tolist() == [0.5, 0.5]
    assert F.generate_pseudo_caption([A, B], 0.25, FakeTokenizer()) == "w3"           # 0 is special
    assert F.generate_pseudo_caption([A, B], 0.2, FakeTokenizer()) == "w3 w5"         # 1 and 2 are special too
    assert F.generate_pseudo_caption([A, B], 0.1, lambda ids: "+".join(map(str, ids))) == "0+1+2+3+4+5"
    assert F.generate_pseudo_caption([A], 0.3, FakeTokenizer()) == "w5"               # one caption: its own maxima
    with pytest.raises(ValueError):
        F.generate_pseudo_caption([], 0.25, FakeTokenizer())
    with pytest.raises(TypeError):
        F.decode_tokens([1, 2], object())


def test_specials_are_skipped_for_each_family():
    from embodied_captioning_amd.captioner import pseudo_caption_fusion as F
    from embodied_captioning_amd.config import Blip2Arch, BlipArch, CocaArch

    class Cap:
        def __init__(self, arch):
            self.arch = arch

        def decode(self, ids):
            return " ".join(str(i) for i in ids)

    b, c, o = BlipArch.tiny(), CocaArch.tiny(), Blip2Arch.tiny()
    assert F.special_token_ids(b) == {b.bos, b.eos, b.pad}
    assert F.special_token_ids(c) == {c.sot, c.eos} and c.pad not in F.special_token_ids(c)     # CoCa's pad id is a real token
    assert F.special_token_ids(o) == {o.bos, o.eos, o.pad}
    ids = sorted({b.pad, b.eos, b.bos, 7, 9})
    assert F.decode_tokens(ids, Cap(b)) == "7 9"
    ids = sorted({c.pad, c.sot, c.eos, 5})
    assert F.decode_tokens(ids, Cap(c)) == " ".join(str(i) for i in sorted({c.pad, 5}))


def test_csr_builder_and_capacity_bound():
    from embodied_captioning_amd.engine import fusion_max_tokens, vocab_group_csr
    rows, off = vocab_group_csr([[4, 0], [], [2, 3, 1]], 5)
    assert rows.dtype == torch.int32 and off.dtype == torch.int32
    assert rows.tolist() == [4, 0, 2, 3, 1] and off.tolist() == [0, 2, 2, 5]
    rows, off = vocab_group_csr([], 5)
    assert rows.tolist() == [] and off.tolist() == [0]
    with pytest.raises(ValueError, match="outside"):
        vocab_group_csr([[0, 5]], 5)
    with pytest.raises(ValueError, match="outside"):
        vocab_group_csr([[-1]], 5)
    with pytest.raises(ValueError, match="more than once"):
        vocab_group_csr([[0, 1], [1]], 5)
    # K = ceil(steps / th) capped by the vocabulary; k tokens above th need k * th < sum_i mean(i) <= steps
    assert fusion_max_tokens(19, 0.25, 30522) == 76 and fusion_max_tokens(19, 0.5, 30522) == 38
    assert fusion_max_tokens(20, 0.3, 50272) == math.ceil(20 / 0.3) == 67
    assert fusion_max_tokens(19, 0.25, 40) == 40 and fusion_max_tokens(19, 0.0, 40) == 40
    g = torch.Generator().manual_seed(0)
    for steps, th in ((3, 0.25), (7, 0.1), (2, 0.5)):
        # the extreme case: every step a different flat distribution over few tokens
        p = torch.zeros((steps, 256), dtype=torch.float64)
        for t in range(steps):
            idx = torch.randperm(256, generator=g)[:3]
            p[t, idx] = 1.0 / 3
        kept = int((p.max(dim=0).values > th).sum())
        assert kept < steps / th <= fusion_max_tokens(steps, th, 256)


class FakeEngine:
    def fuse_vocab_groups(self, vmax, groups, th, max_tokens=None):
        K = max(1, max((int((vmax[g].mean(dim=0) > th).sum()) for g in groups if g), default=1))
        ids = torch.full((len(groups), K), -1, dtype=torch.int32)
        probs = torch.zeros((len(groups), K))
        counts = torch.zeros((len(groups),), dtype=torch.int32)
        for j, g in enumerate(groups):
            if not g:
                continue
            mean = vmax[g].mean(dim=0)
            keep = torch.where(mean > th)[0]
            counts[j] = len(keep)
            ids[j, :len(keep)] = keep.int()
            probs[j, :len(keep)] = mean[keep]
        return ids, probs, counts


class FakeCaptioner:
    """vocab_maxprob of a crop = a function of the crop's mean colour; texts name the crop's size."""
    V = 12

    def __init__(self):
        from embodied_captioning_amd.config import BlipArch
        self.arch = types.SimpleNamespace(bos=1, eos=2, pad=0)
        self.engine = FakeEngine()
        self.calls = []
        assert BlipArch                                         # (the package imports without a GPU)

    def decode(self, ids):
        return " ".join(f"w{i}" for i in ids)

    def generate_batch(self, images, output_vocab_maxprob=False):
        assert output_vocab_maxprob
        self.calls.append(len(images))
        v = torch.zeros((len(images), self.V))
        for r, im in enumerate(images):
            a = np.asarray(im)
            v[r, int(a[..., 0].mean()) % self.V] = 0.75         # red channel of the RGB crop
            v[r, 2] = 0.5                                       # the EOS id is always likely
            v[r, 11] = 0.125
        return {"texts": [f"{im.size[0]}x{im.size[1]}" for im in images], "vocab_maxprob": v}


def _write_records(tmp_path):
    from embodied_captioning_amd.pseudolabeler import record_name, save_record
    frames = [np.zeros((60, 80, 3), dtype=np.uint8), np.zeros((50, 70, 3), dtype=np.uint8)]
    frames[0][..., 2] = 5            # BGR frames: red = channel 2
    frames[1][..., 2] = 5
    frames[1][:, 40:, 2] = 7
    boxes = [[(0, 0, 20, 30), (10, 10, 50, 40)], [(0, 0, 30, 20), (45, 5, 65, 45)]]
    objs = [[1, 2], [1, 2]]
    for f, (fr, bx, ob) in enumerate(zip(frames, boxes, objs)):
        inst = {"captions": ["x"] * len(bx), "pred_boxes": [np.array(b, np.float32) for b in bx],
                "infos": [{"id_episode": 4, "id_object": o} for o in ob]}
        save_record(str(tmp_path), record_name(4, f)[:-4], inst, fr)


def test_fused_pseudo_captions_and_cli_on_a_fake_captioner(tmp_path):
    from embodied_captioning_amd import pseudocaptioner as P
    from embodied_captioning_amd.captioner import pseudo_caption_fusion as F
    rec = tmp_path / "records"
    rec.mkdir()
    _write_records(rec)
    grouped = P.group_records(sorted(str(p) for p in rec.glob("*.npz")), apply_filter=False)
    assert list(grouped) == [(4, 1), (4, 2)]
    cap = FakeCaptioner()
    out = F.fused_pseudo_captions(grouped, cap, th=0.25)
    assert cap.calls == [4]                                     # one batched generate for every crop of every group
    assert list(out) == ["(4, 1)", "(4, 2)"]
    # object 1: both crops red 5 -> token 5 at 0.75; object 2: red 5 and red 7 -> 0.375 each; token 2 (EOS) is skipped in the text
    assert out["(4, 1)"]["captions"] == ["20x30", "30x20"] and out["(4, 2)"]["captions"] == ["40x30", "20x40"]
    assert out["(4, 1)"]["token_ids"] == [2, 5] and out["(4, 1)"]["token_probs"] == [0.5, 0.75]
    assert out["(4, 1)"]["pseudo_caption"] == "w5"
    assert out["(4, 2)"]["token_ids"] == [2, 5, 7] and out["(4, 2)"]["token_probs"] == [0.5, 0.375, 0.375]
    assert out["(4, 2)"]["pseudo_caption"] == "w5 w7"
    # groups are batched up to rows_per_call crops
    cap2 = FakeCaptioner()
    assert F.fused_pseudo_captions(grouped, cap2, th=0.25, rows_per_call=2) == out and cap2.calls == [2, 2]
    # the CLI writes the reference's CSV
    path = tmp_path / "out.csv"
    rc = F.main(["--file_path", str(rec), "--output_csv_path", str(path), "--arch_name", "blip", "--th", "0.25"], captioner=FakeCaptioner())
    assert rc == 0
    rows = list(csv.reader(open(path)))
    assert rows[0] == ["episode_id", "object_id", "pseudo_caption"]
    assert rows[1:] == [["4", "1", "w5"], ["4", "2", "w5 w7"]]
    with pytest.raises(SystemExit):
        F.main(["--file_path", str(rec), "--output_csv_path", str(path), "--arch_name", "llm"])


def test_beams_and_beam_groups_are_refused_by_name():
    from embodied_captioning_amd._native import CaptionerHipError
    from embodied_captioning_amd.engine import CaptionerEngine
    eng = object.__new__(CaptionerEngine)                       # the refusal comes before anything touches the handle
    eng._h = None
    with pytest.raises(CaptionerHipError, match="num_beams = 3"):
        CaptionerEngine.generate(eng, None, num_beams=3, output_vocab_maxprob=True)
    with pytest.raises(CaptionerHipError, match="num_beam_groups = 3"):
        CaptionerEngine.generate(eng, None, num_beams=6, num_beam_groups=3, output_vocab_maxprob=True)


def test_library_exports_the_fusion_entry_points_and_pool_splits_the_new_output():
    from embodied_captioning_amd import _native, build
    from embodied_captioning_amd.engine import EnginePool
    build.build(verbose=False)
    lib = _native.load_library()
    text = open(os.path.join(ROOT, "include", "captioner_hip.h")).read()
    for name in ("cap_generate_vocab", "cap_op_select_vocab", "cap_op_vocab_group_threshold"):
        assert hasattr(lib, name) and name in _native.EXPORTS and name + "(" in text
    assert "vocab_maxprob" in EnginePool._PER_ROW_OUTPUTS
    v = torch.arange(5 * 8, dtype=torch.float32).reshape(5, 8)[:, :6]        # a view without its padding columns
    outs = EnginePool.split_merged_outputs([[0, 1]], [2, 3], [{"sequences": torch.zeros((5, 3)), "vocab_maxprob": v}])
    assert torch.equal(outs[0]["vocab_maxprob"], v[:2]) and torch.equal(outs[1]["vocab_maxprob"], v[2:])
    assert outs[1]["vocab_maxprob"].stride(0) == 8


@pytest.mark.parametrize("arch_name", ["blip", "coca", "blip2"])
def test_cli_builds_the_captioner_configuration_for_every_family(tmp_path, monkeypatch, arch_name):
    """main() without an injected captioner: argparse -> Configuration -> select_captioner (stubbed: no GPU here)."""
    from embodied_captioning_amd.captioner import pseudo_caption_fusion as F
    from embodied_captioning_amd.captioner.utils import utils_captioner
    rec = tmp_path / "records"
    rec.mkdir()
    _write_records(rec)
    seen = {}

    def fake_select(cfg):
        seen["cfg"] = cfg
        cap = FakeCaptioner()
        cap.eval = lambda: cap
        return cap

    monkeypatch.setattr(utils_captioner, "select_captioner", fake_select)
    path = tmp_path / "out.csv"
    argv = ["--file_path", str(rec), "--output_csv_path", str(path), "--arch_name", arch_name, "--batch_size", "32", "--streams", "2"]
    if arch_name == "blip":
        argv += ["--model", "procedural-tiny:4:2.0", "--dtype", "bf16"]
    assert F.main(argv) == 0
    cfg = seen["cfg"]
    assert cfg.arch_name == arch_name and cfg.batch_size == 32 and cfg.streams == 2 and cfg.device == "cuda:0"
    assert cfg.model_name == ("procedural-tiny:4:2.0" if arch_name == "blip" else F.DEFAULT_MODELS[arch_name])
    assert cfg.dtype == ("bf16" if arch_name == "blip" else None)
    assert [r[:2] for r in list(csv.reader(open(path)))[1:]] == [["4", "1"], ["4", "2"]]
