"""CPU: the host side of sampling (captioner/sampling.py, the engine's key layout) and the restatement the GPU tests compare with
(tests/_sampling_ref.py): Philox4x32-10 known answers, the restatement's kept set and probabilities against HF's own warpers
(tests/golden/sampling_warpers.npz, tools/make_goldens_sampling.py), the refusals of `validate_sampling` by message, the key layout
of `num_return_sequences` and of a pool's batches, and the chi-square of the restatement's own draws on the distribution fixture."""
import os
import types

import numpy as np
import pytest

import _sampling_ref as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampling_warpers.npz")


def _hex(words):
    return " ".join(f"{int(w):08x}" for w in words)


def test_philox_known_answers():
    f = 0xFFFFFFFF
    assert _hex(S.philox4x32_10((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert _hex(S.philox4x32_10((f, f, f, f), (f, f))) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    # the digits-of-pi vector of the Random123 distribution
    assert _hex(S.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))) == \
        "d16cfe09 94fdcceb 5001e420 24126ea1"
    # the counter layout of a draw: (j, 0, key_lo, key_hi), key (seed_lo, seed_hi), U = (out0 << 32) | out1; scalar = vectorised
    seed, key, j = 0x0123456789ABCDEF, 0xFEDCBA9876543210, 5
    o = S.philox4x32_10((j, 0, key & f, key >> 32), (seed & f, seed >> 32))
    assert S.uniform64(seed, key, j) == (int(o[0]) << 32) | int(o[1])
    many = S.uniform64(seed, np.array([key, 1, 2], dtype=np.uint64), j)
    assert int(many[0]) == S.uniform64(seed, key, j) and int(many[2]) == S.uniform64(seed, 2, j)
    assert S.uniform64(seed, key, j) != S.uniform64(seed, key, j + 1) != S.uniform64(seed + 1, key, j + 1)


def test_restatement_against_the_hf_warpers():
    g = np.load(GOLDEN)
    off = g["offsets"]
    assert len(g["V"]) >= 20
    for c in range(len(g["V"])):
        V, seed, T, k, p = int(g["V"][c]), int(g["seed"][c]), float(g["temperature"][c]), int(g["top_k"][c]), float(g["top_p"][c])
        ids, probs = g["ids"][off[c]:off[c + 1]], g["probs"][off[c]:off[c + 1]].astype(np.float64)
        ref = S.reference(S.golden_row(seed, V), T, k, p)
        assert not ref["topk_tie"] and not ref["edge"]
        mine = np.flatnonzero(ref["w"] > 0)
        assert np.array_equal(mine, ids), (V, seed, T, k, p, len(mine), len(ids))
        pr = ref["w"][mine] / ref["total"]
        # weights below 2^-40 of the maximum are cut: none here, or the kept ids would differ
        assert np.abs(pr / probs - 1.0).max() < 1e-6, (V, seed, T, k, p, np.abs(pr / probs - 1.0).max())


def test_restatement_edge_cases():
    row = np.array([0.5, -np.inf, np.nan, 0.5, 0.25, -60.0], dtype=np.float32)
    ref = S.reference(row, 1.0, 0, 1.0)
    assert ref["kept"] == 3 and ref["w"][1] == 0 and ref["w"][2] == 0 and ref["w"][5] == 0       # exp(-60.5) < 2^-40
    ref = S.reference(row, 1.0, 1, 1.0)                                                          # ties with the k-th value stay
    assert ref["kept"] == 2 and ref["topk_tie"]
    ref = S.reference(row, 0.5, 0, 1e-6)                                                         # the maximal value always stays, ties together
    assert ref["kept"] == 2
    empty = S.reference(np.full(8, -np.inf, dtype=np.float32), 1.0, 3, 0.5)
    assert empty["kept"] == 0 and S.draw(empty, 123) == 0 and S.check_draw(empty, 0, 123) is None
    # the draw walks ids in ascending order; U = 0 gives the first token with weight, U = 2^64 - 1 the last
    ref = S.reference(row, 1.0, 0, 1.0)
    assert S.draw(ref, 0) == 0 and S.draw(ref, 2 ** 64 - 1) == 4
    assert S.check_draw(ref, 0, 0) is None and S.check_draw(ref, 4, 2 ** 64 - 1) is None
    assert S.check_draw(ref, 4, 0) is not None and S.check_draw(ref, 1, 0) is not None


def test_validate_sampling_refusals():
    from embodied_captioning_amd.captioner.sampling import validate_sampling
    from embodied_captioning_amd.config import BlipArch, CocaArch
    assert validate_sampling() == (False, 1.0, 0, 1.0, 0)
    assert validate_sampling(True, 0.7, 50, 0.9, 2 ** 64 - 1, BlipArch.tiny()) == (True, float(np.float32(0.7)), 50, float(np.float32(0.9)), 2 ** 64 - 1)
    for kw, word in (({"temperature": 0}, "temperature must be"), ({"temperature": -1.0}, "temperature must be"),
                     ({"temperature": float("inf")}, "temperature must be"), ({"temperature": float("nan")}, "temperature must be"),
                     ({"temperature": "1"}, "temperature must be"), ({"temperature": True}, "temperature must be"),
                     ({"temperature": 1e-60}, "temperature must be"),
                     ({"top_k": -1}, "top_k must be"), ({"top_k": 1.5}, "top_k must be"), ({"top_k": True}, "top_k must be"),
                     ({"top_p": 0.0}, "top_p must be"), ({"top_p": 1.0001}, "top_p must be"), ({"top_p": float("nan")}, "top_p must be"),
                     ({"top_p": -0.5}, "top_p must be"), ({"seed": -1}, "seed must be"), ({"seed": 2 ** 64}, "seed must be"),
                     ({"seed": 1.0}, "seed must be")):
        with pytest.raises(ValueError, match=word):
            validate_sampling(True, **kw)
    with pytest.raises(ValueError, match="CoCa"):
        validate_sampling(True, 0.7, arch=CocaArch.tiny())
    assert validate_sampling(False, 0.7, arch=CocaArch.tiny())[0] is False               # the state may be held, off


def test_resolve_sampling_and_the_wrappers_keys():
    from embodied_captioning_amd.captioner.sampling import reject_sampling_keys, resolve_sampling
    from embodied_captioning_amd.captioner.utils.utils import Configuration
    from embodied_captioning_amd.config import BlipArch
    a = BlipArch.tiny()
    cfg = Configuration(arch_name="blip", do_sample=True, temperature=0.7, top_k=50, top_p=0.9, sample_seed=5, num_return_sequences=4).captioner
    assert resolve_sampling(cfg, a, 8) == (True, float(np.float32(0.7)), 50, float(np.float32(0.9)), 5, 4)
    assert resolve_sampling(Configuration(arch_name="blip").captioner, a, 8) == (False, 1.0, 0, 1.0, 0, 1)
    assert resolve_sampling(Configuration(arch_name="blip", top_k=1, temperature=1.0).captioner, a, 8)[0] is False
    for kw, word in (({"temperature": 0.5}, "temperature=0.5"), ({"top_k": 5}, "top_k=5"), ({"num_return_sequences": 3}, "num_return_sequences = 3 needs"),
                     ({"sample_seed": 3}, "sample_seed"), ({"do_sample": True, "top_p": 2.0}, r"captioner\.top_p must be"),
                     ({"do_sample": True, "num_return_sequences": 9}, "exceeds batch_size"),
                     ({"do_sample": True, "num_return_sequences": 0}, "num_return_sequences must be")):
        with pytest.raises(ValueError, match=word):
            resolve_sampling(Configuration(arch_name="blip", **kw).captioner, a, 8)
    with pytest.raises(ValueError, match="beam sampling is not built"):
        resolve_sampling(Configuration(arch_name="blip", do_sample=True, num_beams=3).captioner, a, 8, num_beams=3)
    for kw in ({"do_sample": True}, {"sample_seed": 1}, {"num_return_sequences": 2}):
        with pytest.raises(ValueError, match=r"CoCa\(cfg\): captioner\." + next(iter(kw))):
            reject_sampling_keys(Configuration(arch_name="coca", **kw).captioner, "CoCa(cfg)")
    reject_sampling_keys(Configuration(arch_name="coca", do_sample=False, num_return_sequences=1).captioner, "CoCa(cfg)")
    reject_sampling_keys(types.SimpleNamespace(), "CoCa(cfg)")
    # the plugin forwards the keys
    import inspect
    from embodied_captioning_amd.utils.predictor_utils import Captioner
    src = inspect.getsource(Captioner.get_captioner)
    assert all(f'"{k}"' in src for k in ("do_sample", "temperature", "top_k", "top_p", "sample_seed", "num_return_sequences"))


def test_key_layout():
    from embodied_captioning_amd.captioner.sampling import default_sample_keys, keys_tensor, return_sequence_keys
    k = default_sample_keys(3, 4)
    assert k.dtype == np.uint64 and k.tolist() == [(3 << 32) | r for r in range(4)]
    # num_return_sequences = n: caption r of image b has key (call_no << 32) | (b * n + r), image-major
    k = return_sequence_keys(2, 3, 4).reshape(3, 4)
    assert all(int(k[b, r]) == (2 << 32) | (b * 4 + r) for b in range(3) for r in range(4))
    with pytest.raises(ValueError, match="32 bits"):
        default_sample_keys(2 ** 32, 1)
    # any 64 bits travel through the int64 tensor the engine uploads
    import torch
    big = np.array([2 ** 64 - 1, 1 << 63, 5], dtype=np.uint64)
    t = keys_tensor(big, 3)
    assert t.dtype == torch.int64 and t.numpy().view(np.uint64).tolist() == big.tolist()
    assert torch.equal(keys_tensor(t, 3), t) and keys_tensor([1, 2, 3], 3).tolist() == [1, 2, 3]
    with pytest.raises(ValueError, match="one key per caption"):
        keys_tensor(t, 4)
    with pytest.raises(ValueError, match="int64"):
        keys_tensor(torch.zeros(3, dtype=torch.int32), 3)
    # a pool numbers the BATCHES of generate_many from its own counter, before any plan: batch j = call counter + j
    from embodied_captioning_amd.engine import EnginePool
    pool = types.SimpleNamespace()
    ks = EnginePool.batch_sample_keys(pool, [4, 2, 3])
    assert [x.numpy().view(np.uint64).tolist() for x in ks] == [[(j << 32) | r for r in range(n)] for j, n in enumerate([4, 2, 3])]
    ks = EnginePool.batch_sample_keys(pool, [2])
    assert ks[0].numpy().view(np.uint64).tolist() == [(3 << 32) | 0, (3 << 32) | 1] and pool._sample_call_no == 4
    # merged passes concatenate the batches' keys in plan order: every caption keeps the key of its own batch
    merged = torch.cat([EnginePool.batch_sample_keys(types.SimpleNamespace(), [2, 2])[j] for j in (0, 1)])
    assert merged.numpy().view(np.uint64).tolist() == [0, 1, (1 << 32), (1 << 32) | 1]


def test_generation_options_judgement_is_unchanged():
    from embodied_captioning_amd.captioner.generation_options import reject_unsupported_generation_options
    reject_unsupported_generation_options({"do_sample": False, "temperature": 1.0, "top_k": 1})
    for opts, word in (({"do_sample": True}, "do_sample=True"), ({"temperature": 0.5}, "temperature=0.5"), ({"top_k": 5}, "top_k=5")):
        with pytest.raises(ValueError, match=word):
            reject_unsupported_generation_options(opts)


def test_native_exports_match_the_header():
    import re
    from embodied_captioning_amd import _native
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "captioner_hip.h")).read()
    for name in ("cap_set_sampling", "cap_sampling", "cap_op_select_sampled", "cap_generate_sampled"):
        assert name in _native.EXPORTS and re.search(r"\b" + name + r"\(", header), name
    m = re.search(r"int cap_op_select_sampled\((.*?)\);", header, re.S)
    assert len(m.group(1).split(",")) == len(_native._SIGNATURES["cap_op_select_sampled"][1])
    m = re.search(r"int cap_set_sampling\((.*?)\);", header, re.S)
    assert len(m.group(1).split(",")) == len(_native._SIGNATURES["cap_set_sampling"][1])
    m = re.search(r"int cap_generate_sampled\((.*?)\);", header, re.S)
    assert len(m.group(1).split(",")) == len(_native._SIGNATURES["cap_generate_sampled"][1]) == 4
    assert len(_native.CapGenerateArgs._fields_) == 18          # the request struct is unchanged: the keys are the call's own argument


def test_distribution_fixture_chi_square_of_the_restatements_own_draws():
    """Seed 1234, keys 0 .. 4095, draws 0 .. 15: 65 536 draws of the restatement itself from the V = 64 fixture (T = 0.7, top_k = 12,
    top_p = 0.9: 8 tokens stay, the rarest at p = 0.035).  Pearson's chi-square is 16.36 on 7 degrees of freedom against the
    1 - 1e-6 quantile 41.87 (Wilson-Hilferty); over 40 other seeds the statistic averages 6.9."""
    row, T, k, p = S.distribution_fixture()
    ref = S.reference(row, T, k, p)
    probs = ref["w"] / ref["total"]
    assert ref["kept"] == 8 and 0.03 < probs[probs > 0].min() < 0.04 and ref["topp_margin"] > 100 * S.delta(ref)
    keys = np.arange(4096, dtype=np.uint64)
    counts = np.zeros(64, dtype=np.int64)
    for d in range(16):
        counts += np.bincount(S.draw_many(ref, S.uniform64(1234, keys, d)), minlength=64)
    assert S.draw(ref, S.uniform64(1234, 5, 3)) == int(S.draw_many(ref, S.uniform64(1234, np.array([5], dtype=np.uint64), 3))[0])
    stat, df = S.chi_square(counts, probs)
    assert df == 7 and abs(S.chi_square_quantile(7) - 41.87) < 0.01
    assert abs(stat - 16.36) < 0.01 and stat < S.chi_square_quantile(df)
