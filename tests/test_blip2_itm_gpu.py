"""GPU: the BLIP-2 image-text scorer (CAP_ARCH_BLIP2_ITM) against the float64 HF `Blip2ForImageTextRetrieval` goldens
(tools/make_goldens_blip2_itm.py; procedural weights), its batch invariance, the 364 px geometry, the pseudo-caption driver and the
ABI's refusals.

Bars come from the reference's own rounding, stored in the fixtures: the same HF model run in float32 / bfloat16 on the CPU against
its float64 self (`ref_err_fp32`, `ref_err_bf16`).  f32 / f32s: 8 x ref_err_fp32 (maximum absolute difference of every output);
bf16: 4 x ref_err_bf16 (features: 1 - cosine, as in the CLIP test).  The maxima a run reaches are printed (`-s`) and recorded in
profiles/blip2_itm_gpu_tolerances.txt.
"""
import ctypes as C
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ERR_KEYS = ("itc_image", "itc_text", "itc_scores", "itm_logits", "itm_prob", "itc_image_cos", "itc_text_cos")
DTYPES = ["f32", "f32s", "bf16"]


def _arch(name, pre=""):
    from embodied_captioning_amd.config import Blip2ItmArch
    if name == "blip2_itm_tiny":
        return Blip2ItmArch.tiny()
    return Blip2ItmArch.width(364 if pre else 224)


_FIX = {}


def _fixture(name, pre=""):
    """-> (golden arrays with the `pre` keys un-prefixed, arch, frames uint8 [n, S, S, 3])"""
    from embodied_captioning_amd.weights import synthetic_frames_u8
    if (name, pre) not in _FIX:
        raw = np.load(os.path.join(GOLDEN, f"{name}.npz"))
        g = {k[len(pre):]: raw[k] for k in raw.files if k.startswith(pre)} if pre else {k: raw[k] for k in raw.files if not k.startswith("s364_")}
        arch = _arch(name, pre)
        n = g["itc_image"].shape[0]
        frames = synthetic_frames_u8(n, arch.image_size, arch.image_size, seed=int(raw["frame_seed"])).numpy()
        _FIX[(name, pre)] = (g, arch, frames, int(raw["seed"]))
    return _FIX[(name, pre)][:3]


def _bars(g, dtype):
    err = dict(zip(ERR_KEYS, g["ref_err_bf16" if dtype == "bf16" else "ref_err_fp32"]))
    return {k: (4 if dtype == "bf16" else 8) * float(v) for k, v in err.items()}


_ENGINES = {}


def _engine(name, dtype, max_batch=48, pre=""):
    key = (name, dtype, max_batch, pre)
    if key not in _ENGINES:
        from embodied_captioning_amd.engine import Blip2ItmEngine
        from embodied_captioning_amd.weights import procedural_blip2_itm_state_dict
        _fixture(name, pre)
        arch, seed = _FIX[(name, pre)][1], _FIX[(name, pre)][3]
        eng = Blip2ItmEngine(arch, dtype=dtype, max_batch=max_batch)
        rep = eng.load_state_dict(procedural_blip2_itm_state_dict(arch, seed))
        assert rep["unknown"] == ["query_tokens"]          # (it enters as derived.qformer_x0)
        _ENGINES[key] = eng
    return _ENGINES[key]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()


def _feat_err(out, ref, dtype, bars, key):
    """f32 / f32s: maximum absolute difference; bf16: 1 - cosine (rows are unit vectors on both sides)."""
    out, ref = out.astype(np.float64), ref.astype(np.float64)
    if dtype == "bf16":
        err = float((1.0 - (out * ref).sum(-1) / (np.linalg.norm(out, axis=-1) * np.linalg.norm(ref, axis=-1))).max())
        return err, bars[key + "_cos"]
    return float(np.abs(out - ref).max()), bars[key]


def _text(g):
    return torch.from_numpy(g["ids"]), torch.from_numpy(g["lens"])


def _check_against_golden(name, dtype, pre=""):
    g, arch, frames = _fixture(name, pre)
    eng = _engine(name, dtype, pre=pre)
    bars = _bars(g, dtype)
    ids, lens = _text(g)
    ni = frames.shape[0]
    if dtype == "f32s":
        eng.saturations(reset=True)
    assert eng.encode_images(torch.from_numpy(frames)) == ni
    img = eng.itc_image_features()
    txt = eng.itc_text_features(ids, lens)
    logits, prob = eng.itm(ids[:ni], lens[:ni])              # the paired rows: image i with caption i (ITM after ITC, tower ran once)
    mat = eng.itc_scores(img, txt, paired=False)
    img_n, txt_n = img.cpu().numpy(), txt.cpu().numpy()
    assert np.allclose(np.linalg.norm(img_n, axis=-1), 1.0, atol=1e-5) and np.allclose(np.linalg.norm(txt_n, axis=-1), 1.0, atol=1e-5)
    e_img, b_img = _feat_err(img_n, g["itc_image"], dtype, bars, "itc_image")
    e_txt, b_txt = _feat_err(txt_n, g["itc_text"], dtype, bars, "itc_text")
    e_mat = float(np.abs(mat.cpu().numpy().astype(np.float64) - g["itc_scores"]).max())
    e_lg = float(np.abs(logits.cpu().numpy().astype(np.float64) - g["itm_logits"]).max())
    e_pr = float(np.abs(prob.cpu().numpy().astype(np.float64) - g["itm_prob"]).max())
    # the groups' pairs under both heads
    gi, gt = g["group_images"], g["group_captions"]
    eng.encode_images(torch.from_numpy(frames[gi.reshape(-1)]))
    g_lg, g_pr = eng.itm(ids[gt.reshape(-1)], lens[gt.reshape(-1)])
    e_lg = max(e_lg, float(np.abs(g_lg.cpu().numpy().astype(np.float64).reshape(g["group_itm_logits"].shape) - g["group_itm_logits"]).max()))
    g_pr = g_pr.cpu().numpy().astype(np.float64).reshape(gi.shape)
    e_pr = max(e_pr, float(np.abs(g_pr - g["group_itm"]).max()))
    g_itc = mat.cpu().numpy()[gi, gt]
    sat = eng.saturations() if dtype == "f32s" else 0
    qual = {}
    for head, sc, bar in (("itm", g_pr, bars["itm_prob"]), ("itc", g_itc, bars["itc_scores"])):
        ok = g[f"group_{head}_margin"] > 2 * bar
        qual[head] = int(ok.sum())
        for row, rank, use in zip(sc, g[f"group_{head}_rank"], ok):
            if use:          # HF's top-1 wherever HF's margin exceeds twice the mode's bar
                assert int(np.argsort(-row, kind="stable")[0]) == int(rank[0]), (head, row, rank)
    print(f"\n{name}{' ' + pre.rstrip('_') if pre else ''} {dtype}: itc_image {e_img:.3g} (bar {b_img:.3g})  itc_text {e_txt:.3g} (bar {b_txt:.3g})  "
          f"itc_scores {e_mat:.3g} (bar {bars['itc_scores']:.3g})  itm_logits {e_lg:.3g} (bar {bars['itm_logits']:.3g})  "
          f"itm_prob {e_pr:.3g} (bar {bars['itm_prob']:.3g})  qualifying groups itm {qual['itm']}/{len(gi)} itc {qual['itc']}/{len(gi)}  "
          f"f32s clamps {sat}")
    assert e_img < b_img and e_txt < b_txt, (e_img, b_img, e_txt, b_txt)
    assert e_mat < bars["itc_scores"], (e_mat, bars["itc_scores"])
    assert e_lg < bars["itm_logits"], (e_lg, bars["itm_logits"])
    assert e_pr < bars["itm_prob"], (e_pr, bars["itm_prob"])
    if dtype != "bf16":      # f32 / f32s: at least 3 of every 4 groups must have qualified (bf16: printed and recorded only)
        assert 4 * qual["itm"] >= 3 * len(gi) and 4 * qual["itc"] >= 3 * len(gi), qual
    assert sat == 0
    # paired ITC = the diagonal of the matrix, same bits (one kernel, same sum order)
    n = min(img.shape[0], txt.shape[0])
    assert torch.equal(eng.itc_scores(img[:n], txt[:n], paired=True), mat[torch.arange(n), torch.arange(n)])


@pytest.mark.parametrize("name", ["blip2_itm_tiny", "blip2_itm_width"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_itc_and_itm_match_hf_golden(name, dtype):
    _check_against_golden(name, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_364px_677_tokens_match_hf_golden(dtype):
    g, arch, frames = _fixture("blip2_itm_width", "s364_")
    assert arch.n_tokens == 677 and frames.shape[1] == 364
    _check_against_golden("blip2_itm_width", dtype, pre="s364_")


def _ragged(arch, n, seed):
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 33, size=n)
    lens[0], lens[1], lens[n - 1] = 32, 1, 7
    ids = np.zeros((n, 32), dtype=np.int64)
    for b, k in enumerate(lens):
        ids[b, :k] = rng.integers(3, arch.vocab, size=k)
        ids[b, 0] = 1
    return torch.from_numpy(ids), torch.from_numpy(lens)


@pytest.mark.parametrize("dtype", DTYPES)
def test_batch_invariance_same_bits(dtype):
    """A pair alone, in a full batch, last of a partial micro-batch, with garbage ids after its length and padded to L = 32 against
    its own length: torch.equal on every output.  ITM after ITC on the same image batch = ITM alone."""
    from embodied_captioning_amd.weights import synthetic_frames_u8
    g, arch, _ = _fixture("blip2_itm_tiny")
    B = 64
    eng = _engine("blip2_itm_tiny", dtype, max_batch=B)
    frames = synthetic_frames_u8(B, arch.image_size, arch.image_size, seed=99)
    ids, lens = _ragged(arch, B, 7)
    eng.encode_images(frames)
    lg_alone_first, pr_alone_first = eng.itm(ids, lens)                  # ITM alone on a fresh image batch
    eng.encode_images(frames)
    img = eng.itc_image_features()
    txt = eng.itc_text_features(ids, lens)
    lg, pr = eng.itm(ids, lens)                                          # ITM after ITC on the same image batch
    assert torch.equal(lg, lg_alone_first) and torch.equal(pr, pr_alone_first)
    assert torch.isfinite(lg).all() and torch.isfinite(img).all() and torch.isfinite(txt).all()
    # garbage after each row's length (any valid or invalid id): nothing moves
    junk = ids.clone()
    rnd = torch.from_numpy(np.random.default_rng(1).integers(-5, arch.vocab + 5, size=tuple(ids.shape)))
    mask = torch.arange(32)[None, :] >= lens[:, None]
    junk[mask] = rnd[mask]
    lg_j, pr_j = eng.itm(junk.to("cuda"), lens.to("cuda"))               # (device tensors: the kernels clamp, the host does not look)
    assert torch.equal(lg_j, lg) and torch.equal(pr_j, pr)
    assert torch.equal(eng.itc_text_features(junk.to("cuda"), lens.to("cuda")), txt)
    # alone, at its own length (L = lens[i], not 32)
    for i in (0, 1, 17, B - 1):
        k = int(lens[i])
        eng.encode_images(frames[i:i + 1])
        a_lg, a_pr = eng.itm(ids[i:i + 1, :k], lens[i:i + 1])
        assert torch.equal(a_lg[0], lg[i]) and torch.equal(a_pr[0], pr[i]), i
        assert torch.equal(eng.itc_image_features()[0], img[i]), i
        assert torch.equal(eng.itc_text_features(ids[i:i + 1, :k], lens[i:i + 1])[0], txt[i]), i
        a32_lg, _ = eng.itm(ids[i:i + 1], lens[i:i + 1])                  # alone, padded to L = 32
        assert torch.equal(a32_lg[0], lg[i]), i
    # the end of a partial micro-batch, padded to that batch's own longest row
    sl = slice(40, 53)
    Lp = int(lens[sl].max())
    eng.encode_images(frames[sl])
    p_lg, p_pr = eng.itm(ids[sl, :Lp], lens[sl])
    assert torch.equal(p_lg, lg[sl]) and torch.equal(p_pr, pr[sl])
    assert torch.equal(eng.itc_image_features(), img[sl])
    assert torch.equal(eng.itc_text_features(ids[sl, :Lp], lens[sl]), txt[sl])
    # paired ITC scores = the diagonal of the full matrix
    mat = eng.itc_scores(img, txt, paired=False)
    assert mat.shape == (B, B)
    assert torch.equal(eng.itc_scores(img, txt, paired=True), mat.diagonal())


@pytest.mark.parametrize("dtype", DTYPES)
def test_batch_invariance_at_production_width_and_the_scorer_batch(dtype):
    """Production widths (ViT-g 1408 / 6144, Q-Former 768 / 3072, two layers per tower) at the scorer's micro-batch of 256: the GEMM
    tile the launcher picks depends on the row count there (one pair: the 64 x 64 tile; 256 pairs: the 128 / 256 tiles), so this is
    where 'alone = in a batch' rests on every tile forming the same sums.  torch.equal on every output."""
    from embodied_captioning_amd.weights import synthetic_frames_u8
    g, arch, _ = _fixture("blip2_itm_width")
    B = 256
    eng = _engine("blip2_itm_width", dtype, max_batch=B)
    frames = synthetic_frames_u8(B, arch.image_size, arch.image_size, seed=41)
    ids, lens = _ragged(arch, B, 11)
    eng.encode_images(frames)
    img = eng.itc_image_features()
    txt = eng.itc_text_features(ids, lens)
    lg, pr = eng.itm(ids, lens)
    assert torch.isfinite(lg).all() and torch.isfinite(img).all() and torch.isfinite(txt).all()
    for i in (0, 1, 130, B - 1):
        k = int(lens[i])
        eng.encode_images(frames[i:i + 1])
        a_lg, a_pr = eng.itm(ids[i:i + 1, :k], lens[i:i + 1])
        assert torch.equal(a_lg[0], lg[i]) and torch.equal(a_pr[0], pr[i]), i
        assert torch.equal(eng.itc_image_features()[0], img[i]), i
        assert torch.equal(eng.itc_text_features(ids[i:i + 1, :k], lens[i:i + 1])[0], txt[i]), i
    sl = slice(200, 237)                                   # the end of a partial micro-batch, padded to its own longest row
    Lp = int(lens[sl].max())
    eng.encode_images(frames[sl])
    p_lg, p_pr = eng.itm(ids[sl, :Lp], lens[sl])
    assert torch.equal(p_lg, lg[sl]) and torch.equal(p_pr, pr[sl])
    assert torch.equal(eng.itc_image_features(), img[sl])
    assert torch.equal(eng.itc_text_features(ids[sl, :Lp], lens[sl]), txt[sl])
    eng.close()
    _ENGINES.pop(("blip2_itm_width", dtype, B, ""))        # 256-pair arenas at production width: freed at once


def test_scorer_pairs_matrix_and_driver_end_to_end(tmp_path):
    from PIL import Image
    from embodied_captioning_amd import pseudocaptioner as P
    from embodied_captioning_amd.captioner.blip2_itm_scorer import Blip2ItmScorer
    from embodied_captioning_amd.pseudolabeler import record_name, save_record
    name = "procedural-blip2-itm-tiny:3"
    rng = np.random.default_rng(5)
    frames = [rng.integers(0, 256, size=(96, 128, 3), dtype=np.uint8), rng.integers(0, 256, size=(80, 100, 3), dtype=np.uint8)]
    boxes = [[(10, 12, 60, 70), (30, 5, 120, 90), (0, 0, 40, 40)], [(5, 5, 50, 60), (20, 10, 90, 70)]]
    caps = [["a red chair", "a wooden table", "a lamp"], ["a green sofa", "a tv"]]
    objs = [[1, 1, 2], [1, 2]]
    for f, (fr, bx, cp, ob) in enumerate(zip(frames, boxes, caps, objs)):
        inst = {"captions": cp, "pred_boxes": [np.array(b, np.float32) for b in bx], "infos": [{"id_episode": 0, "id_object": o} for o in ob]}
        save_record(str(tmp_path), record_name(0, f)[:-4], inst, fr)
    grouped = P.group_records(sorted(str(p) for p in tmp_path.glob("*.npz")))
    assert list(grouped) == [(0, 1), (0, 2)] and [len(v) for v in grouped.values()] == [3, 2]

    class IdScorer(Blip2ItmScorer):                # a procedural checkpoint has no vocabulary: captions -> seeded id rows
        def tokenize(self, captions):
            return [[1] + [3 + (ord(ch) * 7 + j) % 290 for j, ch in enumerate(c)][:30] + [2] for c in captions]

    sc = IdScorer(name, dtype="f32s", batch_size=4)       # batch_size 4 over 5 pairs: a partial micro-batch at the end
    try:
        S = sc.arch.image_size
        for head in ("itm", "itc"):
            out = P.blip2_pseudo_scores(grouped, sc, head)
            assert list(out) == ["(0, 1)", "(0, 2)"]
            assert out["(0, 1)"]["captions"] == ["a red chair", "a wooden table", "a green sofa"] and out["(0, 2)"]["captions"] == ["a lamp", "a tv"]
            # the same pairs through the host path: the reference's slice, BGR -> RGB, Pillow's straight bicubic resize to S x S
            pil, flat = [], []
            for k in grouped:
                for inst in grouped[k]:
                    x1, y1, x2, y2 = P.crop_rect(inst["pred_box"], inst["image"].shape)
                    pil.append(Image.fromarray(np.ascontiguousarray(inst["image"][y1:y2, x1:x2, ::-1])).resize((S, S), Image.BICUBIC))
                    flat.append(inst["caption"])
            ref = sc.score_pairs(pil, flat, head=head).cpu().numpy().astype(np.float64)
            got = np.array(out["(0, 1)"]["scores"] + out["(0, 2)"]["scores"])
            assert np.array_equal(got, ref)                 # device crop = Pillow, bit for bit, and batches do not matter
            if head == "itm":
                assert ((got > 0) & (got < 1)).all()
                pr, lg = sc.score_pairs(pil, flat, head="itm", return_logits=True)
                assert torch.allclose(torch.softmax(lg, 1)[:, 1], pr, atol=1e-6)
        # itc_matrix: all images x all captions; its diagonal = the paired ITC scores
        mat = sc.itc_matrix(pil, flat)
        assert mat.shape == (5, 5) and torch.equal(mat.diagonal(), sc.score_pairs(pil, flat, head="itc"))
        with pytest.raises(ValueError, match="different number"):
            sc.score_pairs(pil, flat[:3])
        # a long caption is truncated at 32 tokens, not refused
        long_ids = [[1] + list(range(3, 60)) + [2]]
        assert sc.tokenizer is None and len(Blip2ItmScorer.tokenize(sc, long_ids)[0]) == 32
    finally:
        sc.close()
    # the command line, with the procedural checkpoint standing in for a directory (id rows come from the patched tokenizer)
    import embodied_captioning_amd.captioner.blip2_itm_scorer as M
    orig = M.Blip2ItmScorer
    M.Blip2ItmScorer = IdScorer
    try:
        outp = tmp_path / "scores.json"
        assert P.main(["--file_path", str(tmp_path), "--output_csv_path", str(outp), "--method", "blip2_itc", "--model", name,
                       "--batch_size", "4"]) == 0
    finally:
        M.Blip2ItmScorer = orig
    res = json.loads(outp.read_text())
    assert list(res) == ["(0, 1)", "(0, 2)"] and set(res["(0, 1)"]) == {"captions", "scores"}
    assert res["(0, 1)"]["scores"] + res["(0, 2)"]["scores"] == got.tolist()


def test_abi_refusals_by_message():
    from embodied_captioning_amd import _native as N
    from embodied_captioning_amd.config import ClipArch
    from embodied_captioning_amd.engine import Blip2ItmEngine, ClipEngine
    from embodied_captioning_amd.weights import procedural_blip2_itm_state_dict, synthetic_frames_u8
    g, arch, frames = _fixture("blip2_itm_tiny")
    lib = N.load_library()
    eng = Blip2ItmEngine(arch, dtype="f32", max_batch=4, max_len=16)
    clip = ClipEngine(ClipArch.tiny(), dtype="f32", max_batch=2)
    try:
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ids = torch.ones((8, 32), dtype=torch.int32, device="cuda")
        lens = torch.full((8,), 3, dtype=torch.int32, device="cuda")
        out = torch.empty((8, 64), device="cuda")
        p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
        # weights not loaded yet
        assert lib.cap_blip2_itc_text_features(eng._h, p(ids), p(lens), 2, 8, p(out), s) != 0 and "not loaded" in N.last_error()
        eng.load_state_dict(procedural_blip2_itm_state_dict(arch, 3))
        assert lib.cap_blip2_itc_text_features(eng._h, p(ids), p(lens), 2, 8, p(out), s) == 0
        assert lib.cap_blip2_itc_text_features(eng._h, p(ids), p(lens), 2, 17, p(out), s) != 0 and "max_len (16)" in N.last_error()
        assert lib.cap_blip2_itc_text_features(eng._h, p(ids), p(lens), 5, 8, p(out), s) != 0 and "max_batch 4" in N.last_error()
        assert lib.cap_blip2_itm_logits(eng._h, p(ids), p(lens), 2, 8, p(out), None, s) != 0 and "no image batch is resident" in N.last_error()
        px = synthetic_frames_u8(5, arch.image_size, arch.image_size, seed=1).cuda()
        assert lib.cap_blip2_itm_encode_images(eng._h, p(px), N.CAP_PIX_U8_NHWC, 5, s) != 0 and "max_batch 4" in N.last_error()
        assert lib.cap_blip2_itm_encode_images(eng._h, p(px), N.CAP_PIX_U8_NHWC, 3, s) == 0
        assert lib.cap_blip2_itm_logits(eng._h, p(ids), p(lens), 2, 8, p(out), None, s) != 0 and "resident image batch has 3" in N.last_error()
        assert lib.cap_blip2_itc_image_features(eng._h, 4, p(out), s) != 0 and "resident image batch has 3" in N.last_error()
        assert lib.cap_blip2_itm_logits(eng._h, p(ids), p(lens), 3, 8, p(out), None, s) == 0        # the probability output may be NULL
        # wrong handle architecture, both ways
        assert lib.cap_blip2_itm_logits(clip._h, p(ids), p(lens), 2, 8, p(out), None, s) != 0 and "CAP_ARCH_BLIP2_ITM" in N.last_error()
        assert lib.cap_clip_embed_text(eng._h, p(ids), p(lens), 2, 8, p(out), s) != 0 and "CLIP" in N.last_error()
        assert lib.cap_encode(eng._h, p(px), N.CAP_PIX_U8_NHWC, 2, p(out), s) != 0 and "image-text scorer" in N.last_error()
        assert lib.cap_blip2_itc_scores(p(out), p(out), 2, 3, 1, p(out), 8, 64, s) != 0 and "paired" in N.last_error()
        torch.cuda.synchronize()
        # geometries the kernels do not take are refused at create
        with pytest.raises(N.CaptionerHipError, match="image-text scorer"):
            Blip2ItmEngine(dataclasses.replace(arch, num_query_tokens=40), dtype="f32", max_batch=2)
        with pytest.raises(N.CaptionerHipError, match="image-text scorer"):
            Blip2ItmEngine(arch, dtype="f32", max_batch=2, max_len=33)
    finally:
        eng.close()
        clip.close()
