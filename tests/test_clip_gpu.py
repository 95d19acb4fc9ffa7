"""GPU: the CLIP scorer (CAP_ARCH_CLIP) against the float64 HF `CLIPModel` goldens (tools/make_goldens_clip.py), its batch
invariance, the crop path with HF's shortest-edge geometry, the pseudo-caption driver and the ABI's refusals."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# tolerances per mode: embeddings (max abs; bf16: 1 - cosine), logits_per_image (max abs).  Measured on the MI355X over both
# fixtures (profiles/clip_gpu_tolerances.txt): embeddings f32 2.7e-7, f32s 1.5e-7, bf16 3.0e-5 (1 - cos); logits f32 3.8e-6,
# f32s 2.2e-6, bf16 0.023 - the bars are about 8x those
TOL = {"f32": (2e-6, 2e-5), "f32s": (2e-6, 2e-5), "bf16": (0.9997, 0.2)}


def _fixture(name):
    from embodied_captioning_amd.config import ClipArch
    from embodied_captioning_amd.weights import procedural_clip_state_dict, synthetic_frames_u8
    g = dict(np.load(os.path.join(GOLDEN, f"{name}.npz")))
    arch = ClipArch.tiny() if name == "clip_tiny" else ClipArch()
    if "frames" not in g:
        g["frames"] = synthetic_frames_u8(int(g["n_images"]), arch.image_size, arch.image_size, seed=int(g["frame_seed"])).numpy()
    return g, arch, procedural_clip_state_dict(arch, int(g["seed"]))


_ENGINES = {}


def _engine(name, dtype, max_batch=64):
    key = (name, dtype, max_batch)
    if key not in _ENGINES:
        from embodied_captioning_amd.engine import ClipEngine
        g, arch, sd = _fixture(name)
        eng = ClipEngine(arch, dtype=dtype, max_batch=max_batch)
        eng.load_state_dict(sd)
        _ENGINES[key] = eng
    return _ENGINES[key]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()


def _check_embeds(out, ref, dtype):
    tol = TOL[dtype][0]
    if dtype == "bf16":
        cos = (out * ref).sum(1)
        assert cos.min() >= tol, cos.min()
        return float(1 - cos.min())
    err = float(np.abs(out - ref).max())
    assert err < tol, err
    return err


@pytest.mark.parametrize("name", ["clip_tiny", "clip_b32"])
@pytest.mark.parametrize("dtype", ["f32", "f32s", "bf16"])
def test_embeddings_and_logits_match_hf_golden(name, dtype):
    g, arch, _ = _fixture(name)
    eng = _engine(name, dtype)
    img = eng.embed_images(torch.from_numpy(g["frames"])).cpu().numpy()
    img_f = eng.embed_images(torch.from_numpy(normalise(g["frames"]))).cpu().numpy()     # the fp32 NCHW input form
    txt = eng.embed_text(torch.from_numpy(g["ids"]), torch.from_numpy(g["lens"])).cpu().numpy()
    e_img = _check_embeds(img, g["image_embeds"], dtype)
    _check_embeds(img_f, g["image_embeds"], dtype)
    e_txt = _check_embeds(txt, g["text_embeds"], dtype)
    assert np.allclose(np.linalg.norm(img, axis=1), 1.0, atol=1e-5) and np.allclose(np.linalg.norm(txt, axis=1), 1.0, atol=1e-5)
    assert abs(eng.logit_scale - float(g["logit_scale"])) < 1e-6
    lpi = eng.logits(torch.from_numpy(img), torch.from_numpy(txt), paired=False).cpu().numpy()
    e_l = float(np.abs(lpi - g["logits_per_image"]).max())
    print(f"\n{name} {dtype}: image {e_img:.3g} text {e_txt:.3g} logits {e_l:.3g}")
    assert e_l < TOL[dtype][1], e_l
    # paired form = the diagonal pairs of the full matrix, same bits (one kernel, same sum order)
    n = min(img.shape[0], txt.shape[0])
    pa = eng.logits(torch.from_numpy(img[:n]), torch.from_numpy(txt[:n]), paired=True).cpu().numpy()
    assert np.array_equal(pa, lpi[np.arange(n), np.arange(n)])
    # HF's top-1 per synthetic group, wherever its margin exceeds twice the mode's logit tolerance
    for gi, gt, rank, margin in zip(g["group_images"], g["group_captions"], g["group_rank"], g["group_margin"]):
        if margin > 2 * TOL[dtype][1]:
            sc = lpi[gi, gt]
            assert int(np.argsort(-sc, kind="stable")[0]) == int(rank[0])


def normalise(frames):
    from embodied_captioning_amd.engine import OPENAI_CLIP_MEAN, OPENAI_CLIP_STD
    x = frames.astype(np.float32) / np.float32(255.0)
    x = (x - np.asarray(OPENAI_CLIP_MEAN, np.float32)) / np.asarray(OPENAI_CLIP_STD, np.float32)
    return np.ascontiguousarray(x.transpose(0, 3, 1, 2))


@pytest.mark.parametrize("dtype", ["f32s", "bf16", "f32"])
def test_batch_invariance_same_bits(dtype):
    """An image alone, inside a batch of 256 and at the end of a partial micro-batch; a caption with other ids after lens[b]
    and alone against a ragged batch: torch.equal."""
    from embodied_captioning_amd.weights import synthetic_frames_u8
    g, arch, _ = _fixture("clip_tiny")
    eng = _engine("clip_tiny", dtype, max_batch=256)
    frames = synthetic_frames_u8(256, arch.image_size, arch.image_size, seed=99)
    full = eng.embed_images(frames)
    for i in (0, 77, 255):
        assert torch.equal(eng.embed_images(frames[i:i + 1])[0], full[i])
    part = eng.embed_images(frames[200:237])
    assert torch.equal(part, full[200:237])
    ids, lens = torch.from_numpy(g["ids"]), torch.from_numpy(g["lens"])
    txt = eng.embed_text(ids, lens)
    noisy = ids.clone()
    for b in range(ids.shape[0]):
        n = int(lens[b])
        noisy[b, n:] = torch.randint(0, arch.vocab, (ids.shape[1] - n,), generator=torch.Generator().manual_seed(b))
    assert torch.equal(eng.embed_text(noisy, lens), txt)
    for b in range(ids.shape[0]):
        n = int(lens[b])
        assert torch.equal(eng.embed_text(ids[b:b + 1, :n], lens[b:b + 1])[0], txt[b])


@pytest.mark.parametrize("dtype", ["f32s", "bf16", "f32"])
def test_batch_invariance_b32_at_the_scorer_batch(dtype):
    """ViT-B/32 at the scorer's default micro-batch of 256: there the towers' GEMMs (fc1 with its quick-GELU epilogue included)
    run on the 256 x 256 kernels - gemm_pp.hip for bf16 / f32s, interior and edge tiles - while one image or caption alone runs on
    the 64 x 64 tile.  Same bits either way."""
    from embodied_captioning_amd.engine import ClipEngine
    from embodied_captioning_amd.weights import synthetic_frames_u8
    g, arch, sd = _fixture("clip_b32")
    eng = ClipEngine(arch, dtype=dtype, max_batch=256)
    eng.load_state_dict(sd)
    frames = synthetic_frames_u8(256, arch.image_size, arch.image_size, seed=7)
    full = eng.embed_images(frames)
    for i in (0, 131, 255):
        assert torch.equal(eng.embed_images(frames[i:i + 1])[0], full[i]), i
    rng = np.random.default_rng(5)
    lens = rng.integers(3, 41, size=256)
    lens[0] = 40                                           # 256 x 40 rows: fc1 is 10240 x 2048, past the 256 x 256 threshold
    ids = np.full((256, 40), arch.eos_token_id, dtype=np.int64)
    for b in range(256):
        ids[b, 0] = arch.bos_token_id
        ids[b, 1:lens[b] - 1] = rng.integers(1, 49000, size=lens[b] - 2)
    ids, lens = torch.from_numpy(ids), torch.from_numpy(lens.astype(np.int32))
    txt = eng.embed_text(ids, lens)
    for b in (0, 100, 255):
        n = int(lens[b])
        assert torch.equal(eng.embed_text(ids[b:b + 1, :n], lens[b:b + 1])[0], txt[b]), b
    eng.close()


def test_abi_errors():
    from embodied_captioning_amd import _native as N
    from embodied_captioning_amd.config import BlipArch
    from embodied_captioning_amd.engine import CaptionerEngine, ClipEngine
    g, arch, sd = _fixture("clip_tiny")
    eng = _engine("clip_tiny", "f32s", max_batch=64)
    lib = eng.lib
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    frames = torch.from_numpy(g["frames"]).cuda()
    big = frames[:1].repeat(65, 1, 1, 1).contiguous()
    with pytest.raises(ValueError, match="outside 1..64"):
        eng.embed_images(big)
    out = torch.empty((65, arch.projection_dim), device="cuda")
    assert lib.cap_clip_embed_images(eng._h, C.c_void_p(big.data_ptr()), N.CAP_PIX_U8_NHWC, 65, C.c_void_p(out.data_ptr()), s) != 0
    assert "capacity" in N.last_error()
    ids, lens = torch.from_numpy(g["ids"]), torch.from_numpy(g["lens"])
    with pytest.raises(ValueError, match="lens"):
        eng.embed_text(ids, lens + ids.shape[1])
    with pytest.raises(ValueError, match="lens"):
        eng.embed_text(ids, lens * 0)
    # cap_generate / cap_encode on a CLIP handle
    oid = torch.empty((1, 8), dtype=torch.int32, device="cuda")
    assert lib.cap_generate(eng._h, C.c_void_p(frames.data_ptr()), N.CAP_PIX_U8_NHWC, 1, 1, 8, C.c_float(1.0), C.c_void_p(oid.data_ptr()),
                            None, None, None, s) != 0
    assert "CLIP scorer" in N.last_error()
    assert lib.cap_encode(eng._h, C.c_void_p(frames.data_ptr()), N.CAP_PIX_U8_NHWC, 1, C.c_void_p(out.data_ptr()), s) != 0
    assert "CLIP scorer" in N.last_error()
    # missing weights: cap_finalize_weights counts them, the entry points refuse
    part = ClipEngine(arch, dtype="f32s", max_batch=4)
    part.load_state_dict({k: v for k, v in sd.items() if "text_model" not in k}, strict=False)
    n_text = sum(1 for k in sd if "text_model" in k)
    assert lib.cap_finalize_weights(part._h) == n_text
    assert lib.cap_clip_embed_images(part._h, C.c_void_p(frames.data_ptr()), N.CAP_PIX_U8_NHWC, 1, C.c_void_p(out.data_ptr()), s) != 0
    assert "not loaded" in N.last_error()
    part.close()
    # cap_clip_* on a BLIP handle
    blip = CaptionerEngine(BlipArch.tiny(), dtype="f32", max_batch=2, max_len=8)
    assert lib.cap_clip_embed_images(blip._h, C.c_void_p(frames.data_ptr()), N.CAP_PIX_U8_NHWC, 1, C.c_void_p(out.data_ptr()), s) != 0
    assert "not a CLIP scorer" in N.last_error()
    idd, ld = ids.cuda().int().contiguous(), lens.cuda().int().contiguous()
    assert lib.cap_clip_embed_text(blip._h, C.c_void_p(idd.data_ptr()), C.c_void_p(ld.data_ptr()), 1, ids.shape[1], C.c_void_p(out.data_ptr()), s) != 0
    assert "not a CLIP scorer" in N.last_error()
    blip.close()


def test_shared_weights_engine_gives_same_bits():
    from embodied_captioning_amd.engine import ClipEngine
    g, arch, _ = _fixture("clip_tiny")
    eng = _engine("clip_tiny", "f32s")
    other = ClipEngine(arch, dtype="f32s", max_batch=8, share_weights_with=eng)
    fr = torch.from_numpy(g["frames"])
    assert torch.equal(other.embed_images(fr), eng.embed_images(fr))
    assert other.device_bytes < eng.device_bytes
    other.close()


def test_device_crop_hf_geometry_is_byte_identical_with_pillow():
    """Box crops resized on the device with HF's shortest-edge geometry = Pillow's crop -> resize(shortest edge, BICUBIC) ->
    centre crop, byte for byte."""
    from PIL import Image
    from embodied_captioning_amd.preprocess import crop_resize_u8_frames, hf_shortest_edge_geometry
    rng = np.random.default_rng(1)
    frames = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in ((480, 640), (721, 1280), (97, 53))]
    rects = [[(10, 20, 300, 200), (0, 0, 37, 91), (600, 400, 640, 480)], [(1000, 5, 1280, 721), (3, 3, 227, 228)], [(0, 0, 53, 97)]]
    S = 224
    out = crop_resize_u8_frames(frames, rects, S, bgr=True, center_crop=True, geometry="hf").cpu().numpy()
    k = 0
    for f, rs in zip(frames, rects):
        pil = Image.fromarray(np.ascontiguousarray(f[..., ::-1]))
        for r in rs:
            c = pil.crop(r)
            nw, nh, left, top = hf_shortest_edge_geometry(c.size[0], c.size[1], S)
            ref = np.asarray(c.resize((nw, nh), Image.BICUBIC))[top:top + S, left:left + S]
            assert np.array_equal(out[k], ref), (r, np.abs(out[k].astype(int) - ref).max())
            k += 1


def test_pseudo_captions_from_frames_match_host_pil_path():
    """clip_pseudo_captions (device crop + resize, batched towers) against a host path: the reference's numpy slice + BGR->RGB,
    then Pillow's resize (shortest edge, BICUBIC) + centre crop on the host, scored by the same engine - same scores, same
    order."""
    from PIL import Image
    from embodied_captioning_amd.preprocess import hf_shortest_edge_geometry
    from embodied_captioning_amd.captioner.clip_scorer import ClipScorer
    from embodied_captioning_amd.pseudocaptioner import clip_pseudo_captions, crop_rect
    sc = ClipScorer("procedural-clip-tiny:3", dtype="f32s", batch_size=4)      # micro-batches of 4: several per call
    rng = np.random.default_rng(2)
    frames = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in ((480, 640), (720, 1280), (1280, 1280))]
    a = sc.arch
    grouped = {}
    for k in range(4):
        lst = []
        for j in range(3 + k % 2):
            f = frames[(k + j) % 3]
            x1 = float(rng.integers(0, f.shape[1] - 40)); y1 = float(rng.integers(0, f.shape[0] - 40))
            box = np.array([x1, y1, x1 + rng.integers(20, 400), y1 + rng.integers(20, 400)], np.float32)
            n = int(rng.integers(3, a.max_pos))
            ids = [a.bos_token_id] + rng.integers(1, 290, size=n - 2).tolist() + [a.eos_token_id]
            lst.append({"image": f, "pred_box": box, "caption": ids})
        grouped[(0, k)] = lst
    out = clip_pseudo_captions(grouped, sc)
    crops, caps = [], []
    for lst in grouped.values():
        for inst in lst:
            x1, y1, x2, y2 = crop_rect(inst["pred_box"], inst["image"].shape)
            c = Image.fromarray(np.ascontiguousarray(inst["image"][y1:y2, x1:x2, ::-1]))
            nw, nh, left, top = hf_shortest_edge_geometry(c.size[0], c.size[1], a.image_size)
            crops.append(np.asarray(c.resize((nw, nh), Image.BICUBIC))[top:top + a.image_size, left:left + a.image_size])
            caps.append(inst["caption"])
    host = sc.score_pairs(torch.from_numpy(np.stack(crops)), caps).cpu().numpy()      # [n, S, S, 3]: no further resize
    i = 0
    for key, lst in grouped.items():
        want = sorted([[float(host[i + j]), inst["caption"]] for j, inst in enumerate(lst)], key=lambda x: x[0], reverse=True)
        i += len(lst)
        assert out[str(key)]["captions_list"] == want
        assert out[str(key)]["pseudocaption"] == want[0]
    sc.close()


@pytest.mark.parametrize("N", [33, 50, 64])
def test_vit_attention_two_key_block_mfma_kernel(N):
    """bf16 attention at two key blocks (CLIP ViT-B/32: 50 tokens) on the MFMA kernel: against float64 and against the scalar
    kernel on the same bf16 inputs."""
    from embodied_captioning_amd import _native as N_
    lib = N_.load_library()
    B, H = 3, 12
    g = torch.Generator().manual_seed(N)
    qkv = (torch.randn(B * N, 3 * H * 64, generator=g) * 1.5).to(torch.bfloat16)
    qd = qkv.cuda()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    mf = torch.full((B * N, H * 64), float("nan"), dtype=torch.bfloat16, device="cuda")
    sc = torch.full_like(mf, float("nan"))
    assert lib.cap_op_vit_attention(1, C.c_void_p(qd.data_ptr()), C.c_void_p(mf.data_ptr()), B, N, H, 2, s) == 0, N_.last_error()
    assert lib.cap_op_vit_attention(1, C.c_void_p(qd.data_ptr()), C.c_void_p(sc.data_ptr()), B, N, H, 1, s) == 0, N_.last_error()
    torch.cuda.synchronize()
    x = qkv.double().view(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    ref = (torch.softmax((x[0] @ x[1].transpose(-1, -2)) * 0.125, -1) @ x[2]).permute(0, 2, 1, 3).reshape(B * N, H * 64)
    assert (mf.double().cpu() - ref).abs().max().item() < 3e-2
    assert (mf.float() - sc.float()).abs().max().item() < 2e-2
