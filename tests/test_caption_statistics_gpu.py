"""GPU, end to end: captions -> sentence embeddings -> per-object disagreement / cosine statistics / medoid, on the procedural MiniLM
weights the MiniLM tests use.  Procedural weights have no vocabulary, so the encoder gets a word-hash stand-in for its WordPiece
step; everything after the ids is the product path (cap_embed_text, cap_group_similarity, cap_cosine_matrix)."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _word_ids(self, sentences):
    a = self.arch
    return [[a.cls] + [3 + sum((i + 1) * ord(ch) for i, ch in enumerate(w)) % (a.vocab - 3) for w in s.lower().split()] + [a.sep]
            for s in sentences]


@pytest.fixture(scope="module")
def enc():
    from embodied_captioning_amd.captioner.sentence_encoder import SentenceEncoder
    e = SentenceEncoder("procedural-minilm-tiny:3", dtype="f32", batch_size=4)
    e.tokenize_ids = _word_ids.__get__(e)
    return e


def test_caption_statistics_equal_group_similarity_of_the_encoded_rows(enc):
    from embodied_captioning_amd.distributed import captions_frequency, group_captions, medoid_caption
    from embodied_captioning_amd.similarity import group_similarity
    caps = ["a red chair", "a wooden chair", "a red chair", "a chair by the wall", "a lamp", "a tall lamp", "a white lamp shade",
            "a tall lamp", "a tall lamp"]
    keys = [(0, 1)] * 4 + [(0, 2)] + [(1, 7)] * 4
    freq = captions_frequency(group_captions(keys, caps))
    assert [len(v) for v in freq.values()] == [3, 1, 2]            # three keys: one single caption, two with a repeated caption
    stats = enc.caption_statistics(freq)
    assert list(stats) == list(freq)
    sentences = ["a red chair", "a wooden chair", "a chair by the wall", "a lamp", "a tall lamp", "a white lamp shade"]
    emb = enc.encode(sentences, convert_to_tensor=True)
    st = group_similarity(emb, [0, 3, 4, 6], torch.tensor([2., 1., 1., 1., 3., 1.]))
    off = [0, 3, 4, 6]
    for g, key in enumerate(freq):
        rec = stats[key]
        assert np.float32(rec["disagreement"]) == st.disagreement[g].item()
        assert np.float32(rec["mean"]) == st.pair_mean[g].item()
        assert rec["std"] == float(np.sqrt(st.pair_var[g].cpu().numpy()))
        assert rec["pairs"] == int(st.pairs[g])
        assert rec["row_mean"] == [float(v) for v in st.row_mean[off[g]:off[g + 1]].cpu()]
        assert rec["medoid_caption"] == sentences[int(st.medoid[g])] == medoid_caption(freq[key], rec["row_mean"])
    assert [stats[k]["pairs"] for k in freq] == [6, 0, 6]
    single = stats[(0, 2)]
    assert single["mean"] == 0.0 and single["std"] == 0.0 and single["row_mean"] == [0.0] and single["medoid_caption"] == "a lamp"
    assert abs(single["disagreement"]) < 1e-5                      # one caption agrees with itself
    # against float64 on the same embeddings (unit rows: the encoder normalises)
    e64 = emb.double().cpu().numpy()
    w = np.array([2., 1., 1.])
    s = e64[:3] @ e64[:3].T
    assert abs(stats[(0, 1)]["disagreement"] - (1 - (np.outer(w, w) * s).sum() / 16)) < 1e-5
    assert enc.caption_statistics({}) == {}


def test_similarity_is_the_cosine_matrix_and_pairwise_its_diagonal(enc):
    from embodied_captioning_amd.similarity import cosine_matrix
    a = enc.encode(["a red chair", "a lamp", "a tall lamp"], convert_to_tensor=True)
    b = enc.encode(["a wooden chair", "a white lamp shade", "a chair by the wall"], convert_to_tensor=True)
    m = enc.similarity(a, b)
    assert m.shape == (3, 3) and m.is_cuda and torch.equal(m, cosine_matrix(a, b))
    assert torch.equal(enc.similarity_pairwise(a, b), torch.diagonal(m))
    assert torch.equal(enc.similarity(a[0], b), m[:1])             # a single embedding is one row, as in sentence-transformers
    assert (m.double().cpu() - (a.double() @ b.double().T).cpu()).abs().max() < 1e-5
    from embodied_captioning_amd._native import CaptionerHipError
    with pytest.raises(CaptionerHipError):
        cosine_matrix(a.cpu(), b.cpu())                            # no host path


def test_method_sbert_writes_each_objects_medoid(enc, tmp_path, monkeypatch):
    from embodied_captioning_amd import pseudocaptioner as P
    from embodied_captioning_amd.captioner import sentence_encoder as SE
    from embodied_captioning_amd.pseudolabeler import save_record
    monkeypatch.setattr(SE.SentenceEncoder, "tokenize_ids", _word_ids)
    img = np.zeros((32, 32, 3), dtype=np.uint8)
    recs = [(["a red chair", "a tall lamp"], [5, 9]), (["a wooden chair", "a tall lamp"], [5, 9]),
            (["a red chair", "a white lamp shade"], [5, 9]), (["a chair by the wall", "a lamp"], [5, 9])]
    for i, (caps, objs) in enumerate(recs):
        inst = {"captions": caps, "pred_boxes": [np.array([2, 2, 20, 20], dtype=np.float32)] * len(caps),
                "infos": [{"id_episode": 0, "id_object": o} for o in objs]}
        save_record(str(tmp_path), f"episode_0_step_{i}", inst, img)
    out = tmp_path / "out.json"
    assert P.main(["--file_path", str(tmp_path), "--output_csv_path", str(out), "--method", "sbert", "--model",
                   "procedural-minilm-tiny:3"]) == 0
    got = json.loads(out.read_text())
    assert set(got) == {"(0, 5)", "(0, 9)"}
    freq = {(0, 5): [[2, "a red chair"], [1, "a wooden chair"], [1, "a chair by the wall"]],
            (0, 9): [[2, "a tall lamp"], [1, "a white lamp shade"], [1, "a lamp"]]}
    stats = enc.caption_statistics(freq)
    for key, rec in stats.items():
        g = got[str(key)]
        assert g["pseudocaption"][1] == rec["medoid_caption"]
        assert g["pseudocaption"] == g["captions_list"][0]
        assert sorted(c for _, c in g["captions_list"]) == sorted(c for _, c in freq[key])
        assert [s for s, _ in g["captions_list"]] == sorted(rec["row_mean"], reverse=True)
    assert "sbert" not in P.REFUSED_METHODS and P.REFUSED_METHODS == ("llm", "mobileclip", "openclip")
