"""Teacher forcing on the CPU oracle: what `CaptionerEngine.score` must return, restated with oracle.blip_ref (test infrastructure).

BLIP: the image side once per image (`encode_image`, `cross_kv` with the captions of an image repeating its rows), then
`decoder_step` fed the GIVEN token of every position.  float32 is the oracle as it stands; float64 is the same code on a state
dict and pixels cast to float64 (nothing in these functions casts back), the reference the GPU tests' bars are taken against.
Every reduction of a logits row (log-softmax at the target, log max softmax, arg-max, top-2 margin) is made in float64."""
import numpy as np
import torch

from oracle import blip_ref as R


def reduce_rows(logits, targets):
    """logits [n, V] (any float type), targets int [n] -> float64 (target log-prob, log max softmax), int64 arg-max, float64 top-2
    logit margin - each [n]."""
    x = logits.double()
    lp = torch.log_softmax(x, dim=-1)
    top2 = torch.topk(x, k=2, dim=-1)
    return (lp.gather(1, targets.long()[:, None])[:, 0], lp.max(dim=-1).values, top2.indices[:, 0], top2.values[:, 0] - top2.values[:, 1])


@torch.no_grad()
def blip_score(sd, arch, pixels, ids, lens, captions_per_image=1, dtype=torch.float64):
    """ids int [N, L], lens int [N] (0 = absent slot), N = B * captions_per_image -> dict of numpy arrays [N, L - 1]:
    token_logprobs, top_logprobs (float64, 0 behind a caption's end), top_ids (int64, 0 behind), margin (float64, +inf behind:
    no constraint), and live (bool)."""
    ids = torch.as_tensor(np.asarray(ids)).long()
    lens = torch.as_tensor(np.asarray(lens)).long()
    N, L = ids.shape
    sdd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    emb = R.encode_image(sdd, arch, pixels.to(dtype))
    assert emb.shape[0] * captions_per_image == N
    state = R.DecoderState(arch.t_layers)
    R.cross_kv(sdd, arch, emb, state, repeat=captions_per_image)
    tlp = np.zeros((N, L - 1))
    top = np.zeros((N, L - 1))
    tid = np.zeros((N, L - 1), dtype=np.int64)
    margin = np.full((N, L - 1), np.inf)
    live = np.zeros((N, L - 1), dtype=bool)
    for j in range(L - 1):
        logits = R.decoder_step(sdd, arch, ids[:, j], state)
        a, b, c, d = reduce_rows(logits, ids[:, j + 1])
        on = (j < lens - 1).numpy()
        live[:, j] = on
        tlp[on, j], top[on, j], tid[on, j], margin[on, j] = a.numpy()[on], b.numpy()[on], c.numpy()[on], d.numpy()[on]
    return {"token_logprobs": tlp, "top_logprobs": top, "top_ids": tid, "margin": margin, "live": live}


def random_captions(arch, n, L, lens, seed, special=()):
    """n rows of L ids: BOS, then random ids that are none of BOS / EOS / pad / `special`; a row of full length L ends as drawn, a
    shorter one likewise (the caller places EOS where it wants the end scored).  Columns from lens[n] on hold other random ids."""
    g = np.random.default_rng(seed)
    ok = np.array([i for i in range(arch.vocab) if i not in {arch.bos, arch.eos, arch.pad, *special}])
    ids = ok[g.integers(0, len(ok), size=(n, L))].astype(np.int32)
    ids[:, 0] = arch.bos
    return ids


@torch.no_grad()
def blip2_score(sd, arch, pixels, ids, lens, captions_per_image=1, dtype=torch.float64):
    """BLIP-2: `language_inputs` and the prompt pass once per image (`opt_forward` over the projected queries + BOS), its caches and
    BOS logits repeated for the image's captions, then `opt_forward` fed the GIVEN token of every further position.  float64 through
    tests/_blip2_beam_ref.py::in_format (the oracle's `.float()` calls then keep float64).  Same outputs as `blip_score`."""
    from _blip2_beam_ref import LM, in_format
    from oracle import blip2_ref as R2
    ids = torch.as_tensor(np.asarray(ids)).long()
    lens = torch.as_tensor(np.asarray(lens)).long()
    N, L = ids.shape
    C = captions_per_image
    sdd = in_format(sd, np.float64 if dtype == torch.float64 else np.float32)
    _, _, proj = R2.language_inputs(sdd, arch, pixels.to(dtype))
    B = proj.shape[0]
    assert B * C == N
    tok = sdd[LM + "embed_tokens.weight"].float()
    st = R2.OptState(arch.t_layers)
    logits = R2.opt_forward(sdd, arch, torch.cat([proj, tok[torch.full((B, 1), arch.bos)]], 1), st).repeat_interleave(C, 0)
    st.k = [k.repeat_interleave(C, 0) for k in st.k]
    st.v = [v.repeat_interleave(C, 0) for v in st.v]
    tlp = np.zeros((N, L - 1))
    top = np.zeros((N, L - 1))
    tid = np.zeros((N, L - 1), dtype=np.int64)
    margin = np.full((N, L - 1), np.inf)
    live = np.zeros((N, L - 1), dtype=bool)
    for j in range(L - 1):
        if j > 0:
            logits = R2.opt_forward(sdd, arch, tok[ids[:, j]][:, None], st)
        a, b, c, d = reduce_rows(logits, ids[:, j + 1])
        on = (j < lens - 1).numpy()
        live[:, j] = on
        tlp[on, j], top[on, j], tid[on, j], margin[on, j] = a.numpy()[on], b.numpy()[on], c.numpy()[on], d.numpy()[on]
    return {"token_logprobs": tlp, "top_logprobs": top, "top_ids": tid, "margin": margin, "live": live}
