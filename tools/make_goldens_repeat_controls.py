#!/usr/bin/env python
"""Golden vectors for `repetition_penalty` / `no_repeat_ngram_size` from the REAL HF implementation (transformers 5.x, CPU fp32):
`generate(..., repetition_penalty=, no_repeat_ngram_size=)` of `BlipForConditionalGeneration` and `Blip2ForConditionalGeneration` on
the fixture-size architectures with procedural weights.  Run in the build container only; data only:

    python tools/make_goldens_repeat_controls.py   # writes tests/golden/blip_tiny_repeat_controls.npz and blip2_tiny_repeat_controls.npz

Per file, per case the ids, lengths, `sequences_scores` (beams) and the per-step top-1 / top-2 margins of HF's PROCESSED scores
(`output_scores`; beams: the smallest over an image's K rows) -
  penalty         generate(pixel_values, repetition_penalty=1.5)
  ngram           generate(pixel_values, no_repeat_ngram_size=n)                 n = 1 for BLIP (whose captions repeat few bigrams), 2 for BLIP-2
  all             generate(pixel_values, repetition_penalty=1.5, no_repeat_ngram_size=n, bad_words_ids=ban)
  beams3          generate(pixel_values, num_beams=3, repetition_penalty=1.5, no_repeat_ngram_size=n)
  prompted (BLIP) generate(pixel_values, input_ids=[bos, x, y, x, sep], repetition_penalty=1.5, no_repeat_ngram_size=2): y is the token
                  most images emit first behind [bos, x] unconstrained, so the bigram `x y` of the PROMPT bans y at the first step
The ban list of `all` is taken from HF's run under the two controls alone (tools/make_goldens_bad_words.py::ban_list).
A test compares a row only when every step's margin in HF's run is at least the logit bar of its mode.  So that neither condition can
hide a failure, the seed is searched (0, 1, ...) for the first one with, in every case, at most 1 row in 8 below the f32s bar (1e-3)
AND at least 2 rows in 8 that differ from HF's unconstrained run of the same call; both are asserted on what is written.
"""
import dataclasses
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from embodied_captioning_amd.config import Blip2Arch, BlipArch                                          # noqa: E402
from embodied_captioning_amd.weights import procedural_blip2_state_dict, procedural_blip_state_dict, synthetic_pixels  # noqa: E402
import make_goldens                                                                                      # noqa: E402
import make_goldens_blip2                                                                                # noqa: E402
from make_goldens_bad_words import BAR, BATCH, ban_list, case, rows_of                                   # noqa: E402

PENALTY = 1.5
MIN_CHANGED = 2
X = 31                # BLIP: the prompt is [bos, X, y, X]


def changed_rows(a, b):
    """Rows whose returned sequences differ (either may be the longer tensor: HF stops a batch at its longest caption)."""
    n = max(a.shape[1], b.shape[1])
    pa, pb = torch.zeros((a.shape[0], n), dtype=torch.long), torch.zeros((b.shape[0], n), dtype=torch.long)
    pa[:, : a.shape[1]], pb[:, : b.shape[1]] = a, b
    return int((pa != pb).any(dim=1).sum())


def blip(seed):
    a = BlipArch.tiny()
    L, boost, n1 = 16, 1.0, 1
    sd = procedural_blip_state_dict(a, seed, eos_boost=boost)
    m = make_goldens.build_hf(a, sd)
    px = synthetic_pixels(BATCH, a.image_size, seed=seed)
    special = {a.bos, a.eos, a.pad}
    kw = dict(pixel_values=px, max_length=L, do_sample=False, return_dict_in_generate=True, output_scores=True)
    with torch.no_grad():
        free = m.generate(num_beams=1, **kw)
        free3 = m.generate(num_beams=3, **kw)
        short = m.generate(num_beams=1, input_ids=torch.tensor([[a.bos, X, a.eos]] * BATCH, dtype=torch.long), **kw)
        first = short.sequences[:, 2].tolist()
        y = max(set(first), key=first.count)
        if y in special or y == X:
            return None
        prompt = [a.bos, X, y, X]
        inp = torch.tensor([prompt + [a.eos]] * BATCH, dtype=torch.long)
        pfree = m.generate(num_beams=1, input_ids=inp, **kw)
        pen = m.generate(num_beams=1, repetition_penalty=PENALTY, **kw)
        ng = m.generate(num_beams=1, no_repeat_ngram_size=n1, **kw)
        both = m.generate(num_beams=1, repetition_penalty=PENALTY, no_repeat_ngram_size=n1, **kw)
        ban = ban_list(rows_of(both.sequences[:, 1:], a.eos), special)
        if ban is None:
            return None
        al = m.generate(num_beams=1, repetition_penalty=PENALTY, no_repeat_ngram_size=n1, bad_words_ids=ban, **kw)
        b3 = m.generate(num_beams=3, repetition_penalty=PENALTY, no_repeat_ngram_size=n1, **kw)
        pr = m.generate(num_beams=1, input_ids=inp, repetition_penalty=PENALTY, no_repeat_ngram_size=2, **kw)
    out, low, changed = {}, {}, {}
    P = len(prompt)
    for key, o, ref, first_col, K in (("penalty", pen, free, 1, 1), ("ngram", ng, free, 1, 1), ("all", al, free, 1, 1),
                                      ("beams3", b3, free3, 1, 3), ("prompted", pr, pfree, P, 1)):
        r, low[key] = case(o, first_col, o.sequences[:, first_col:], L - first_col, a.pad, a.eos, K, key)
        out.update(r)
        changed[key] = changed_rows(o.sequences, ref.sequences)
    assert not (pr.sequences[:, P] == y).any()
    out["ban"] = np.array(json.dumps(ban))
    out["prompt_ids"] = np.asarray(prompt, dtype=np.int32)
    out["meta"] = np.array(json.dumps(dict(seed=seed, eos_boost=boost, batch=BATCH, max_length=L, bar=BAR, rows_below_bar=low,
                                           rows_changed=changed, penalty=PENALTY, ngram=n1, ngram_prompted=2, arch=a.__dict__,
                                           transformers=__import__("transformers").__version__)))
    return out, low, changed


def blip2(seed):
    a = Blip2Arch.tiny()
    n, boost, n2 = a.max_new_tokens, 0.3, 2
    sd = procedural_blip2_state_dict(a, seed, eos_boost=boost)
    m = make_goldens_blip2.build_hf(a, sd)
    px = synthetic_pixels(BATCH, a.image_size, seed=seed)
    special = {a.bos, a.eos, a.pad, a.image_token}
    kw = dict(pixel_values=px, max_new_tokens=n, do_sample=False, return_dict_in_generate=True, output_scores=True)
    cut = a.num_query_tokens + 1                                       # HF returns image placeholders + BOS + new tokens
    fill = a.pad if a.pad else a.eos
    with torch.no_grad():
        free = m.generate(num_beams=1, **kw)
        free3 = m.generate(num_beams=3, **kw)
        pen = m.generate(num_beams=1, repetition_penalty=PENALTY, **kw)
        ng = m.generate(num_beams=1, no_repeat_ngram_size=n2, **kw)
        both = m.generate(num_beams=1, repetition_penalty=PENALTY, no_repeat_ngram_size=n2, **kw)
        ban = ban_list(rows_of(both.sequences[:, cut:], a.eos), special)
        if ban is None:
            return None
        al = m.generate(num_beams=1, repetition_penalty=PENALTY, no_repeat_ngram_size=n2, bad_words_ids=ban, **kw)
        b3 = m.generate(num_beams=3, repetition_penalty=PENALTY, no_repeat_ngram_size=n2, **kw)
    out, low, changed = {}, {}, {}
    for key, o, ref, K in (("penalty", pen, free, 1), ("ngram", ng, free, 1), ("all", al, free, 1), ("beams3", b3, free3, 3)):
        r, low[key] = case(o, 0, o.sequences[:, cut:], n, fill, a.eos, K, key)
        out.update(r)
        changed[key] = changed_rows(o.sequences, ref.sequences)
    out["ban"] = np.array(json.dumps(ban))
    out["meta"] = np.array(json.dumps(dict(seed=seed, eos_boost=boost, batch=BATCH, bar=BAR, rows_below_bar=low, rows_changed=changed,
                                           penalty=PENALTY, ngram=n2, arch=dataclasses.asdict(a),
                                           transformers=__import__("transformers").__version__)))
    return out, low, changed


def main():
    torch.manual_seed(0)
    gold = os.path.join(ROOT, "tests", "golden")
    for name, make in (("blip_tiny_repeat_controls", blip), ("blip2_tiny_repeat_controls", blip2)):
        for seed in range(64):
            r = make(seed)
            if r is None:
                print(name, "seed", seed, "no prompt token / ban list to take")
                continue
            out, low, changed = r
            print(name, "seed", seed, "rows below the bar", low, "rows changed", changed)
            if max(low.values()) * 8 <= BATCH and min(changed.values()) >= MIN_CHANGED:
                break
        else:
            raise SystemExit(f"{name}: no seed keeps all but 1 row in 8 above the bar and changes {MIN_CHANGED} rows in every case")
        assert max(low.values()) * 8 <= BATCH and min(changed.values()) >= MIN_CHANGED
        np.savez_compressed(os.path.join(gold, name + ".npz"), **out)
        print(name, "written: seed", seed, {k: v.tolist() for k, v in out.items() if k.endswith("_ids")})
    print("done")


if __name__ == "__main__":
    main()
