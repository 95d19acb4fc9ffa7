"""CPU only, run once: HF's own beam search on the scripted model of tests/_beam_script.py.

    python -m oracle.beam_scripted_ref          # writes tests/golden/beam_scripted.npz

The scripted model is wrapped in the smallest module transformers' `generate` accepts (a PreTrainedModel with a GenerationMixin
whose forward returns the scripted fp32 logits of every row's prefix, no cache), and `generate(num_beams=K, length_penalty=lp,
max_length=L, early_stopping=False)` of the installed transformers 5.x runs its `_beam_search` unchanged.  Recorded per HF-v5 case
without constructed ties: the case's parameters, HF's sequences (padded to max_len with the case's fill value) and
sequences_scores.  The legacy scorer does not exist in 5.x (tests/_beam_ref.py is its only reference) and torch.topk does not
specify an order among equal values, so the legacy and the exact-tie cases have no record; nor have the K = 1 cases, because
`generate(num_beams=1)` runs HF's greedy loop, not a one-beam beam search."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from _beam_script import CASES, PAD, V5, logits_row  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "beam_scripted.npz")


def _model(case):
    import transformers
    from transformers.modeling_outputs import CausalLMOutput

    class ScriptedConfig(transformers.PretrainedConfig):
        model_type = "scripted_beam"

    class Scripted(transformers.PreTrainedModel, transformers.GenerationMixin):
        config_class = ScriptedConfig
        main_input_name = "input_ids"

        def __init__(self, config):
            super().__init__(config)
            self.anchor = torch.nn.Parameter(torch.zeros(1))        # gives the module a device and a dtype

        def forward(self, input_ids=None, **kwargs):
            rows = input_ids.shape[0]
            assert rows == case.B * case.K
            out = np.stack([logits_row(case, r // case.K, input_ids[r].tolist()) for r in range(rows)])
            return CausalLMOutput(logits=torch.from_numpy(out)[:, None, :])

        def prepare_inputs_for_generation(self, input_ids, **kwargs):
            return {"input_ids": input_ids}

    cfg = ScriptedConfig(vocab_size=case.V, bos_token_id=case.bos, eos_token_id=case.eos, pad_token_id=PAD)
    return Scripted(cfg).eval()


def hf_generate(case):
    """-> (sequences int32 [B, max_len] padded with the case's fill, sequences_scores fp32 [B])."""
    model = _model(case)
    ids = torch.full((case.B, 1), case.bos, dtype=torch.long)
    with torch.no_grad():
        out = model.generate(ids, num_beams=case.K, length_penalty=float(case.lp), max_length=case.max_len, early_stopping=False,
                             do_sample=False, use_cache=False, num_return_sequences=1, return_dict_in_generate=True,
                             output_scores=True, eos_token_id=case.eos, pad_token_id=PAD, bos_token_id=case.bos)
    seq = np.full((case.B, case.max_len), case.fill, dtype=np.int32)
    got = out.sequences.numpy()
    seq[:, : got.shape[1]] = got
    return seq, out.sequences_scores.numpy().astype(np.float32)


def main():
    import transformers
    rec = {"transformers_version": np.array(transformers.__version__)}
    names = []
    for case in CASES:
        if case.mode != V5 or case.tie or case.K == 1:
            continue
        seq, sc = hf_generate(case)
        names.append(case.name)
        rec[case.name + "/sequences"] = seq
        rec[case.name + "/scores"] = sc
        rec[case.name + "/params"] = np.array([case.seed, case.B, case.K, case.V, case.max_len, case.eos, case.bos], dtype=np.int64)
        rec[case.name + "/lp"] = np.array(case.lp, dtype=np.float64)
        print(case.name, seq.tolist(), sc.tolist())
    rec["names"] = np.array(names)
    np.savez_compressed(OUT, **rec)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
