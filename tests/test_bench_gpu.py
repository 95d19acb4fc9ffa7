"""GPU: bench.py's plain run (the headline figure only) and --dump-outputs, in a child process as the driver runs it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from _util import load_golden

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FULL_ONLY = ("pool_uncoalesced", "strong_scaling", "power", "single_stream", "roofline", "kernels", "decode", "pass_rows_profile",
             "encoder_only", "latency", "parity", "bf16", "f32_exact", "f32s_fp32kv", "cpu_baseline", "summary")


def test_plain_bench_run_is_the_headline_and_dumps_the_golden_captions(tmp_path):
    """`bench.py --gpus 1 --steps 2 --warmup 1 --dump-outputs DIR`: the line has the headline keys and none of the --full legs;
    the dumped captions of the last timed step are the 256 rows of the HF greedy golden (same frames and weights; the default
    split mode is token-identical to it)."""
    d = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 2 and line["value"] > 0 and line["higher_is_better"] is True
    assert abs(line["ms_per_step"] - 1e3 * 256 / line["value"]) < 0.01 * line["ms_per_step"]
    assert not [k for k in FULL_ONLY if k in line], line.keys()
    g, meta, arch = load_golden("blip_base256")
    ids, lens = np.load(d / "sequences.npy"), np.load(d / "lengths.npy")
    assert ids.dtype == np.float64 and ids.shape == (256, meta["max_length"]) and lens.shape == (256,)
    assert np.array_equal(ids, g["greedy_sequences"].astype(np.float64))
