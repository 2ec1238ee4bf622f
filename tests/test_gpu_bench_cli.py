"""bench.py's command line on the GPU, on a 2-layer cut of its workload
(--layers 2, 2 requests, 16 + 8 tokens; the full-size workload is
test_gpu_bench_workload.py's): a plain run times --steps generates and
prints only the headline line, --dump-outputs writes the last timed
generate's tokens and the same arguments give the same arrays again, and
--full adds the side runs behind the timed steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, P, D, STEPS = 2, 16, 8, 2
SMALL = ["--gpus", "1", "--layers", "2", "--batch", str(B), "--prefill", str(P),
         "--decode", str(D), "--steps", str(STEPS), "--warmup", "1"]
SIDE_KEYS = ("roofline", "op_breakdown_sampled", "incr_decoding", "spec_width4", "spec_4ssm",
             "spec_token_chain", "cpu_baseline")


def bench(*args):
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, *args],
                       capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_plain_run_is_the_headline_only_and_dumps_reproducible_outputs(tmp_path):
    d = bench("--dump-outputs", str(tmp_path / "a"))
    assert d["unit"] == "tokens/s" and d["higher_is_better"] is True and d["dtype"] == "f16"
    assert d["metric"].startswith("decoded tokens/s") and d["steps"] == STEPS
    assert not [k for k in SIDE_KEYS if k in d]
    # value = decoded tokens / time of the STEPS timed generates
    assert d["value"] * d["ms_per_step"] * 1e-3 == pytest.approx(B * D, rel=0.01)
    assert sorted(os.listdir(tmp_path / "a")) == ["output_lengths.npy", "output_tokens.npy"]
    toks = np.load(tmp_path / "a" / "output_tokens.npy")
    lens = np.load(tmp_path / "a" / "output_lengths.npy")
    assert toks.dtype == np.float64 and toks.shape == (B, P + D)
    assert lens.dtype == np.float64 and lens.tolist() == [P + D] * B
    assert np.all(toks == np.round(toks)) and toks.min() >= 0 and toks.max() < 32000
    sys.path.insert(0, ROOT)
    from bench import make_prompts
    assert toks[:, 1:P].tolist() == make_prompts(B, P - 1, 32000)  # (column 0: BOS)
    bench("--dump-outputs", str(tmp_path / "b"))
    assert np.array_equal(np.load(tmp_path / "b" / "output_tokens.npy"), toks)
    assert np.array_equal(np.load(tmp_path / "b" / "output_lengths.npy"), lens)


def test_full_run_adds_the_side_runs():
    d = bench("--full", "--no-cpu-baseline")
    assert d["steps"] == STEPS and d["ms_per_step"] > 0
    assert not [k for k in SIDE_KEYS[:-1] if k not in d]
    assert "cpu_baseline" not in d
