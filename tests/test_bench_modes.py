"""bench.py's two modes: a plain run (set-up, warm-up, timed regions, --dump-outputs, result line) and --full (every side
measurement and check after the same timed regions)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from markushgrapher_amd import synth

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.mark.parametrize("shape_name, B", [("tiny", 3), ("large", 2)])
def test_bench_inputs_equal_synth_batch(shape_name, B):
    """bench.bench_batch (no host pixel_values) hands the timed region exactly the fields of synth.synth_batch(..., return_pages=True)
    that it uploads: the text fields and the 1024 px (2 x image_size) pages."""
    import bench
    shape = synth.SHAPES[shape_name]
    for seed in (synth.BENCH_SEED, synth.BENCH_SEED + 1000, synth.BENCH_SEED + 1 + 2000):
        want = synth.synth_batch(shape, B, seed=seed, return_pages=True)
        got = bench.bench_batch(shape, B, seed=seed)
        assert sorted(got) == sorted(k for k in want if k != "pixel_values")
        for k in got:
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k


def _run(args, timeout=900):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.gpu
def test_bench_plain_and_full_time_the_same_steps(tmp_path):
    """Tiny configuration (3 steps over 2 contexts): the plain run reports the headline with the side figures null; --full (side runs
    that need the large shape or other models switched off) fills the one-batch, one-call and phase figures and the per-batch identity
    check.  Both runs dump the same arrays."""
    common = ["--shape", "tiny", "--batch", "2", "--new-tokens", "6", "--steps", "3", "--warmup", "1", "--repeats", "1", "--inflight", "2",
              "--batches-per-call", "2"]
    plain = _run(common + ["--dump-outputs", str(tmp_path / "plain")])
    full = _run(common + ["--full", "--no-extra-runs", "--no-cpu-baseline", "--no-pmc", "--dump-outputs", str(tmp_path / "full")])
    for out in (plain, full):
        assert out["steps"] == 3 and out["warmup"] == 1 and out["value"] > 0 and out["ms_per_step"] > 0
        assert out["unit"] == "images/s" and out["higher_is_better"] is True and out["dtype"] == "bf16"
    assert plain["full"] is False and full["full"] is True
    for k in ("roofline", "phases", "one_call_alone", "one_batch_in_flight", "extra_runs", "cpu_baseline", "images_per_s_one_batch_in_flight"):
        assert plain[k] is None, k
    assert plain["config"]["ids_equal_one_batch_calls"] is None
    assert full["config"]["ids_equal_one_batch_calls"] is True
    assert full["one_batch_in_flight"]["images_per_s"] > 0 and full["one_call_alone"]["batches_per_call"] == 2
    assert full["one_batch_in_flight"]["phases"] is not None and full["one_batch_in_flight"]["roofline"] is not None
    for n in ("ids", "gathered_ids", "gathered_lengths"):
        a, b = np.load(tmp_path / "plain" / f"{n}.npy"), np.load(tmp_path / "full" / f"{n}.npy")
        assert np.array_equal(a, b), n
