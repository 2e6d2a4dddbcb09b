"""bench.py contract (driver reads this JSON line) on the tiny BASELINE config 1, a plain run against a --full run on config 2,
and __graft_entry__.smoke()."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_emits_one_contract_line_with_roofline_and_cpu_baseline(tmp_path):
    dump = tmp_path / "outputs"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--config", "c1", "--steps", "3", "--warmup",
                          "1", "--cpu-sample", "2", "--cpu-threads", "4", "--dump-outputs", str(dump)], capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    j = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in j, k
    assert j["metric"] == "utterances/sec" and j["n_gpus"] == 1 and j["steps"] == 3 and j["scaling"] == "weak"
    assert j["dtype"] == "f32" and j["vs_baseline"] is None and j["value"] > 0
    assert set(("bound", "achieved", "peak", "unit", "frac", "traffic")) <= set(j["roofline"])
    assert abs(j["roofline"]["frac"] - j["roofline"]["achieved"] / j["roofline"]["peak"]) < 1e-3
    assert j["roofline"]["launches"] > 0 and j["roofline"]["profiled_steps"].startswith("1 of the 3 timed steps")
    assert j["cpu_baseline"]["kind"] == "port" and j["cpu_baseline"]["cores"] == 4 and j["cpu_baseline"]["value"] > 0
    assert j["loss_rel_delta"] < 1e-4          # north_star tolerance on the whole path (mel, label) -> loss
    assert "workload" in j["config"] and "model" not in j["config"]
    assert set(j["grad_max_abs_dev"]) == {"fc.weight", "encoder.rnn.weight_hh_l0", "decoder.embedding.weight"}
    for v in j["grad_max_abs_dev"].values():   # vs the FLOAT64 oracle at the INITIAL weights: the fixture tests' bound, no widening
        assert v["max_abs_dev"] <= 2e-4 * max(v["ref_max_abs"], 1e-3)
    assert j["parity"]["ok"] is True and j["parity"]["all_rows_finite"] is True and "INITIAL weights" in j["parity"]["oracle"]
    assert j["parity_after_training"]["informational"] is True      # reported next to the fp32 oracle's own distance, never a gate
    assert "fp32_oracle_max_abs_dev" in j["parity_after_training"]["grad_max_abs_dev"]["fc.weight"]
    assert j["rccl_ranks"] == 1
    assert j["cpu_baseline"]["cpu_model"] and j["cpu_baseline"]["host_logical_cpus"] >= 4
    assert "1 warm-up" in j["cpu_baseline"]["sample"] and "3 timed" in j["cpu_baseline"]["sample"]
    assert j["memory"]["peak_allocated_bytes"] > 0
    # --dump-outputs: the last timed step's loss, gradients and updated weights (c1 is small enough to be dumped whole)
    files = sorted(os.listdir(dump))
    assert "loss.npy" in files and "grad.jointnet.fc.weight.npy" in files and "param.jointnet.fc.weight.npy" in files
    assert all(np.load(dump / f).dtype in (np.float32, np.float64) for f in files)
    assert sum((dump / f).stat().st_size for f in files) <= 64 << 20
    assert abs(float(np.load(dump / "loss.npy")) - j["last_loss"]) < 1e-3
    assert np.isfinite(np.load(dump / "grad.jointnet.fc.weight.npy")).all()


def test_plain_bench_run_times_what_the_full_run_times(tmp_path):
    """A run without --full prints the same contract line without the CPU legs, and its timed steps compute what those of a --full
    run compute.  On c2, whose 4-layer encoder applies inter-layer dropout: the masks follow the recurrent layers' call counters, so the
    dumped outputs agree only if both runs time the same masks (another mask moves the gradients by far more than the bound)."""
    common = ["--config", "c2", "--steps", "2", "--warmup", "1", "--parity-sample", "1"]
    runs = {}
    for mode, extra in (("plain", []), ("full", ["--full", "--cpu-sample", "1"])):
        dump = tmp_path / mode
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + common + extra + ["--dump-outputs", str(dump)],
                             capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1
        runs[mode] = (json.loads(lines[0]), dump)
    plain, full = runs["plain"][0], runs["full"][0]
    for k in ("metric", "unit", "higher_is_better", "dtype", "n_gpus", "steps", "warmup", "scaling", "data", "config"):
        assert plain[k] == full[k], k
    assert plain["value"] > 0 and plain["ms_per_step"] > 0 and "roofline" in plain
    for k in ("cpu_baseline", "speedup_vs_cpu_baseline", "parity", "loss_rel_delta", "grad_max_abs_dev", "parity_after_training"):
        assert k not in plain and k in full, k
    assert full["parity"]["ok"] is True
    assert abs(plain["last_loss"] - full["last_loss"]) <= 1e-6 * abs(full["last_loss"])
    files = sorted(os.listdir(runs["full"][1]))
    assert files and sorted(os.listdir(runs["plain"][1])) == files
    for f in files:
        a, b = np.load(runs["plain"][1] / f), np.load(runs["full"][1] / f)
        assert a.shape == b.shape and np.abs(a - b).max() <= 1e-6 * max(float(np.abs(b).max()), 1e-30), f


def test_smoke_entry_point():
    sys.path.insert(0, ROOT)
    import __graft_entry__
    __graft_entry__.smoke()
