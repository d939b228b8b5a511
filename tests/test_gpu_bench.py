"""bench.py's output contract (the driver parses ONE JSON line per run): a short default-config
--full run at N=1 -- the metric / config of BASELINE.json, the roofline object with a live measurement
(achieved / peak = frac, HBM traffic from the committed PMC summary), whole-job throughput
consistent with ms_per_step, and the DDIM legs -- so a change to the bench cannot silently drop a
field the round-end run needs -- and the --dump-outputs files of the same run (what the last timed
step computed, float32, within the 64 MB budget)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_json_contract(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    log = tmp_path / "bench.log"
    dump = tmp_path / "dump"
    cmd = [sys.executable, "bench.py", "--full", "--steps", "3", "--warmup", "1", "--skip-cpu", "--ddim-steps", "20",
           "--dump-outputs", str(dump)]
    with open(log, "w") as fh:
        r = subprocess.run(cmd, cwd=REPO, stdout=fh, stderr=subprocess.STDOUT, timeout=600)
    out = open(log).read()
    assert r.returncode == 0, out[-3000:]
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    base = json.load(open(os.path.join(REPO, "BASELINE.json")))
    assert d["metric"].startswith("training imgs/sec") and base["metric"].startswith(d["metric"][:20])
    for k in ("value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "imgs/s"
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["dtype"] == "bf16"
    assert "workload" in d["config"] and d["config"]["global_batch"] == 128
    # value = whole-job images / timed seconds
    assert abs(d["value"] - 128 * 1000.0 / d["ms_per_step"]) / d["value"] < 1e-6
    rf = d["roofline"]
    assert rf["bound"] in ("hbm", "mfma") and rf["unit"] in ("GB/s", "TFLOP/s")
    assert 0 < rf["achieved"] < rf["peak"] and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-9
    assert rf["traffic"] is None or rf["traffic"] > 0
    for k in ("ddim_steps_per_sec", "ddim_steps_per_sec_b128"):
        assert d[k]["value"] > 0, k
    # the dump: the last timed step's loss, denoiser output and arena samples
    arrs = {f[:-4]: np.load(dump / f) for f in sorted(os.listdir(dump))}
    assert set(arrs) == {"loss", "eps", "grad", "params", "ema"}, sorted(arrs)
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= 64 * 2 ** 20
    assert arrs["eps"].shape == (128, 3, 16, 16) and arrs["eps"].std() > 0
    assert arrs["grad"].shape == arrs["params"].shape == arrs["ema"].shape and np.abs(arrs["grad"]).max() > 0
    # the dump is written before any later leg steps the model again: its loss is the line's
    assert float(arrs["loss"][0]) == d["loss_simple_last"]
