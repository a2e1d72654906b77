"""bench.py without --full on one GPU: the run times exactly --steps steps and prints the headline line only (no legs, no
roofline, no CPU baseline, no reference comparison), and --dump-outputs writes what the last timed step returned - for
rank 0's samples 0 and 1 the reference golden's root cubes and proposals (tests/golden/rootnet_full.npz)."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_prints_the_headline_and_dumps_the_step_outputs(tmp_path):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    out = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2",
           "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["metric"] == "multi-view samples/sec (5-view Panoptic, 80x80x20 voxel)"
    assert rec["unit"] == "samples/s" and rec["higher_is_better"] is True and rec["dtype"] == "f32"
    assert rec["steps"] == 5 and rec["warmup"] == 2 and rec["n_gpus"] == 1 and rec["full"] is False
    assert rec["ms_per_step"] > 0 and abs(rec["value"] - 4e3 / rec["ms_per_step"]) <= 1e-3 * rec["value"]
    for k in ("roofline", "cpu_baseline", "cpu_reference", "output_check", "box_spread", "fp32_matrix_instructions_only"):
        assert k not in rec, k
    assert rec["legs"] == {} and rec["legs_complete"] is True
    rc, gc = np.load(out / "root_cubes.npy"), np.load(out / "grid_centers.npy")
    assert rc.dtype == np.float32 and gc.dtype == np.float32
    assert rc.shape == (4, 80, 80, 20) and gc.shape == (4, 10, 5)
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    chk = bench.check_output((torch.from_numpy(rc), torch.from_numpy(gc)),
                             np.load(os.path.join(ROOT, "tests", "golden", "rootnet_full.npz")))
    assert chk["ok"], chk
