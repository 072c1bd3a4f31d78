"""bench.py's plain run and --full: a plain run prints the headline line alone (no roofline, no cpu_baseline, no `also`),
and --full adds them around the SAME timed steps -- the same losses, the same dumped outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_plain_line_is_the_headline_and_full_adds_the_rest(tmp_path):
    common = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--unrolls-per-step", "2"]
    plain = _bench(common + ["--dump-outputs", str(tmp_path / "plain")])
    assert plain["metric"].startswith("unroll-steps/sec") and plain["unit"] == "coordinate-steps/s"
    assert plain["higher_is_better"] is True and plain["dtype"] == "f32"
    assert plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["steps"] == 3 and plain["warmup"] == 1
    assert plain["config"]["kernel"].startswith("k_unroll_pair")
    assert not {"roofline", "cpu_baseline", "also", "value_replayed_problem"} & set(plain), sorted(plain)
    full = _bench(common + ["--full", "--no-also", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "full")])
    assert full["roofline"]["kernel_ms_avg"] > 0 and full["roofline"]["hbm_copy_measured_GBps"] > 0
    assert full["value_replayed_problem"] > 0 and "also" not in full
    assert full["fx_0"] == pytest.approx(plain["fx_0"], rel=1e-6)
    assert full["final_loss_fx_T"] == pytest.approx(plain["final_loss_fx_T"], rel=1e-6)
    names = sorted(os.listdir(str(tmp_path / "plain")))
    assert "fx.npy" in names and names == sorted(os.listdir(str(tmp_path / "full")))
    for n in names:
        np.testing.assert_allclose(np.load(str(tmp_path / "full" / n)), np.load(str(tmp_path / "plain" / n)),
                                   rtol=1e-5, atol=1e-7, err_msg=n)
