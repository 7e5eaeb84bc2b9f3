"""bench.py on the device: a plain run and what --dump-outputs writes.  Needs a real MI355X: run with ``-m gpu``."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests.helpers import Inputs, compare_clouds, sort_cloud

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]


def _bench(args: list[str]) -> dict:
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    proc = subprocess.run([sys.executable, str(ROOT / "bench.py")] + args, env=env, capture_output=True, text=True,
                          timeout=300)
    assert proc.returncode == 0, proc.stderr[-3000:]
    lines = [ln for ln in proc.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, proc.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.timeout(900)
def test_bench_dump_outputs_are_the_last_steps_events(tmp_path):
    """Two plain runs with the same arguments dump the same arrays (float64, within 64 MB); the sampled events lie in
    the last timed step's id range, the step's counts agree with the line, and sampled events match the CPU oracle."""
    from oracle import pyoracle as orc

    events, steps, seed = 4000, 2, 3
    args = ["--gpus", "1", "--steps", str(steps), "--warmup", "1", "--events", str(events), "--seed", str(seed)]
    lines, dumps = [], []
    for tag in ("a", "b"):
        lines.append(_bench(args + ["--dump-outputs", str(tmp_path / tag)]))
        dumps.append({p.stem: np.load(p) for p in sorted((tmp_path / tag).iterdir())})
    line, (a, b) = lines[0], dumps
    assert line["steps"] == steps and line["ms_per_step"] > 0
    assert "cpu_baseline" not in line and "delivered" not in line
    assert sorted(a) == ["event_ids", "labels", "offsets", "p4", "points", "status", "step_counts", "vertex"]
    assert sum(p.stat().st_size for p in (tmp_path / "a").iterdir()) <= 64_000_000
    for name in a:
        assert a[name].dtype == np.float64, name
        np.testing.assert_array_equal(a[name], b[name], err_msg=name)
    ids = a["event_ids"].astype(np.int64)
    assert len(ids) == 64 and ids.min() >= (steps - 1) * events and ids.max() < steps * events
    assert a["step_counts"][0] == events and a["step_counts"][3] == 0  # events of the step, no failed event
    offsets = a["offsets"].astype(np.int64)
    assert offsets[0] == 0 and offsets[-1] == len(a["points"]) == len(a["labels"]) and len(offsets) == len(ids) + 1

    inp = Inputs("o16aa", seed=seed)
    for k in (0, len(ids) - 1):
        ref = orc.sim_batch(inp.kin, inp.det_raw, inp.layout, seed=seed, first=int(ids[k]), n=1, capacity=1 << 20,
                            threads=4)
        np.testing.assert_allclose(a["p4"][k], ref["p4"][0], rtol=0, atol=1e-9)
        np.testing.assert_allclose(a["vertex"][k], ref["vertex"][0], rtol=0, atol=1e-12)
        lo, hi = offsets[k], offsets[k + 1]
        got = sort_cloud(a["points"][lo:hi], a["labels"][lo:hi].astype(np.int64))
        compare_clouds(*got, *sort_cloud(ref["points"], ref["labels"]))
