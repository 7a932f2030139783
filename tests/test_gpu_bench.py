"""bench.py's plain run on the GPU box (-m gpu): the headline only, and --dump-outputs writing what the last timed step computed, the
same from run to run (seeded inputs and weights)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "HPE_FORCE_DIST")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "16",
           "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_dumps_its_outputs(tmp_path):
    a, b = _run(tmp_path / "a"), _run(tmp_path / "b")
    for d in (a, b):
        assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
        assert d["unit"] == "images/sec" and d["higher_is_better"] is True and d["dtype"] == "f32"
        # the extra measurements are --full's: a plain run carries none of them
        assert d["roofline"] is None and d["cpu_baseline"] is None
        assert not {"sustained", "parity", "configs", "graph", "from_host"} & set(d)
    names = sorted(f for f in os.listdir(tmp_path / "a") if f.endswith(".npy"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert names == sorted("stage%d_%s.npy" % (s, k) for s in (1, 2, 3) for k in ("verts", "joints", "cams", "theta", "J_transformed", "kp2d"))
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype == np.float32 and x.shape[0] == 16 and np.all(np.isfinite(x)), n
        assert np.array_equal(x, y), n  # the path is bitwise repeatable on the same inputs
    assert np.load(tmp_path / "a" / "stage3_verts.npy").shape == (16, 6890, 3)
