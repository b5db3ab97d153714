"""bench.py's plain run and its --dump-outputs: the frame a plain run writes is the frame whose SHA-256 the --full line
carries, and a frame beyond the size budget is written as a fixed seeded sample of its pixels."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]


def test_dump_outputs_sample_a_frame_over_the_budget(tmp_path):
    """write_outputs in a child process (importing bench.py sets an environment default this process should not inherit):
    a frame over the budget becomes the same seeded pixel sample of every buffer, within the budget, run after run."""
    script = f"""
import sys
import numpy as np
sys.path.insert(0, {str(ROOT)!r})
import bench
rng = np.random.default_rng(7)
a, b = rng.random((48, 64, 4), dtype=np.float32), rng.random((48, 64, 4), dtype=np.float32)
np.save({str(tmp_path / "a.npy")!r}, a)
np.save({str(tmp_path / "b.npy")!r}, b)
for d in ("whole", "s1", "s2"):
    bench.write_outputs({str(tmp_path)!r} + "/" + d, {{"mean": a, "m2": b}}, budget=10 ** 9 if d == "whole" else 24000)
"""
    subprocess.run([sys.executable, "-c", script], check=True, cwd=str(ROOT), timeout=120)
    a, b = np.load(tmp_path / "a.npy"), np.load(tmp_path / "b.npy")
    whole = tmp_path / "whole"
    assert sorted(p.name for p in whole.iterdir()) == ["m2.npy", "mean.npy"]
    assert np.array_equal(np.load(whole / "mean.npy"), a) and np.array_equal(np.load(whole / "m2.npy"), b)
    s1, s2 = tmp_path / "s1", tmp_path / "s2"
    names = sorted(p.name for p in s1.iterdir())
    assert names == ["m2.npy", "mean.npy", "sample_pixel_index.npy"]
    assert sum((s1 / n).stat().st_size for n in names) <= 24000
    idx = np.load(s1 / "sample_pixel_index.npy")
    assert idx.dtype == np.float64 and len(idx) > 0 and np.all(np.diff(idx) > 0)
    flat = idx.astype(np.int64)
    for n, full in (("mean.npy", a), ("m2.npy", b)):
        got = np.load(s1 / n)
        assert got.dtype == np.float32 and np.array_equal(got, full.reshape(-1, 4)[flat])
    assert all(np.array_equal(np.load(s1 / n), np.load(s2 / n)) for n in names)


@pytest.mark.gpu
def test_plain_run_dumps_the_frame_the_full_line_hashes(tmp_path):
    """A plain run (no --full) prints the headline without the legs, and its --dump-outputs frame is the [mean | M2] whose
    SHA-256 the --full line of the same arguments reports."""
    import hashlib
    common =[sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--volume", "64", "--width", "128",
              "--height", "96", "--spp-per-step", "24"]
    got = {}
    for name, extra in (("plain", ["--dump-outputs", str(tmp_path / "out")]),
                        ("full", ["--full", "--no-cpu-baseline", "--no-pmc-traffic", "--no-delta-leg", "--no-progressive-leg"])):
        r = subprocess.run(common + extra, capture_output=True, text=True, timeout=600, cwd=str(ROOT))
        assert r.returncode == 0, name + ": " + r.stdout[-1500:] + r.stderr[-3000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{") and '"metric"' in l]
        assert len(lines) == 1, name
        got[name] = json.loads(lines[0])
    plain, full = got["plain"], got["full"]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in plain, k
    assert plain["steps"] == 3 and plain["ms_per_step"] > 0 and plain["value"] > 0 and plain["subframes_in_the_frame"] == 96
    assert "frame_sha256" not in plain and plain["cpu_baseline"] is None
    assert not any(k in plain for k in ("progressive_10spp", "delta_estimator"))
    mean, m2 = np.load(tmp_path / "out" / "mean.npy"), np.load(tmp_path / "out" / "m2.npy")
    assert mean.dtype == m2.dtype == np.float32 and mean.shape == m2.shape == (96, 128, 4)
    assert hashlib.sha256(mean.tobytes() + m2.tobytes()).hexdigest() == full["frame_sha256"]     # (bench.frame_sha256)
