#!/usr/bin/env python3
"""What an update of the radiance collector costs with its loop on the host (collector.RadianceCollector over
ct_point_radiance_launch) and on the device (ct_collector_*): a procedural cloud, --tasks tasks from
ct_generate_scatter_samples, the reference's constants (20 480 threads, 100 launches per update, 2 %, 1e-4, 100 000).
A window is the first --updates updates of a fresh collector, the same work every time; the two routes alternate, one warm-up
window each and then --repeats timed ones.  A window's time is a host clock around calls that end in a device synchronise.
One JSON line per route: wall ms per update of every window, their lowest, median and highest; for the device collector also
trace_ms / fold_ms / test_ms per update of the lowest window (CtCollectorInfo: the estimator launches, the rays and
fold-and-merge kernels, the scan and compaction) and what is left of the wall time beside them -- the host's share, launches and
waits included.  The routes' tasks after the window are compared bit for bit.
Needs a GPU.  No threshold.
    python tools/collect_time.py [--volume 256] [--tasks 2048] [--updates 20] [--repeats 7] [--estimator march|delta]"""
import argparse, json, statistics, sys, time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--volume", type=int, default=256)
    ap.add_argument("--tasks", type=int, default=2048)
    ap.add_argument("--updates", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--estimator", choices=["march", "delta"], default="march")
    a = ap.parse_args()
    import deepestscatter_amd as ds
    from deepestscatter_amd import collector as col
    tr = ds.CloudTracer(ds.make_procedural_cloud(a.volume), width=64, height=64, mode=1, estimator=0 if a.estimator == "march" else 1)
    pos, view = tr.generate_scatter_samples(a.tasks, 0)

    def host_window():
        t0 = time.perf_counter()
        tasks, converged_update, history = col.collect_reference(tr.point_radiance_launch, pos, view, updates=a.updates)
        return (time.perf_counter() - t0) * 1e3 / len(history), tasks, converged_update, None

    def device_window():
        with tr.radiance_collector(pos, view) as c:
            t0 = time.perf_counter()
            c.update(a.updates)
            info = c.info()
            wall = (time.perf_counter() - t0) * 1e3 / info["updates"]
            tasks, converged_update = c.tasks()
        return wall, tasks, converged_update, info

    routes = {"host loop over ct_point_radiance_launch": host_window, "ct_collector_update": device_window}
    walls = {name: [] for name in routes}
    last = {}
    for repeat in range(a.repeats + 1):                                   # (window 0 warms up: code objects, the point buffers' growth)
        for name, window in routes.items():
            wall, tasks, converged_update, info = window()
            if repeat:
                if not walls[name] or wall < min(walls[name]):
                    last[name] = info
                walls[name].append(wall)
            last[name + " state"] = (tasks.tobytes(), converged_update.tobytes())
    same = last["host loop over ct_point_radiance_launch state"] == last["ct_collector_update state"]
    for name in routes:
        w = walls[name]
        line = {"route": name, "volume": a.volume, "tasks": a.tasks, "estimator": a.estimator, "updates_per_window": a.updates, "windows": len(w),
                "wall_ms_per_update": [round(v, 3) for v in w], "lowest": min(w), "median": statistics.median(w), "highest": max(w),
                "tasks_equal_bit_for_bit": same}
        info = last.get(name)
        if info:
            n = info["updates"]
            line.update({"trace_ms_per_update": info["trace_ms"] / n, "fold_ms_per_update": info["fold_ms"] / n, "test_ms_per_update": info["test_ms"] / n,
                         "host_share_ms_per_update": min(w) - (info["trace_ms"] + info["fold_ms"] + info["test_ms"]) / n,
                         "remaining_after_the_window": info["remaining"], "repeat_count_after_the_window": info["repeat_count"]})
        print(json.dumps(line), flush=True)
    tr.close()
    sys.exit(0 if same else 1)
