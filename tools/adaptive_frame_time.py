#!/usr/bin/env python3
"""What the image costs with the stopping rule applied to the whole frame and per pixel: a procedural cloud at
--size, the reference's constants (10 subframes per update, first test at 100, 2 %, 1e-2) and --cap samples per pixel at most.
  route (a)  the reference's loop: ct_render_accumulate_async in batches of 40 under ct_set_stop_when_converged(10, 100), read at
             the save points (every 40 subframes, as the headless CLI does) until the image has frozen or holds --cap subframes
  route (b)  the adaptive frame: ct_adaptive_frame_update(0) on a frame of R --round (10), min 100, max --cap
A window is one whole image from nothing, the same work every time; the two routes alternate, one warm-up window each and then
--repeats timed ones.  A window's time is a host clock around calls that end in a device synchronise.
One JSON line per route: the paths traced, wall ms of every window and their lowest / median / highest, the Msamples/s of the
estimator launches alone (paths over their GPU time), and the relative L2 distance of the route's RGB mean to a uniform render of
8 x route (a)'s count, beside the distance between two such renders (the noise floor).  The long renders use subframes that
neither route has drawn and that the other long render has not: subframes cap + 1 .. cap + 8 N and cap + 8 N + 1 .. cap + 16 N of one
progressive render, separated on the host in float64 from its running means at cap, cap + 8 N and cap + 16 N.
--shards N [N ...] measures something else: the shards of an N-GPU adaptive frame, driven one after the other on
this one GPU, each on a sharded handle of its own (ct_adaptive_frame_create_shard), alternating with the whole frame on the
unsharded handle -- one warm-up window each, then --repeats timed ones.  One JSON line per shard (own pixels, paths, rounds, wall
ms) and one per N: the slowest shard's lowest / median / highest beside the whole frame's from the same run.  What N GPUs would
take is the slowest shard plus the merge, which is not timed here.
Needs a GPU.  No threshold.
    python tools/adaptive_frame_time.py [--volume 256] [--size 512] [--cap 1000] [--round 10] [--repeats 5] [--estimator march|delta] [--mode 0]
                                        [--shards N [N ...]]"""
import argparse, json, statistics, sys, time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--volume", type=int, default=256)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--cap", type=int, default=1000)
    ap.add_argument("--round", type=int, default=10, help="R of route (b): subframes per live pixel and round (the reference's cadence: 10)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--estimator", choices=["march", "delta"], default="march")
    ap.add_argument("--mode", type=int, default=0)
    ap.add_argument("--shards", type=int, nargs="+", default=[], metavar="N",
                    help="instead of the two routes: the shards of an N-GPU job, one after the other on this GPU, beside the whole frame")
    a = ap.parse_args()
    if a.cap < 100 or a.cap % 40:
        sys.exit("--cap: a multiple of 40, at least 100")
    min_samples = -(-100 // a.round) * a.round                             # (the first multiple of R that is >= 100)
    if a.round < 1 or a.cap % a.round or min_samples > a.cap:
        sys.exit("--round: a divisor of --cap")
    import numpy as np
    import deepestscatter_amd as ds
    cloud = ds.make_procedural_cloud(a.volume)
    tr = ds.CloudTracer(cloud, width=a.size, height=a.size, mode=a.mode, estimator=0 if a.estimator == "march" else 1)
    pixels = a.size * a.size

    def uniform_window():
        tr.reset()
        tr.set_stop_when_converged(10, 100)
        paths0, ms0 = tr.counters()["paths"], tr.kernel_time()[0]
        t0 = time.perf_counter()
        done = at = 0
        while done < a.cap and not at:
            tr.render_accumulate_async(done + 1, 40)
            done += 40
            tr.synchronize()
            at = tr.converged_at()[0]
        wall = (time.perf_counter() - t0) * 1e3
        mean = tr.mean()
        tr.set_stop_when_converged(0, 100)
        return wall, mean, {"paths": tr.counters()["paths"] - paths0, "estimator_ms": tr.kernel_time()[0] - ms0, "stopped_at": at or done,
                            "frozen": bool(at), "subframes_rendered": done}

    def adaptive_window():
        with tr.adaptive_frame(round_samples=a.round, max_samples=a.cap, min_samples=min_samples, rel_tol=2e-2, abs_tol=1e-2) as f:
            t0 = time.perf_counter()
            info = f.update()
            wall = (time.perf_counter() - t0) * 1e3
            mean, counts = f.mean(), f.counts()
        return wall, mean, {"paths": info["paths"], "estimator_ms": info["trace_ms"], "fold_ms": info["fold_ms"], "test_ms": info["test_ms"],
                            "rounds": info["rounds"], "converged": info["converged"], "capped": info["capped"],
                            "round_samples": a.round, "pixels_done_at_first_test": int((counts == min_samples).sum()), "mean_count": float(counts.mean()), "max_count": int(counts.max())}

    def shard_windows(n):
        """The shards of an n-GPU job, one after the other on this GPU (each on a sharded handle of its own, ct_adaptive_frame_create_shard),
        alternating with the whole frame on the unsharded handle: one warm-up window each, then --repeats timed ones."""
        shards = [ds.CloudTracer(cloud, width=a.size, height=a.size, mode=a.mode, estimator=0 if a.estimator == "march" else 1,
                                 shard_index=i, shard_count=n) for i in range(n)]
        whole_walls, walls, facts, whole_facts = [], [[] for _ in shards], [None] * n, None
        for repeat in range(a.repeats + 1):
            wall, _, whole_facts = adaptive_window()
            if repeat:
                whole_walls.append(wall)
            for i, s in enumerate(shards):
                with s.adaptive_frame(round_samples=a.round, max_samples=a.cap, min_samples=min_samples, rel_tol=2e-2, abs_tol=1e-2, shard=True) as f:
                    t0 = time.perf_counter()
                    info = f.update()
                    wall = (time.perf_counter() - t0) * 1e3
                if repeat:
                    walls[i].append(wall)
                facts[i] = info
        for s in shards:
            s.close()
        for i, (w, info) in enumerate(zip(walls, facts)):
            print(json.dumps({"shards": n, "shard": i, "pixels": info["pixels"], "paths": info["paths"], "rounds": info["rounds"], "capped": info["capped"],
                              "wall_ms": [round(v, 2) for v in w], "lowest": min(w), "median": statistics.median(w), "highest": max(w),
                              "estimator_ms": info["trace_ms"]}), flush=True)
        medians = [statistics.median(w) for w in walls]
        slowest = max(range(n), key=lambda i: medians[i])
        assert sum(info["paths"] for info in facts) == whole_facts["paths"]   # the shards' paths are the whole frame's
        print(json.dumps({"shards": n, "volume": a.volume, "size": a.size, "estimator": a.estimator, "mode": a.mode, "cap": a.cap, "round_samples": a.round,
                          "windows": a.repeats, "slowest_shard": slowest, "slowest_shard_ms": [min(walls[slowest]), medians[slowest], max(walls[slowest])],
                          "whole_frame_ms": [min(whole_walls), statistics.median(whole_walls), max(whole_walls)], "whole_frame_paths": whole_facts["paths"],
                          "whole_frame_rounds": whole_facts["rounds"], "whole_over_slowest_shard": statistics.median(whole_walls) / medians[slowest],
                          "sum_of_shard_medians_ms": sum(medians)}), flush=True)

    if a.shards:
        for n in a.shards:
            shard_windows(n)
        tr.close()
        sys.exit(0)

    routes = {"(a) whole-frame rule, ct_set_stop_when_converged": uniform_window, "(b) adaptive frame": adaptive_window}
    walls = {name: [] for name in routes}
    last = {}
    for repeat in range(a.repeats + 1):                                   # (window 0 warms up: code objects, the scratch's growth)
        for name, window in routes.items():
            wall, mean, facts = window()
            if repeat:
                walls[name].append(wall)
            last[name] = (mean, facts)

    n = last["(a) whole-frame rule, ct_set_stop_when_converged"][1]["stopped_at"]
    tr.reset()
    snaps, done = [], 0
    for upto in (a.cap, a.cap + 8 * n, a.cap + 16 * n):
        while done < upto:
            step = min(4000, upto - done)
            tr.render_accumulate(done + 1, step)
            done += step
        snaps.append(tr.mean()[..., :3].astype(np.float64) * upto)          # (sums of the samples 1 .. upto)
    ref1, ref2 = (snaps[1] - snaps[0]) / (8 * n), (snaps[2] - snaps[1]) / (8 * n)

    def rel_l2(x, ref):
        return float(np.linalg.norm(x - ref) / np.linalg.norm(ref))

    floor = rel_l2(ref2, ref1)
    for name in routes:
        w = walls[name]
        mean, facts = last[name]
        line = {"route": name, "volume": a.volume, "size": a.size, "estimator": a.estimator, "mode": a.mode, "cap": a.cap, "windows": len(w),
                "wall_ms": [round(v, 2) for v in w], "lowest": min(w), "median": statistics.median(w), "highest": max(w),
                "Msamples_per_s_estimator": facts["paths"] / facts["estimator_ms"] / 1e3,
                "Msamples_per_s_wall": facts["paths"] / statistics.median(w) / 1e3,
                "paths_over_uniform_at_cap": facts["paths"] / (a.cap * pixels),
                "rel_l2_to_long_render": rel_l2(mean[..., :3].astype(np.float64), ref1), "rel_l2_between_long_renders": floor,
                "long_render_subframes": 8 * n, **facts}
        print(json.dumps(line), flush=True)
    tr.close()
