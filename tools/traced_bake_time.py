#!/usr/bin/env python3
"""What a traced bake (ct_bake_traced) costs and how close its pictures come to the path tracer's: a procedural
cloud, the default pose, a compact traced bake per grid (g^3 x --azimuths x --cosines) and sample count.  One JSON line each:
  the table's size, the active-node share, trace_ms and fold_ms (CtBakeTraceInfo), the bake's wall ms and paths per second
  (paths / trace_ms);
  the baked subframe's GPU ms (ct_debug_baked_render_time);
  the relative L2, over the pixels that have a record in one of the subframes, between the mean of
  baked_render_accumulate(direct=True) on the traced bake and the mode-0 path-traced mean of the same --subframes subframes;
  beside it the same distance between two path-traced means over disjoint subframe ranges (1 .. S and S + 1 .. 2 S): the noise
  floor a picture of S subframes cannot be told from.
--adaptive R,MAX[,REL[,ABS[,ZERO]]] (defaults: the reference's 0.02, 1e-4, 100000): per grid an adaptive bake
(ct_bake_traced_adaptive) in place of the --samples list -- its rounds, converged and capped shares, paths and
trace / fold / test ms (CtBakeAdaptiveInfo) -- and then a uniform bake of the nearest S with at least as many paths, each with
the same distances.
--shards N ...: the same bake on a group (ct_group_bake_*), rehearsed on one device: per N every shard's span
is traced alone, one after the other (ct_debug_bake_shard), and the slowest shard's trace_ms + fold_ms + test_ms and wall ms are
printed beside the whole bake's; then the bake is built once on TracerGroup([0] * N) for the bytes and the host ms of its
exchange (ct_debug_group_bake_exchange) and the wall ms of the whole group call, whose shards share the one device there.
Needs a GPU.  No threshold: resolution and samples are the user's trade.
    python tools/traced_bake_time.py [--volume 256] [--size 512] [--subframes 16] [--grids 16 32] [--azimuths 8] [--cosines 4]
                                     [--samples 4 16 | --adaptive 16,256] [--estimator march|delta] [--kind compact|sparse|dense]
                                     [--shards 2 4 8]"""
import argparse, json, statistics, sys, time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def rel_l2(a, b, where):
    import numpy as np
    a, b = a[where].astype(np.float64), b[where].astype(np.float64)
    den = (b ** 2).sum()
    return float(np.sqrt(((a - b) ** 2).sum() / den)) if den > 0 else None


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--volume", type=int, default=256)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--subframes", type=int, default=16)
    ap.add_argument("--grids", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--azimuths", type=int, default=8)
    ap.add_argument("--cosines", type=int, default=4)
    ap.add_argument("--samples", type=int, nargs="+", default=[4, 16])
    ap.add_argument("--adaptive", default=None, metavar="R,MAX[,REL[,ABS[,ZERO]]]")
    ap.add_argument("--estimator", choices=["march", "delta"], default="march")
    ap.add_argument("--kind", choices=["compact", "sparse", "dense"], default="compact")
    ap.add_argument("--shards", type=int, nargs="*", default=[])
    a = ap.parse_args()
    import numpy as np
    import torch  # noqa: F401  (before the library: descriptor_frame allocates through it)
    import deepestscatter_amd as ds
    S = a.subframes
    tr = ds.CloudTracer(ds.make_procedural_cloud(a.volume), width=a.size, height=a.size, estimator=0 if a.estimator == "march" else 1)
    # the path tracer's two means, and the pixels with a record
    tr.render_accumulate(1, S)
    first = tr.mean()[..., :3].astype(np.float64)
    tr.render_accumulate(S + 1, S)
    second = 2.0 * tr.mean()[..., :3].astype(np.float64) - first          # the mean of subframes S + 1 .. 2 S
    lit = np.zeros(a.size * a.size, bool)
    for sid in range(1, S + 1):
        lit[tr.descriptor_frame(sid)[3].cpu().numpy()] = True
    lit = lit.reshape(a.size, a.size)
    common = {"volume": a.volume, "frame": [a.size, a.size], "estimator": a.estimator, "kind": a.kind, "subframes": S,
              "pixels_with_a_record": int(lit.sum()),
              "relative_l2_of_two_path_traced_means": rel_l2(second, first, lit)}
    kw = {"compact": a.kind == "compact", "sparse": a.kind == "sparse"}
    adaptive = None
    if a.adaptive:
        v = a.adaptive.split(",")
        adaptive = dict(zip(("round_samples", "max_samples", "rel_tol", "abs_tol", "zero_samples"),
                            [int(v[0]), int(v[1])] + [float(x) for x in v[2:4]] + [int(x) for x in v[4:5]]))
    for g in a.grids:
        runs = [None] if adaptive else list(a.samples)                    # None: the adaptive bake, which appends its uniform twin
        for samples in runs:
            t0 = time.perf_counter()
            if samples is None:
                bake = tr.traced_bake_adaptive((g, g, g), a.azimuths, a.cosines, **adaptive, **kw)
            else:
                bake = tr.traced_bake((g, g, g), a.azimuths, a.cosines, samples, **kw)
            wall = (time.perf_counter() - t0) * 1e3
            ti, sp, st = bake.trace_info(), bake.sparse_info, bake.storage_info
            extra = {}
            if samples is None:
                ai = bake.adaptive_info()
                extra = {"adaptive": adaptive, "rounds": ai["rounds"], "entries_active": ai["entries_active"],
                         "converged_share": ai["converged"] / max(ai["entries_active"], 1), "capped_share": ai["capped"] / max(ai["entries_active"], 1),
                         "test_ms": ai["test_ms"], "mean_samples_per_entry": ai["paths"] / max(ai["entries_active"], 1)}
                runs.append(min(65535, max(1, -(-ai["paths"] // max(ai["entries_active"], 1)))))
            gpu = []
            for _ in range(6):                                            # (the first subframe of a fresh table reads it cold)
                tr.baked_render_subframe(bake, 1, out=False, direct=True)
                gpu.append(tr.baked_render_time())
            tr.reset()
            tr.baked_render_accumulate(bake, 1, S, direct=True)
            got = tr.mean()[..., :3].astype(np.float64)
            print(json.dumps({"route": "ct_bake_traced_adaptive" if samples is None else "ct_bake_traced", **common, **extra,
                              "grid": [g, g, g, a.azimuths, a.cosines], "samples": ti["samples"],
                              "nodes": sp["nodes"], "active_nodes": sp["active_nodes"], "active_share": sp["active_nodes"] / sp["nodes"],
                              "table_bytes": st["table_bytes"], "paths": ti["paths"], "trace_ms": ti["trace_ms"], "fold_ms": ti["fold_ms"],
                              "bake_wall_ms": wall, "paths_per_second": ti["paths"] / ti["trace_ms"] * 1e3 if ti["trace_ms"] > 0 else None,
                              "baked_subframe_gpu_ms": statistics.median(gpu[1:]),
                              "relative_l2_against_the_path_traced_mean": rel_l2(got, first, lit)}), flush=True)
            bake.close()
            for n in a.shards:                                            # the same job cut for a group of n, on this one device
                from deepestscatter_amd.network import AdaptiveParams, Bake
                per_shard = []
                for i in range(n):
                    t0 = time.perf_counter()
                    if samples is None:
                        part = Bake.traced_shard(tr, (g, g, g), a.azimuths, a.cosines, i, n, adaptive=AdaptiveParams(**adaptive), **kw)
                    else:
                        part = Bake.traced_shard(tr, (g, g, g), a.azimuths, a.cosines, i, n, samples=samples, **kw)
                    shard_wall = (time.perf_counter() - t0) * 1e3
                    pi, pa = part.trace_info(), part.adaptive_info()
                    per_shard.append({"wall_ms": shard_wall, "gpu_ms": pi["trace_ms"] + pi["fold_ms"] + pa["test_ms"], "paths": pi["paths"],
                                      "rounds": pa["rounds"]})
                    part.close()
                grp = ds.TracerGroup(ds.make_procedural_cloud(a.volume), [0] * n, width=a.size, height=a.size,
                                     estimator=0 if a.estimator == "march" else 1)
                t0 = time.perf_counter()
                if samples is None:
                    gb = grp.traced_bake_adaptive((g, g, g), a.azimuths, a.cosines, **adaptive, **kw)
                else:
                    gb = grp.traced_bake((g, g, g), a.azimuths, a.cosines, samples, **kw)
                group_wall = (time.perf_counter() - t0) * 1e3
                ex = gb.exchange_info()
                gb.close()
                grp.close()
                print(json.dumps({"route": "ct_group_bake_traced_adaptive" if samples is None else "ct_group_bake_traced", "rehearsal": "one device",
                                  "grid": [g, g, g, a.azimuths, a.cosines], "samples": ti["samples"], "shards": n,
                                  "whole_bake_gpu_ms": ti["trace_ms"] + ti["fold_ms"] + extra.get("test_ms", 0.0), "whole_bake_wall_ms": wall,
                                  "slowest_shard_gpu_ms": max(s["gpu_ms"] for s in per_shard),
                                  "slowest_shard_wall_ms": max(s["wall_ms"] for s in per_shard),
                                  "shard_gpu_ms": [round(s["gpu_ms"], 3) for s in per_shard], "shard_paths": [s["paths"] for s in per_shard],
                                  "shard_rounds": [s["rounds"] for s in per_shard],
                                  "exchange_bytes": ex["bytes"], "exchange_ms": ex["ms"], "group_call_wall_ms_on_one_device": group_wall}), flush=True)
    tr.close()
