#!/usr/bin/env python3
"""What a hybrid frame (ct_baked_render_hybrid_*) costs per traced collision and what the depth buys: a
procedural cloud, the default pose, MARCH, compact traced bakes of g^3 x --azimuths x --cosines with --samples experiments per
entry.  Per bake and depth one JSON line:
  the subframe's GPU ms (ct_debug_baked_render_time) as lowest / median / highest of --repeats, the routes -- ct_baked_render_subframe
  and every depth -- taking turns within a repeat; the depth-1 row is to reproduce ct_baked_render_subframe's time, the control;
  the relative L2, over the whole frame, between the mean of baked_render_hybrid_accumulate over subframes 1 .. S and a
  path-traced mean over the L subframes S + 1 .. S + L, which shares no subframe with it.
Before them one line with the two yardsticks for that distance: the same distance between that path-traced mean and a second
one over S + L + 1 .. S + 2 L (the noise floor), and the path tracer's own mean over subframes 1 .. S.
Needs a GPU.  No threshold: the depth is the user's trade.
    python tools/hybrid_render_time.py [--volume 256] [--size 512] [--subframes 64] [--long 2048] [--grids 16 32] [--azimuths 16]
                                       [--cosines 8] [--samples 256] [--depths 1 2 4 8 16] [--repeats 5]"""
import argparse, json, statistics, sys
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def rel_l2(a, b):
    import numpy as np
    den = (b ** 2).sum()
    return float(np.sqrt(((a - b) ** 2).sum() / den)) if den > 0 else None


def spread(v):
    return [round(min(v), 4), round(statistics.median(v), 4), round(max(v), 4)]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--volume", type=int, default=256)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--subframes", type=int, default=64)
    ap.add_argument("--long", type=int, default=2048)
    ap.add_argument("--grids", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--azimuths", type=int, default=16)
    ap.add_argument("--cosines", type=int, default=8)
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--depths", type=int, nargs="+", default=[1, 2, 4, 8, 16])
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import numpy as np
    import torch  # noqa: F401  (before the library, as everywhere)
    import deepestscatter_amd as ds
    S, L = a.subframes, a.long
    tr = ds.CloudTracer(ds.make_procedural_cloud(a.volume), width=a.size, height=a.size, estimator=0)

    def image():
        return tr.mean()[..., :3].astype(np.float64)

    # the path tracer: subframes 1 .. S, then two long means over disjoint ranges behind them
    tr.render_accumulate(1, S)
    short = image()
    tr.render_accumulate(S + 1, L)
    upto = image()
    long_a = ((S + L) * upto - S * short) / L
    tr.render_accumulate(S + L + 1, L)
    long_b = ((S + 2 * L) * image() - (S + L) * upto) / L
    common = {"volume": a.volume, "frame": [a.size, a.size], "estimator": "march", "subframes": S, "long_subframes": L}
    print(json.dumps({"route": "ct_render_accumulate", **common,
                      "relative_l2_of_the_two_long_means": rel_l2(long_b, long_a),
                      "relative_l2_of_the_path_traced_mean_of_S_subframes": rel_l2(short, long_a)}), flush=True)
    for g in a.grids:
        bake = tr.traced_bake((g, g, g), a.azimuths, a.cosines, a.samples, compact=True)
        ti, sp, st = bake.trace_info(), bake.sparse_info, bake.storage_info
        routes = [None] + list(a.depths)                                  # None: ct_baked_render_subframe
        gpu = {r: [] for r in routes}
        for rep in range(a.repeats + 1):                                  # (the first round reads a fresh table cold: dropped)
            for r in routes:
                if r is None:
                    tr.baked_render_subframe(bake, 1, out=False, direct=True)
                else:
                    tr.baked_render_hybrid_subframe(bake, r, 1, out=False)
                if rep:
                    gpu[r].append(tr.baked_render_time())
        table = {"grid": [g, g, g, a.azimuths, a.cosines], "samples": ti["samples"], "paths": ti["paths"], "trace_ms": ti["trace_ms"],
                 "active_share": sp["active_nodes"] / sp["nodes"], "table_bytes": st["table_bytes"]}
        for r in routes:
            tr.reset()
            if r is None:
                tr.baked_render_accumulate(bake, 1, S, direct=True)
            else:
                tr.baked_render_hybrid_accumulate(bake, r, 1, S)
            print(json.dumps({"route": "ct_baked_render_subframe" if r is None else "ct_baked_render_hybrid_subframe", "depth": r, **common, **table,
                              "subframe_gpu_ms_lowest_median_highest": spread(gpu[r]), "repeats": a.repeats,
                              "relative_l2_against_the_long_mean": rel_l2(image(), long_a)}), flush=True)
        bake.close()
    tr.close()
