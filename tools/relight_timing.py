#!/usr/bin/env python3
"""What a new light costs: ct_create against ct_set_light on a procedural cloud, dense and sparse march bricks.  One JSON line:
  create_ms / create_sparse_ms        wall time of ct_create (a 32^3 handle is created first: runtime start-up is not measured)
  set_light_ms / set_light_sparse_ms  wall time of ct_set_light to a different direction: median of --repeats alternations
                                      between two lights, after one warm-up call
--create-only measures the first pair alone (a library without ct_set_light: the baseline of the commit before the verb);
--parent-create-ms A,B records that baseline's two figures beside the new ones, with the ratios against them.
    python tools/relight_timing.py [--volume 512] [--repeats 7]"""
import argparse, json, os, statistics, sys, time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--volume", type=int, default=512)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--create-only", action="store_true")
    ap.add_argument("--parent-create-ms", default="")
    a = ap.parse_args()
    import deepestscatter_amd as ds
    side, back = ds.LIGHT_DIRECTIONS["Side"], ds.LIGHT_DIRECTIONS["Back"]
    ds.CloudTracer(ds.make_procedural_cloud(32), width=32, height=32).close()
    tex = ds.make_procedural_cloud(a.volume)
    out = {"volume": a.volume, "frame": a.size, "repeats": a.repeats}
    for name, sparse in (("", "0"), ("_sparse", "1")):
        os.environ["CT_SPARSE"] = sparse
        t0 = time.perf_counter()
        tr = ds.CloudTracer(tex, width=a.size, height=a.size, light_direction=side)
        out["create" + name + "_ms"] = (time.perf_counter() - t0) * 1e3
        if not a.create_only:
            tr.set_light(back)                                        # warm-up
            ms = []
            for k in range(a.repeats):
                t0 = time.perf_counter()
                tr.set_light(side if k % 2 == 0 else back)
                ms.append((time.perf_counter() - t0) * 1e3)
            out["set_light" + name + "_ms"] = statistics.median(ms)
            out["set_light" + name + "_all_ms"] = [round(v, 3) for v in ms]
            out["inscatter_checksum" + name] = int(tr.inscatter().sum(dtype="uint64"))
        tr.close()
    if a.parent_create_ms:
        p = [float(v) for v in a.parent_create_ms.split(",")]
        out["parent_create_ms"], out["parent_create_sparse_ms"] = p[0], p[1]
        if not a.create_only:
            out["set_light_over_parent_create"] = out["set_light_ms"] / p[0]
            out["set_light_sparse_over_parent_create_sparse"] = out["set_light_sparse_ms"] / p[1]
    print(json.dumps(out))
