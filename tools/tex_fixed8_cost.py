#!/usr/bin/env python3
"""What CT_FLAG_TEX_FIXED8 costs: the headline configuration (BASELINE.json configs[2]: 512^3 procedural density, 1024^2,
1024 spp per step, the steady state of bench.py) with the flag off and on, for the MARCH and the DELTA estimator.  One process,
one handle per (estimator, flag); the two handles of an estimator take their steps alternately, so both see the same machine,
and every step is timed on its own (host clock around the enqueued batch and the synchronize).
    python tools/tex_fixed8_cost.py [--repeats 7] [--spp 1024] [--volume 512] [--size 1024]
Prints one JSON line: per estimator and flag the Msamples/s of every step, their median, min and max, and the median ratio."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--spp", type=int, default=1024)
    ap.add_argument("--volume", type=int, default=512)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--estimators", default="0,1")
    a = ap.parse_args()
    try:
        import torch  # noqa: F401  (first, like bench.py: see tests/conftest.py)
    except Exception:
        pass
    import deepestscatter_amd as ds
    from deepestscatter_amd import _lib

    tex = ds.make_procedural_cloud(a.volume)
    W = H = a.size
    out = {"config": {"volume": a.volume, "width": W, "height": H, "spp_per_step": a.spp, "repeats": a.repeats}}
    for est in (int(e) for e in a.estimators.split(",")):
        name = "MARCH" if est == 0 else "DELTA"
        handles = {f: ds.CloudTracer(tex, width=W, height=H, estimator=est, flags=f) for f in (0, _lib.CT_FLAG_TEX_FIXED8)}
        nxt = {}
        for f, t in handles.items():   # warm-up: code objects, scratch, the cost-measuring launch and the tuned job order
            t.render_accumulate_async(1, a.spp)
            t.synchronize()
            nxt[f] = 1 + a.spp
        rates = {f: [] for f in handles}
        for r in range(a.repeats):
            order = list(handles) if r % 2 == 0 else list(handles)[::-1]
            for f in order:
                t = handles[f]
                t0 = time.perf_counter()
                t.render_accumulate_async(nxt[f], a.spp)
                t.synchronize()
                dt = time.perf_counter() - t0
                nxt[f] += a.spp
                rates[f].append(W * H * a.spp / dt / 1e6)
        res = {}
        for f, v in rates.items():
            res["fixed8" if f else "exact"] = {"msamples_per_s": [round(x, 1) for x in v], "median": round(statistics.median(v), 1),
                                               "min": round(min(v), 1), "max": round(max(v), 1)}
        res["fixed8_over_exact"] = round(res["fixed8"]["median"] / res["exact"]["median"], 4)
        res["checksums"] = {("fixed8" if f else "exact"): float(t.mean().astype("float64").sum()) for f, t in handles.items()}
        out[name] = res
        for t in handles.values():
            t.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
