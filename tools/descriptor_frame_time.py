#!/usr/bin/env python3
"""What the network's input for one frame costs: warm whole-frame calls of ct_descriptor_frame on the flagship scene (the 512^3
procedural cloud, 1024 x 1024, default pose), split with the library's HIP events into the first flights with their compaction and
the descriptor gather -- and, beside it, the only route the library offered for the gather half before: ct_collect_descriptors
on the same positions through host arrays (2250 bytes per record over PCIe, two copies of the inputs the other way).
Needs a GPU.  Prints one JSON line per route.
    python tools/descriptor_frame_time.py [--repeats 5] [--volume 512] [--size 1024]"""
import argparse, json, statistics, sys, time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--volume", type=int, default=512)
    ap.add_argument("--size", type=int, default=1024)
    a = ap.parse_args()
    import torch  # noqa: F401  (before the library: both bring a HIP runtime, and torch needs its own)
    import deepestscatter_amd as ds
    tex = ds.make_procedural_cloud(a.volume)
    tr = ds.CloudTracer(tex, width=a.size, height=a.size)
    desc, pos, view, pix = tr.descriptor_frame(1)           # builds the mip pyramid, warms the allocators
    n = len(pix)
    scatter, gather, wall = [], [], []
    for i in range(a.repeats):
        t0 = time.perf_counter()
        got = tr.descriptor_frame(1, capacity=n)
        wall.append((time.perf_counter() - t0) * 1e3)
        s, g = tr.descriptor_frame_time()
        scatter.append(s)
        gather.append(g)
        assert len(got[3]) == n
    med = statistics.median
    print(json.dumps({"route": "ct_descriptor_frame", "volume": a.volume, "frame": [a.size, a.size], "records": n,
                      "first_scatter_and_compaction_ms": med(scatter), "gather_ms": med(gather), "call_wall_ms": med(wall),
                      "records_per_s": n / ((med(scatter) + med(gather)) * 1e-3),
                      "flight_share": med(scatter) / (med(scatter) + med(gather)), "repeats": a.repeats}))
    pos_h, view_h = pos.cpu().numpy(), view.cpu().numpy()
    del got
    host = []
    for i in range(max(1, a.repeats // 2) + 1):             # (the first call is the warm-up)
        t0 = time.perf_counter()
        d = tr.collect_descriptors(pos_h, view_h)
        host.append((time.perf_counter() - t0) * 1e3)
    same = bool((torch.from_numpy(d).to(desc.device) == desc).all())
    print(json.dumps({"route": "ct_collect_descriptors through host arrays (gather half only)", "records": n,
                      "call_wall_ms": med(host[1:]), "records_per_s": n / (med(host[1:]) * 1e-3), "same_bytes": same}))
    tr.close()
