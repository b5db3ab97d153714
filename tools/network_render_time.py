#!/usr/bin/env python3
"""What rendering with the scattering network costs and where the time goes: the flagship scene (the 512^3 procedural cloud,
1024 x 1024, default pose) and a seeded random ScatterNet(200, 1, 3), warm calls, medians.
  line 1  the four stage times of one ct_network_render_subframe (ct_debug_network_render_time: HIP events, summed over the
          bands) and its wall time;
  line 2  the wall time of ct_network_render_accumulate over 16 subframes against the unfused loop
          ct_network_render_subframe + ct_accumulate;
  line 3  the Python route of the same tree, CloudTracer.network_frame (descriptor_frame with its allocations, aux and the
          scatter as torch ops), per subframe.
--direct: what CT_NET_ADD_SINGLE_SCATTER costs.  Lines 1 and 2 are measured twice in the same run, the calls without and with
the flag taking turns, and printed twice ("direct": false, then true); line 1 also carries the smallest and largest
first-flight time of its repeats, the spread the difference has to be read against.
--shards N [N ...]: what N GPUs could reach, measured on one (as profiles/r03l measured strong scaling): instead of lines 2 and
3, the tile path (ct_network_render_shard_subframe) of the unsharded handle against the row path of line 1 -- an 8 x 8 wave
against a 64 x 1 one -- and then, for every N, each of the N shards rendered in turn on a handle of its own (records, the four
stage times, wall time) and the slowest shard against the row-path call of the same run: the speedup N GPUs could reach.
Needs a GPU.  Prints three JSON lines (five with --direct; with --shards 2 + sum(N) + len(N)).
    python tools/network_render_time.py [--repeats 5] [--volume 512] [--size 1024] [--subframes 16] [--band 0] [--direct]
                                        [--shards 2 4 8]"""
import argparse, json, statistics, sys, time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def wall_ms(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--volume", type=int, default=512)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--subframes", type=int, default=16)
    ap.add_argument("--band", type=int, default=0)
    ap.add_argument("--direct", action="store_true")
    ap.add_argument("--shards", type=int, nargs="+", default=[])
    a = ap.parse_args()
    import torch
    import deepestscatter_amd as ds
    from deepestscatter_amd import network as N
    tr = ds.CloudTracer(ds.make_procedural_cloud(a.volume), width=a.size, height=a.size)
    torch.manual_seed(1)
    net = N.Network(tr, N.ScatterNet(200, 1, 3))
    common = {"network": [200, 1, 3], "volume": a.volume, "frame": [a.size, a.size], "band_pixels": a.band, "repeats": a.repeats}
    med = statistics.median

    # one subframe: stages and wall time (the first call allocates the scratch and builds the pyramid: warm-up)
    flags = [False, True] if a.direct else [False]
    stages, wall = {f: [] for f in flags}, {f: [] for f in flags}
    for i in range(a.repeats + 1):
        for f in flags:
            wall[f].append(wall_ms(lambda: tr.network_render_subframe(net, 1, band_pixels=a.band, out=False, direct=f)))
            stages[f].append(tr.network_render_time())
    records = int(tr.descriptor_frame(1)[3].shape[0])
    names = ["flights_and_compaction_ms", "gather_ms", "network_ms", "aux_and_compose_ms"]
    for f in flags:
        line = {"route": "ct_network_render_subframe", **common, "records": records, "wall_ms": med(wall[f][1:])}
        line.update({n: med([s[k] for s in stages[f][1:]]) for k, n in enumerate(names)})
        if a.direct:
            flights = [s[0] for s in stages[f][1:]]
            line.update({"direct": f, "flights_and_compaction_ms_min": min(flights), "flights_and_compaction_ms_max": max(flights)})
        print(json.dumps(line), flush=True)

    if a.shards:
        direct = a.direct
        row = {n: med([s[k] for s in stages[direct][1:]]) for k, n in enumerate(names)}
        row_wall = med(wall[direct][1:])
        pixels = tr.descriptor_frame(1)[3].cpu().numpy()

        def shard_call(t, n):
            """-> (median wall ms, median stage times) of warm ct_network_render_shard_subframe calls on tracer t"""
            w, st = [], []
            for i in range(a.repeats + 1):
                w.append(wall_ms(lambda: t.network_render_shard_subframe(n, 1, band_pixels=a.band, out=False, direct=direct)))
                st.append(t.network_render_time())
            return med(w[1:]), {name: med([x[k] for x in st[1:]]) for k, name in enumerate(names)}

        tile_wall, tile = shard_call(tr, net)
        print(json.dumps({"route": "ct_network_render_shard_subframe", **common, "direct": direct, "shard": [0, 1], "records": records,
                          "wall_ms": tile_wall, **tile, "row_path_wall_ms": row_wall,
                          "row_path_flights_and_compaction_ms": row["flights_and_compaction_ms"], "row_path_gather_ms": row["gather_ms"],
                          "flights_tile_over_row": tile["flights_and_compaction_ms"] / row["flights_and_compaction_ms"],
                          "gather_tile_over_row": tile["gather_ms"] / row["gather_ms"]}), flush=True)
        net.close()
        tr.close()
        tex = ds.make_procedural_cloud(a.volume)
        for count in a.shards:
            slowest = 0.0
            for index in range(count):
                mask = ds.shard_mask(a.size, a.size, index, count).reshape(-1)
                with ds.CloudTracer(tex, width=a.size, height=a.size, shard_index=index, shard_count=count) as t:
                    torch.manual_seed(1)
                    with N.Network(t, N.ScatterNet(200, 1, 3)) as n:
                        w, st = shard_call(t, n)
                slowest = max(slowest, w)
                print(json.dumps({"route": "ct_network_render_shard_subframe", **common, "direct": direct, "shard": [index, count],
                                  "records": int(mask[pixels].sum()), "wall_ms": w, **st}), flush=True)
            print(json.dumps({"route": "shards", **common, "direct": direct, "shards": count, "slowest_shard_wall_ms": slowest,
                              "row_path_wall_ms": row_wall, "speedup_n_gpus_could_reach": row_wall / slowest}), flush=True)
        sys.exit(0)

    # S subframes: fused against the unfused loop
    S = a.subframes

    def unfused(f):
        for sid in range(1, S + 1):
            tr.network_render_subframe(net, sid, band_pixels=a.band, out=False, direct=f)
            tr.accumulate(sid)

    fused_ms, loop_ms = {f: [] for f in flags}, {f: [] for f in flags}
    for i in range(a.repeats + 1):
        for f in flags:
            tr.reset()
            fused_ms[f].append(wall_ms(lambda: tr.network_render_accumulate(net, 1, S, band_pixels=a.band, direct=f)))
            tr.reset()
            loop_ms[f].append(wall_ms(lambda: unfused(f)))
    for f in flags:
        line = {"route": "ct_network_render_accumulate", **common, "subframes": S, "fused_wall_ms": med(fused_ms[f][1:]),
                "unfused_loop_wall_ms": med(loop_ms[f][1:]), "fused_ms_per_subframe": med(fused_ms[f][1:]) / S,
                "unfused_ms_per_subframe": med(loop_ms[f][1:]) / S}
        if a.direct:
            line["direct"] = f
        print(json.dumps(line), flush=True)

    # the Python route: one float per pixel of one rect of at most 2^20 pixels
    py_ms = []
    if a.size * a.size <= 1 << 20:
        for i in range(a.repeats + 1):
            def route():
                tr.network_frame(net, 1)
                torch.cuda.synchronize()
            py_ms.append(wall_ms(route))
    print(json.dumps({"route": "CloudTracer.network_frame", **common, "records": records,
                      "wall_ms": med(py_ms[1:]) if py_ms else None,
                      "note": None if py_ms else "the frame exceeds the 2^20 pixels of one descriptor_frame rect"}), flush=True)
    net.close()
    tr.close()
