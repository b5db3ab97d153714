#!/usr/bin/env python3
"""What rendering from a baked probe table (ct_network_bake, ct_baked_render_*) costs beside the network renderer, and what the
table's resolution costs in accuracy: f-7's scene (the 512^3 procedural cloud, 1024 x 1024, default pose) and a seeded random
ScatterNet(200, 1, 3), warm calls, medians.  Per grid (16^3, 32^3, 64^3, each x 16 azimuths x 8 polar nodes) one JSON line:
  the bake's gather and network GPU ms (CtBakeInfo) and its wall time, the table's size in bytes;
  the baked subframe's GPU ms (ct_debug_baked_render_time) and wall ms beside ct_network_render_subframe's stage sum and wall
  ms -- the two routes take turns in the same run;
  the relative L2 distance between the two routes' means after --subframes subframes, and the same distance relative to the
  network route's variation about its mean level over the lit pixels (--bias raises the output bias so that the seeded
  network's outputs, small and negative as they come, are positive: negative outputs render black on both routes).
--sparse: instead, what ct_network_bake_sparse saves.  Per grid the dense and the sparse bake take turns,
--repeats times each after one warm-up pair, and one JSON line carries the active-node share, and for both routes the medians of
mask_ms, the gather ms, the network ms and the bake's wall ms (with the dense repeats' spread), the baked subframe's GPU ms, and
whether the two routes' means after --subframes subframes are bit-identical (the tool exits with 1 if they are not).
--compact: instead, what ct_network_bake_compact stores and costs.  Per grid the dense, the sparse and the
compact bake take turns, --repeats times each after one warm-up round, and one JSON line carries the active-node share, and per
route the table's and the index's bytes, the medians of the bake's wall ms and of the baked subframe's GPU ms with their spread
over the repeats, and whether the three routes' means after --subframes subframes are bit-identical (exit 1 if not).  Then one
grid beyond the dense limit, --beyond^3 (128), compact only: the active share and the sizes, or -- should (active + 1) x azimuths x
cosines exceed 2^26 -- the library's CT_E_INVAL message.
--half: instead, what a binary16 table (ct_bake_half) costs and saves.  Per grid (default 64^3) one sparse
float32 bake and its half copy take turns, --repeats rounds of 16 subframes each after one warm-up round, and one JSON line
carries, for both: ct_debug_baked_render_time as lowest / median / highest, the table's bytes; the relative L2 of the half bake's
64-subframe mean to the float32 bake's, beside the distance between two float32 means of disjoint subframes (1 .. 64 against
65 .. 128: the noise floor); and the wall ms of ct_bake_save and ct_bake_load of each table (to --scratch, default the system's
temporary directory).
Needs a GPU.  No threshold: the table's resolution is the user's trade.
    python tools/baked_render_time.py [--repeats 5] [--volume 512] [--size 1024] [--subframes 16] [--grids 16 32 64]
                                      [--azimuths 16] [--cosines 8] [--direct] [--bias 1.0] [--sparse | --compact [--beyond 128] | --half [--scratch DIR]]"""
import argparse, json, statistics, sys, time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def wall_ms(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def sparse_against_dense(a, tr, net, common):
    """The --sparse protocol -> True when every grid's two means were bit-identical."""
    import numpy as np
    med = statistics.median
    same = True
    for g in a.grids:
        runs = {False: [], True: []}
        means = {}
        for i in range(a.repeats + 1):          # (the first pair is the warm-up)
            for sparse in (False, True):
                t0 = time.perf_counter()
                bake = tr.network_bake(net, (g, g, g), a.azimuths, a.cosines, sparse=sparse)
                wall = (time.perf_counter() - t0) * 1e3
                info, sp = bake.info, bake.sparse_info
                gpu = []
                for _ in range(3):
                    tr.baked_render_subframe(bake, 1, out=False, direct=a.direct)
                    gpu.append(tr.baked_render_time())
                if i == a.repeats:
                    tr.reset()
                    tr.baked_render_accumulate(bake, 1, a.subframes, direct=a.direct)
                    means[sparse] = tr.mean()
                bake.close()
                if i:
                    runs[sparse].append({"wall": wall, "gather": info["gather_ms"], "network": info["network_ms"], "mask": sp["mask_ms"],
                                         "subframe": med(gpu), "active": sp["active_nodes"], "nodes": sp["nodes"]})
        identical = bool(np.array_equal(means[False], means[True]))
        same = same and identical
        line = {"route": "ct_network_bake_sparse against ct_network_bake", **common, "grid": [g, g, g, a.azimuths, a.cosines],
                "nodes": runs[True][0]["nodes"], "active_nodes": runs[True][0]["active"],
                "active_share": runs[True][0]["active"] / runs[True][0]["nodes"], "subframes": a.subframes,
                "means_bit_identical": identical, "lit_pixels_of_the_mean": int((means[False][..., 0] > 0).sum())}
        for sparse, name in ((False, "dense"), (True, "sparse")):
            r = runs[sparse]
            line.update({f"{name}_mask_ms": med(v["mask"] for v in r), f"{name}_gather_ms": med(v["gather"] for v in r),
                         f"{name}_network_ms": med(v["network"] for v in r), f"{name}_bake_wall_ms": med(v["wall"] for v in r),
                         f"{name}_bake_wall_ms_min_max": [min(v["wall"] for v in r), max(v["wall"] for v in r)],
                         f"{name}_baked_subframe_gpu_ms": med(v["subframe"] for v in r)})
        print(json.dumps(line), flush=True)
    return same


ROUTES = (("dense", {}), ("sparse", {"sparse": True}), ("compact", {"compact": True}))


def compact_against_the_others(a, tr, net, common):
    """The --compact protocol -> True when every grid's three means were bit-identical."""
    import numpy as np
    from deepestscatter_amd import _lib
    med = statistics.median
    same = True
    for g in a.grids:
        runs = {name: [] for name, _ in ROUTES}
        means = {}
        for i in range(a.repeats + 1):          # (the first round is the warm-up)
            for name, kw in ROUTES:
                t0 = time.perf_counter()
                bake = tr.network_bake(net, (g, g, g), a.azimuths, a.cosines, **kw)
                wall = (time.perf_counter() - t0) * 1e3
                sp, st = bake.sparse_info, bake.storage_info
                gpu = []
                for _ in range(6):              # (the first subframe of a fresh table reads it cold)
                    tr.baked_render_subframe(bake, 1, out=False, direct=a.direct)
                    gpu.append(tr.baked_render_time())
                if i == a.repeats:
                    tr.reset()
                    tr.baked_render_accumulate(bake, 1, a.subframes, direct=a.direct)
                    means[name] = tr.mean()
                bake.close()
                if i:
                    runs[name].append({"wall": wall, "subframe": med(gpu[1:]), "first_subframe": gpu[0], "active": sp["active_nodes"],
                                       "nodes": sp["nodes"], "table_bytes": st["table_bytes"], "index_bytes": st["index_bytes"]})
        identical = all(bool(np.array_equal(means["dense"].view(np.uint32), means[name].view(np.uint32))) for name in ("sparse", "compact"))
        same = same and identical
        line = {"route": "ct_network_bake_compact against ct_network_bake_sparse and ct_network_bake", **common,
                "grid": [g, g, g, a.azimuths, a.cosines], "nodes": runs["compact"][0]["nodes"], "active_nodes": runs["compact"][0]["active"],
                "active_share": runs["compact"][0]["active"] / runs["compact"][0]["nodes"], "subframes": a.subframes,
                "means_bit_identical": identical, "lit_pixels_of_the_mean": int((means["dense"][..., 0] > 0).sum())}
        for name, _ in ROUTES:
            r = runs[name]
            line.update({f"{name}_table_bytes": r[0]["table_bytes"], f"{name}_index_bytes": r[0]["index_bytes"],
                         f"{name}_bake_wall_ms": med(v["wall"] for v in r),
                         f"{name}_bake_wall_ms_min_max": [min(v["wall"] for v in r), max(v["wall"] for v in r)],
                         f"{name}_baked_subframe_gpu_ms": med(v["subframe"] for v in r),
                         f"{name}_baked_subframe_gpu_ms_min_max": [min(v["subframe"] for v in r), max(v["subframe"] for v in r)],
                         f"{name}_first_subframe_gpu_ms": med(v["first_subframe"] for v in r)})
        print(json.dumps(line), flush=True)
    # one grid beyond the dense limit, compact only
    g = a.beyond
    line = {"route": "ct_network_bake_compact beyond the dense limit", **common, "grid": [g, g, g, a.azimuths, a.cosines],
            "virtual_entries": g ** 3 * a.azimuths * a.cosines, "stored_limit": 2 ** 26}
    _, nodes, active = tr.bake_mask((g, g, g))
    line.update({"nodes": int(nodes.size), "active_nodes": int(len(active)), "active_share": len(active) / nodes.size,
                 "stored_entries_needed": (len(active) + 1) * a.azimuths * a.cosines})
    try:
        t0 = time.perf_counter()
        bake = tr.network_bake(net, (g, g, g), a.azimuths, a.cosines, compact=True)
        line["bake_wall_ms"] = (time.perf_counter() - t0) * 1e3
        info, st = bake.info, bake.storage_info
        gpu = []
        for _ in range(6):
            tr.baked_render_subframe(bake, 1, out=False, direct=a.direct)
            gpu.append(tr.baked_render_time())
        line.update({"table_bytes": st["table_bytes"], "index_bytes": st["index_bytes"], "stored_entries": st["stored_entries"],
                     "bake_gather_ms": info["gather_ms"], "bake_network_ms": info["network_ms"],
                     "baked_subframe_gpu_ms": med(gpu[1:]), "first_subframe_gpu_ms": gpu[0]})
        bake.close()
    except _lib.CloudTraceError as e:
        line.update({"error_code": e.code, "error": e.message})
    print(json.dumps(line), flush=True)
    return same


def half_against_float(a, tr, net, common):
    """The --half protocol."""
    import os, tempfile
    import numpy as np
    grids = a.grids if a.grids != [16, 32, 64] else [64]
    for g in grids:
        src = tr.network_bake(net, (g, g, g), a.azimuths, a.cosines, sparse=True)
        half = src.half()
        routes = (("float32", src), ("half", half))
        gpu = {name: [] for name, _ in routes}
        for i in range(a.repeats + 1):          # (the first round is the warm-up)
            for name, bake in routes:
                for sid in range(1, 17):
                    tr.baked_render_subframe(bake, sid, out=False, direct=a.direct)
                    if i:
                        gpu[name].append(tr.baked_render_time())

        def rel(x, y):
            return float(np.sqrt(((x - y) ** 2).sum() / (y ** 2).sum()))

        # (a mean over subframes 65 .. 128 would fold onto a count of 64: both means are taken from a count of zero)
        tr.reset()
        tr.baked_render_accumulate(src, 1, 64, direct=a.direct)
        f_a = tr.mean()[..., :3].astype(np.float64)
        tr.reset()
        tr.baked_render_accumulate(half, 1, 64, direct=a.direct)
        h_a = tr.mean()[..., :3].astype(np.float64)
        tr.reset()
        tr.baked_render_accumulate(src, 1, 128, direct=a.direct)
        f_ab = tr.mean()[..., :3].astype(np.float64)
        f_b = 2.0 * f_ab - f_a                      # the mean of subframes 65 .. 128, from the two running means
        line = {"route": "ct_bake_half against its float32 bake", **common, "grid": [g, g, g, a.azimuths, a.cosines], "kind": "sparse",
                "active_share": src.sparse_info["active_nodes"] / src.sparse_info["nodes"], "subframes_timed": len(gpu["half"]),
                "relative_l2_half_mean_to_float32_mean_64_subframes": rel(h_a, f_a),
                "relative_l2_float32_subframes_65_128_to_1_64": rel(f_b, f_a)}
        with tempfile.TemporaryDirectory(dir=a.scratch) as d:
            for name, bake in routes:
                path = os.path.join(d, name + ".bake")
                save = wall_ms(lambda: bake.save(path))
                t0 = time.perf_counter()
                loaded = tr.load_bake(path)
                load = (time.perf_counter() - t0) * 1e3
                loaded.close()
                line.update({f"{name}_baked_subframe_gpu_ms_min_median_max": [min(gpu[name]), statistics.median(gpu[name]), max(gpu[name])],
                             f"{name}_table_bytes": bake.storage_info["table_bytes"], f"{name}_file_bytes": os.path.getsize(path),
                             f"{name}_save_wall_ms": save, f"{name}_load_wall_ms": load})
        print(json.dumps(line), flush=True)
        half.close()
        src.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--volume", type=int, default=512)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--subframes", type=int, default=16)
    ap.add_argument("--grids", type=int, nargs="+", default=[16, 32, 64])
    ap.add_argument("--azimuths", type=int, default=16)
    ap.add_argument("--cosines", type=int, default=8)
    ap.add_argument("--direct", action="store_true")
    ap.add_argument("--bias", type=float, default=1.0)
    ap.add_argument("--sparse", action="store_true")
    ap.add_argument("--compact", action="store_true")
    ap.add_argument("--beyond", type=int, default=128)
    ap.add_argument("--half", action="store_true")
    ap.add_argument("--scratch", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import deepestscatter_amd as ds
    from deepestscatter_amd import network as N
    tr = ds.CloudTracer(ds.make_procedural_cloud(a.volume), width=a.size, height=a.size)
    torch.manual_seed(1)
    module = N.ScatterNet(200, 1, 3)
    with torch.no_grad():
        module.out.bias += a.bias      # a random network's outputs are small and of one sign: negative ones render black
    net = N.Network(tr, module)
    med = statistics.median
    common = {"network": [200, 1, 3], "output_bias_raised_by": a.bias, "volume": a.volume, "frame": [a.size, a.size], "repeats": a.repeats,
              "direct": a.direct}

    if a.half:
        half_against_float(a, tr, net, common)
        net.close()
        tr.close()
        sys.exit(0)
    if a.sparse or a.compact:
        ok = compact_against_the_others(a, tr, net, common) if a.compact else sparse_against_dense(a, tr, net, common)
        net.close()
        tr.close()
        sys.exit(0 if ok else 1)

    # the network route's image, once
    tr.reset()
    tr.network_render_accumulate(net, 1, a.subframes, direct=a.direct)
    want = tr.mean()[..., :3].astype(np.float64)
    lit = want[..., 0] > 0
    level = want[lit].mean() if lit.any() else 0.0      # the image is nearly one level (a random network): the variation is what a table can get wrong
    common.update({"lit_pixels": int(lit.sum()), "network_route_mean_level": float(level),
                   "network_route_min_max": [float(want[lit].min()), float(want[lit].max())] if lit.any() else None})

    for g in a.grids:
        t0 = time.perf_counter()
        bake = tr.network_bake(net, (g, g, g), a.azimuths, a.cosines)
        bake_wall = (time.perf_counter() - t0) * 1e3
        info = bake.info
        baked_gpu, baked_wall, net_gpu, net_wall = [], [], [], []
        for i in range(a.repeats + 1):          # (the first pair is the warm-up)
            baked_wall.append(wall_ms(lambda: tr.baked_render_subframe(bake, 1, out=False, direct=a.direct)))
            baked_gpu.append(tr.baked_render_time())
            net_wall.append(wall_ms(lambda: tr.network_render_subframe(net, 1, out=False, direct=a.direct)))
            net_gpu.append(sum(tr.network_render_time()))
        tr.reset()
        acc_wall = wall_ms(lambda: tr.baked_render_accumulate(bake, 1, a.subframes, direct=a.direct))
        got = tr.mean()[..., :3].astype(np.float64)
        rel = float(np.sqrt(((got - want) ** 2).sum() / (want ** 2).sum())) if lit.any() else None
        var = ((want - level)[lit] ** 2).sum()
        rel_var = float(np.sqrt(((got - want)[lit] ** 2).sum() / var)) if lit.any() and var > 0 else None
        print(json.dumps({"route": "ct_baked_render_subframe", **common, "grid": [g, g, g, a.azimuths, a.cosines],
                          "entries": info["entries"], "table_bytes": 4 * info["entries"], "bake_gather_ms": info["gather_ms"],
                          "bake_network_ms": info["network_ms"], "bake_wall_ms": bake_wall,
                          "baked_gpu_ms": med(baked_gpu[1:]), "baked_wall_ms": med(baked_wall[1:]),
                          "network_route_gpu_ms": med(net_gpu[1:]), "network_route_wall_ms": med(net_wall[1:]),
                          "subframes": a.subframes, "baked_accumulate_wall_ms_per_subframe": acc_wall / a.subframes,
                          "relative_l2_of_the_means": rel,
                          "relative_l2_against_the_variation_about_the_mean_level": rel_var}), flush=True)
        bake.close()
    net.close()
    tr.close()
