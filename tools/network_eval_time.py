#!/usr/bin/env python3
"""What evaluating the scattering network on one frame's records costs: the whole-frame descriptor batch of the flagship scene
(the 512^3 procedural cloud, 1024 x 1024, default pose) through ct_network_eval with a seeded random ScatterNet(200, 1, 3) --
median of warm calls, timed with the library's HIP events (ct_debug_network_time) -- and, beside it, the same module run by
torch on the device from the same bytes in float32, in chunks of records that fit (torch events around the whole loop).
Needs a GPU.  Prints one JSON line.
    python tools/network_eval_time.py [--repeats 5] [--volume 512] [--size 1024] [--chunk 65536]"""
import argparse, json, statistics, sys
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--volume", type=int, default=512)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--chunk", type=int, default=65536)
    a = ap.parse_args()
    import torch
    import deepestscatter_amd as ds
    from deepestscatter_amd import network as N
    tr = ds.CloudTracer(ds.make_procedural_cloud(a.volume), width=a.size, height=a.size)
    torch.manual_seed(1)
    module = N.ScatterNet(200, 1, 3)
    net = N.Network(tr, module)
    desc, pos, view, pix = tr.descriptor_frame(1)
    n = len(pix)
    dev = desc.device
    aux = (view * torch.tensor(tr.light_direction(), device=dev)).sum(dim=1).contiguous()
    out = torch.empty((n,), dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    ms = []
    for i in range(a.repeats + 1):                           # (the first call is the warm-up)
        net.eval(desc.data_ptr(), aux.data_ptr(), n, out.data_ptr())
        ms.append(net.time_ms())
    fused = statistics.median(ms[1:])
    module = module.to(dev)
    ref = torch.empty_like(out)
    t_ms = []
    with torch.no_grad():
        for i in range(a.repeats + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for at in range(0, n, a.chunk):
                ref[at:at + a.chunk] = module(desc[at:at + a.chunk], aux[at:at + a.chunk, None])
            e1.record()
            torch.cuda.synchronize(dev)
            t_ms.append(e0.elapsed_time(e1))
    eager = statistics.median(t_ms[1:])
    macs = module.shape.macs()
    print(json.dumps({"route": "ct_network_eval", "network": [200, 1, 3], "volume": a.volume, "frame": [a.size, a.size], "records": n,
                      "network_eval_ms": fused, "records_per_s": n / (fused * 1e-3), "macs_per_record": macs,
                      "bf16_tflops": 2 * macs * n / (fused * 1e-3) / 1e12, "torch_float32_ms": eager, "torch_chunk": a.chunk,
                      "max_abs_difference_to_torch_float32": float((out - ref).abs().max()), "repeats": a.repeats}))
    net.close()
    tr.close()
