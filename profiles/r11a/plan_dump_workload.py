"""The workload of plan_dump_{parent,head}.txt: a library built with plan_dump.patch applied, a 32^3 procedural cloud on a
64 x 64 frame, two poses, both estimators, six settings.  Run from the repository root:
    CT_LIBRARY=<library with the patch> python profiles/r11a/plan_dump_workload.py 2> dump.txt
(the library's [plan] lines and this script's markers go to stderr)"""
import os
import sys

os.environ["CT_PLAN_DUMP"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import deepestscatter_amd as ds  # noqa: E402

W = H = 64
KNOBS = ["CT_XCD_QUEUES", "CT_XCD_REGIONS", "CT_SHARED_DEPTH", "CT_SCRATCH_MIB", "CT_CHUNK_INTERLEAVE", "CT_TILE_ORDER"]
CONFIGS = [
    ("defaults", {}, {}, (4, 17)),
    ("queues", {"CT_XCD_QUEUES": "1", "CT_XCD_REGIONS": "8", "CT_SHARED_DEPTH": "4"}, {}, (4, 17)),
    ("scratch1", {"CT_SCRATCH_MIB": "1"}, {}, (4, 17, 100)),
    ("scratch1_interleave", {"CT_SCRATCH_MIB": "1", "CT_CHUNK_INTERLEAVE": "1"}, {}, (4, 17, 100)),
    ("hilbert", {"CT_TILE_ORDER": "hilbert"}, {}, (4, 17)),
    ("shard1of3", {}, {"shard_index": 1, "shard_count": 3}, (4, 17)),
]


def mark(text):
    sys.stderr.write(f"[plan] ## {text}\n")
    sys.stderr.flush()


def calls(tr, counts):
    first = 1
    for n in counts:
        mark(f"render_accumulate({first}, {n})")
        tr.render_accumulate(first, n)
        first += n


tex = ds.make_procedural_cloud(32)
eye2, look2 = (1.7, 0.9, -0.8), (0.5, 0.5, 0.5)
pose2 = (eye2,) + tuple(ds.calculate_camera_variables(eye2, look2, (0, 1, 0), 50.0, W / H))
for est in (0, 1):
    for name, env, kw, counts in CONFIGS:
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(env)
        mark(f"config {name} estimator {est}")
        tr = ds.CloudTracer(tex, width=W, height=H, mode=0, estimator=est, device=0, **kw)
        calls(tr, counts)
        mark("second pose")
        tr.set_camera(*pose2)
        tr.reset()
        calls(tr, counts)
        tr.close()
mark("done")
