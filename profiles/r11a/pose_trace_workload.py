"""Host phases of a new pose on the benchmark scene (512^3 cloud, 1024^2 frame, 1024 subframes per call) with CT_TRACE=1.
The workload of host_phases.txt.  Run from the repository root:
    CT_LIBRARY=<lib> python profiles/r11a/pose_trace_workload.py 2> trace.txt
(the library's trace goes to stderr)"""
import math
import os
import sys

os.environ["CT_TRACE"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import deepestscatter_amd as ds  # noqa: E402

W = H = 1024
tex = ds.make_procedural_cloud(512)
tr = ds.CloudTracer(tex, width=W, height=H, mode=0, estimator=0, device=0)
sys.stderr.write("## pose 0 (the handle's first)\n")
sys.stderr.flush()
tr.render_accumulate(1, 1024)
for k in range(1, 7):
    a = 0.35 * k
    eye, look = (0.5 + 1.9 * math.sin(a), 0.8, 0.5 - 1.9 * math.cos(a)), (0.5, 0.5, 0.5)
    sys.stderr.write(f"## pose {k}\n")
    sys.stderr.flush()
    tr.set_camera(eye, *ds.calculate_camera_variables(eye, look, (0, 1, 0), 45.0, W / H))
    tr.reset()
    tr.render_accumulate(1, 1024)
tr.close()
