#!/usr/bin/env python3
"""What the MARCH kernel's fetches are made of on a benchmark scene (CT_STATS=1 build of the kernel): per sample,
the algorithm's lookups, the fetched steps, how many of those returned an all-zero footprint (and with which
clearance), the shadow-volume fetches and the reused ones.  python tools/march_stats.py <volume> <size> <spp>"""
import os, sys, json
from pathlib import Path
os.environ.setdefault("CT_STATS", "1")
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch  # noqa: F401
import deepestscatter_amd as ds
n, size, spp = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
t = ds.CloudTracer(ds.make_procedural_cloud(n), width=size, height=size)
t.render_accumulate(1, 32)
s0, k0, f0 = t.debug_stats(), t.counters(), t.fetch_counters()
t.render_accumulate(33, spp)
s1, k1, f1 = t.debug_stats(), t.counters(), t.fetch_counters()
d = lambda a, b, k: b[k] - a[k]
paths = d(k0, k1, "paths")
out = {"volume": n, "size": size, "spp": spp, "memory": t.debug_memory(),
       "per_sample": {"density_lookups": d(k0, k1, "density_lookups") / paths, "fetched_steps": d(s0, s1, "fetched_steps") / paths,
                      "fetched_zero_footprints": d(s0, s1, "fetched_zero_cells") / paths,
                      "zero_footprints_with_clearance_0": d(s0, s1, "zero_cells_nonfree_brick") / paths,
                      "zero_footprints_with_clearance_1": d(s0, s1, "zero_cells_free_brick_d1") / paths,
                      "skipped_steps": d(s0, s1, "skipped_steps") / paths,
                      # the free-space replay: skips of at least one step, the burst steps in which a lane replayed adds, and
                      # what the waves paid (replay blocks of at most CT_MARCH_REPLAY_MAX adds; the key keeps its name from the
                      # former replay loop, whose iterations it counted)
                      "free_space_skips": d(s0, s1, "free_space_skips") / paths,
                      "replay_lane_steps": d(s0, s1, "replay_lane_steps") / paths,
                      "skip_loop_wave_iterations": d(s0, s1, "skip_loop_wave_iterations") / paths,
                      "inscatter_lookups": d(k0, k1, "inscatter_lookups") / paths, "inscatter_fetches": d(f0, f1, "inscatter_fetches") / paths,
                      "march_phase_lanes": d(s0, s1, "march_lanes") / max(d(s0, s1, "march_phases"), 1),
                      "scatter_phase_lanes": d(s0, s1, "scatter_lanes") / max(d(s0, s1, "scatter_phases"), 1)},
       "per_march_burst_step": {"skip_loop_wave_iterations": d(s0, s1, "skip_loop_wave_iterations") / max(d(s0, s1, "march_phases"), 1)},
       "march_burst_steps_per_sample": d(s0, s1, "march_phases") / paths,
       # the schedule's mix per listed path (through pixels never reach the kernel): what the scheduler's rules are fitted to
       "schedule_mix": {"scheduler_visits_per_sample": d(s0, s1, "scheduler_visits") / paths,
                        "idle_lanes_per_scheduler_visit": d(s0, s1, "idle_lanes_at_visits") / max(d(s0, s1, "scheduler_visits"), 1),
                        "regen_phases_per_sample": d(s0, s1, "regen_phases") / paths,
                        "lanes_per_regen_phase": d(s0, s1, "regen_lanes") / max(d(s0, s1, "regen_phases"), 1),
                        "scatter_phases_per_sample": d(s0, s1, "scatter_phases") / paths,
                        "burst_steps_per_burst": d(s0, s1, "march_phases") / max(d(s0, s1, "march_bursts"), 1),
                        "bursts_ended_by": {k: (s1["bursts_ended_by"][k] - s0["bursts_ended_by"][k]) / max(d(s0, s1, "march_bursts"), 1)
                                            for k in s1["bursts_ended_by"]},
                        "replay_lane_steps_per_sample": d(s0, s1, "replay_lane_steps") / paths,
                        # per LISTED path (a lane that a regeneration phase gave a sample): lane-steps and lane-phases
                        "listed_paths": d(s0, s1, "regen_lanes"),
                        "march_lane_steps_per_listed_path": d(s0, s1, "march_lanes") / max(d(s0, s1, "regen_lanes"), 1),
                        "scatter_lane_phases_per_listed_path": d(s0, s1, "scatter_lanes") / max(d(s0, s1, "regen_lanes"), 1),
                        "replay_lane_steps_per_listed_path": d(s0, s1, "replay_lane_steps") / max(d(s0, s1, "regen_lanes"), 1)}}
print(json.dumps(out, indent=1))
