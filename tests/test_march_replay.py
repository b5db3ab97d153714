"""The MARCH kernel's bounded replay of the free-space skip (run with -m gpu on an MI355X).

A lane replays at most R = CT_MARCH_REPLAY_MAX skipped steps per burst step (R = 4, at least 1; the scene serves R = 8 as well) and
carries the rest of a longer skip to its next burst steps, where it neither steps nor fetches until the skip is done.  A
path's position adds stay the same adds in the same order, so nothing may change by a bit: every case renders with the
product kernel and with the diagnostics kernel (CT_STATS=1, CT_DEBUG_INVARIANTS=1) and holds mean, M2 and the counters of
both against the oracle.

The scene is a 48^3 volume of a few dense blocks with empty gaps of 3, 8, 9, 16, 17 and 40 texels between them, marched at
one texel per step (sample_step = 1/48).  A skip is floor((c - 1/32) / a) steps for a clearance of c texels and a largest
per-axis advance of a in (0.577, 1] texels per step, and the clearances between the blocks run from 1 to about 20: skips of
0 steps (c = 1, a near 1), of fewer than R, of exactly R, of R + 1, of 2 R and of several times R all occur among the
thousands of flights that leave a block in a random direction.  A block is two texels thick and of moderate density (about
one in seven of the flights that enter one crosses it), so the primary flights too go on from gap to gap: mode 2 has no others.
"""
import numpy as np
import pytest

import _oracle as O
import deepestscatter_amd as ds
from deepestscatter_amd import _lib

pytestmark = pytest.mark.gpu

N = 48
SCENE = dict(cloud_size_m=1500.0, sample_step=1.0 / N)
ORACLE_KEYS = ("mode", "cloud_size_m", "sample_step", "max_depth", "light_direction")
CAMERA = ((2.5, -0.4, 0.15), (0.0, 0.0, 0.0))      # looks down the rows of blocks, through the gaps between them
FOV = 28.0
_REF = {}


def gap_volume() -> np.ndarray:
    """uint8 [Z, Y, X]: three rows of blocks along x; the gaps between a row's blocks are the test's skip lengths."""
    tex = np.zeros((N, N, N), np.uint8)

    def row(z, y, starts, length=2):
        for x in starts:
            tex[z[0]:z[1], y[0]:y[1], x:x + length] = 80

    row((19, 29), (19, 29), (1, 6, 16, 27, 45))      # gaps of 3, 8, 9 and 16 texels
    row((2, 10), (2, 10), (2, 44))                   # a gap of 40
    row((38, 46), (38, 46), (3, 22, 41))             # two gaps of 17
    tex.setflags(write=False)
    return tex


TEX = gap_volume()


def pose(w, h):
    eye, lookat = CAMERA
    return (eye,) + tuple(ds.calculate_camera_variables(eye, lookat, (0, 1, 0), FOV, w / h))


def reference(w, h, spp, f8=False, **kw):
    """(mean, M2, counters) of the oracle: computed once per frame size and mode, shared, never modified."""
    key = repr((w, h, spp, f8, sorted(kw.items())))
    if key not in _REF:
        orc = O.Oracle(TEX, w, h, fast="fixed8" if f8 else True, **{k: v for k, v in {**SCENE, **kw}.items() if k in ORACLE_KEYS})
        orc.set_camera(*pose(w, h))
        mean, m2 = orc.render(spp)
        for a in (mean, m2):
            a.setflags(write=False)
        _REF[key] = (mean, m2, orc.counters.as_dict())
    return _REF[key]


def handles(monkeypatch, w, h, env=None, **kw):
    """The product kernel's handle and the diagnostics kernel's (statistics and invariants armed), created under `env`."""
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    tr = ds.CloudTracer(TEX, width=w, height=h, **SCENE, **kw)
    monkeypatch.setenv("CT_STATS", "1")
    monkeypatch.setenv("CT_DEBUG_INVARIANTS", "1")
    st = ds.CloudTracer(TEX, width=w, height=h, **SCENE, **kw)
    for k in ["CT_STATS", "CT_DEBUG_INVARIANTS"] + list(env or {}):
        monkeypatch.delenv(k)
    for t in (tr, st):
        t.set_camera(*pose(w, h))
    return tr, st


def check(tr, st, ref, same_schedule=True):
    mean, m2, counters = ref
    for t in (tr, st):
        assert np.array_equal(t.mean(), mean)
        assert np.array_equal(t.m2(), m2)
        assert t.counters() == counters
    # (how many shadow-volume footprints a lane could reuse depends on the order of its paths: equal only where the schedule is)
    for k in ("density_fetches",) + (("inscatter_fetches",) if same_schedule else ()):
        assert tr.fetch_counters()[k] == st.fetch_counters()[k], k
    iv = st.debug_invariants()
    assert iv["armed"] == 1 and iv["violations"] == 0 and iv["samples_without_alpha_1"] == 0, iv


def run_case(monkeypatch, w=64, h=64, spp=8, env=None, f8=False, flags=0, **kw):
    """One frame on both kernels against the oracle -> (fetch counters, the diagnostics kernel's statistics)."""
    tr, st = handles(monkeypatch, w, h, env=env, flags=flags | (_lib.CT_FLAG_TEX_FIXED8 if f8 else 0), **kw)
    for t in (tr, st):
        t.render_accumulate(1, spp)
    check(tr, st, reference(w, h, spp, f8=f8, **kw))
    fetch, stats = tr.fetch_counters(), st.debug_stats()
    tr.close()
    st.close()
    return fetch, stats


# ---- 1. skips of every length ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [0, 1, 2])
def test_skip_lengths(monkeypatch, mode):
    fetch, stats = run_case(monkeypatch, mode=mode)
    counters = reference(64, 64, 8, mode=mode)[2]
    # the oracle's paths cross the gaps: it looks up half as many steps again as the kernel fetches, at the least (the first
    # step of a flight, the steps inside and next to a block and the steps outside the rows' extents are always fetched)
    assert 2 * counters["density_lookups"] > 3 * stats["fetched_steps"] > 0
    assert fetch["density_fetches"] == stats["fetched_steps"]
    assert stats["skipped_steps"] > 0
    # some skip was spread over several burst steps, and some burst step replayed more than one add
    assert stats["skipped_steps"] > stats["replay_lane_steps"] > stats["free_space_skips"] > 0
    assert stats["skip_loop_wave_iterations"] > 0


# ---- 2. other schedules ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("env", [{"CT_MARCH_BURST": "1"},                                   # every burst ends with lanes in mid-skip
                                 {"CT_MARCH_BURST": "8", "CT_BURST_MARCH_MIN": "64"},
                                 {"CT_REGEN_MIN": "64"}], ids=lambda e: "-".join(f"{k[3:]}={v}" for k, v in e.items()))
def test_schedule_variations(monkeypatch, env):
    fetch, _ = run_case(monkeypatch, env=env)
    default, _ = run_case(monkeypatch)
    assert fetch["density_fetches"] == default["density_fetches"]


# ---- 3. the kernel's other instantiations ------------------------------------------------------------------------------------

def test_sparse_bricks(monkeypatch):
    run_case(monkeypatch, flags=_lib.CT_FLAG_SPARSE_BRICKS)


def test_fixed8_filter(monkeypatch):
    run_case(monkeypatch, f8=True)


def test_wide_offsets(monkeypatch):
    wide, _ = run_case(monkeypatch, env={"CT_WIDE_OFFSETS": "1"})
    narrow, _ = run_case(monkeypatch)
    assert wide == narrow


# ---- 4. paths suspended in mid-skip ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_age", ["1", "3"])
def test_suspension_in_mid_skip(monkeypatch, max_age):
    w = h = 96
    tr, st = handles(monkeypatch, w, h, env={"CT_MAX_AGE": max_age})
    for t in (tr, st):
        for k in range(6):
            t.render_accumulate_async(1 + 2 * k, 2)
        t.synchronize()
    with ds.CloudTracer(TEX, width=w, height=h, **SCENE) as waited:
        waited.set_camera(*pose(w, h))
        waited.render_accumulate(1, 12)
        for t in (tr, st):
            assert np.array_equal(t.mean(), waited.mean()) and np.array_equal(t.m2(), waited.m2())
            assert t.counters() == waited.counters()
            assert t.fetch_counters()["density_fetches"] == waited.fetch_counters()["density_fetches"]
    check(tr, st, reference(w, h, 12), same_schedule=False)
    iv = st.debug_invariants()
    assert iv["resumed"] == iv["suspended"] == st.debug_suspended() > 0, iv
    assert tr.debug_suspended() > 0
    tr.close()
    st.close()


# ---- 5. the dataset entry point ----------------------------------------------------------------------------------------------

def test_point_radiance_launch(monkeypatch):
    rng = np.random.default_rng(11)
    pos = (rng.random((256, 3), dtype=np.float32) - 0.5) * 0.9
    d = rng.normal(size=(256, 3)).astype(np.float32)
    orc = O.Oracle(TEX, 16, 16, fast=True, **SCENE)
    want = orc.point_radiance_launch(ds.make_point_tasks(pos, d), 1, 4)
    tr, st = handles(monkeypatch, 16, 16)
    for t in (tr, st):
        got = t.point_radiance_launch(ds.make_point_tasks(pos, d), 1, 4)
        assert got.tobytes() == want.tobytes()
        c, o = t.counters(), orc.counters.as_dict()      # (point launches count no image paths: the algorithm's tallies)
        for k in ("density_lookups", "scatter_events", "depth_capped"):
            assert c[k] == o[k], k
    assert st.debug_stats()["skipped_steps"] > 0
    tr.close()
    st.close()
