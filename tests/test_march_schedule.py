"""The MARCH kernel's schedule after its refit to a pixel list without through pixels (run with -m gpu on an MI355X).

What changed is when a wave does what: it refills at 4 idle lanes instead of 8, a march burst no longer ends for idle lanes,
and the wave raises its issue priority while it computes a load's address and issues the load (march step, scatter phase,
start records).  None of that may change a result by a bit, so every test holds mean, M2 and the counters against the oracle:
the new schedule in the three modes, the old thresholds and the extremes of every threshold's range (set through the CT_* knobs)
against the default run, a launch enqueued in three pieces with continuation against one waited-for launch, and the sparse-bricks
and CT_FLAG_TEX_FIXED8 instantiations, which carry the priority ranges too.

Shapes: a 32^3 and a 48^3 procedural cloud, a 64 x 64 frame (64 pixel groups: more than one wave, several jobs per wave), 4 and
17 subframes (17: a job list of an odd length, and enough samples for paths to be suspended between the pieces).

What "default" means at these shapes.  A launch this short (subframes x box-hitting pixels < 4e7: ct_api.cpp, short_batch) refills
at 16 idle lanes, not at the handle's regen_min, unless CT_REGEN_MIN is set.  So a handle created with no knob runs the priority
ranges and the burst rules of this change but NOT its refill at 4; that is what a whole-frame launch of a thousand subframes
gets, which is no test shape.  Every case therefore runs twice: with no knob (REFILL "short-batch"), and with CT_REGEN_MIN=4
(REFILL "4"), which switches the short batch's override off and gives the kernel the new threshold itself.

Not here: the CPU-only test that ct_create refuses out-of-range values of the knob whose default changed.  There is no refusal
to assert: knob_int (ct_handle.hpp) clamps a value into its range, and ct_create opens the device before it reads a knob, so
nothing about knobs can be observed without a GPU.  In its place CT_REGEN_MIN = 0 and 1000 are rendered below (clamped to 1 and
64) and must change nothing.
"""
import numpy as np
import pytest

import _oracle as O
import deepestscatter_amd as ds
from deepestscatter_amd import _lib

W = H = 64
VOLUMES = (32, 48)
SUBFRAMES = (4, 17)
_TEX = {}
_REF = {}
_DEFAULT = {}


def tex(n):
    if n not in _TEX:
        t = ds.make_procedural_cloud(n)
        t.setflags(write=False)
        _TEX[n] = t
    return _TEX[n]


def reference(n, spp, mode=0, f8=False):
    """(mean, M2, counters) of the oracle: computed once per case, shared, never modified."""
    key = (n, spp, mode, f8)
    if key not in _REF:
        orc = O.Oracle(tex(n), W, H, mode=mode, fast="fixed8" if f8 else True)
        mean, m2 = orc.render(spp)
        for a in (mean, m2):
            a.setflags(write=False)
        _REF[key] = (mean, m2, orc.counters.as_dict())
    return _REF[key]


REFILLS = {"short-batch": {}, "4": {"CT_REGEN_MIN": "4"}}
refill_cases = pytest.mark.parametrize("refill", list(REFILLS), ids=lambda r: "refill-" + r)


def tracer(monkeypatch, n, env=None, **kw):
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    t = ds.CloudTracer(tex(n), width=W, height=H, **kw)   # (the knobs are read once, at ct_create)
    for k in (env or {}):
        monkeypatch.delenv(k)
    return t


def result(t):
    return t.mean(), t.m2(), t.counters(), t.fetch_counters()["density_fetches"]


def default_run(monkeypatch, n, spp):
    """The default schedule's frame, counters and march fetches for (n, spp), mode 0: rendered once, held to the oracle once."""
    if (n, spp) not in _DEFAULT:
        t = tracer(monkeypatch, n)
        t.render_accumulate(1, spp)
        mean, m2, counters, fetches = result(t)
        t.close()
        ref = reference(n, spp)
        assert np.array_equal(mean, ref[0]) and np.array_equal(m2, ref[1]) and counters == ref[2]
        _DEFAULT[(n, spp)] = (mean, m2, counters, fetches)
    return _DEFAULT[(n, spp)]


def assert_same(got, want):
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1], want[1])
    assert got[2] == want[2]
    assert got[3] == want[3]     # density_fetches: the schedule does not change what a path fetches


# ---- 1. the new schedule ------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@refill_cases
@pytest.mark.parametrize("spp", SUBFRAMES)
@pytest.mark.parametrize("n", VOLUMES)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_new_schedule_equals_the_oracle(monkeypatch, mode, n, spp, refill):
    t = tracer(monkeypatch, n, env=REFILLS[refill], mode=mode)
    t.render_accumulate(1, spp)
    mean, m2, counters = reference(n, spp, mode=mode)
    assert np.array_equal(t.mean(), mean)
    assert np.array_equal(t.m2(), m2)
    assert t.counters() == counters
    assert counters["paths"] > 0 and counters["scatter_events"] > 0
    t.close()


# ---- 2. the thresholds change the schedule only ------------------------------------------------------------------------------------

# The new refill threshold, alone and with the extremes of the burst thresholds; the defaults before the refit; then both ends of the
# legal range of every threshold the refit looked at.  CT_BURST_IDLE is read by the DELTA kernel only since the MARCH kernel lost
# that rule; setting it must change nothing here.  The last two lie outside the range and are clamped into it.
SETTINGS = [
    {"CT_REGEN_MIN": "4"},
    {"CT_REGEN_MIN": "4", "CT_BURST_SCATTER": "1"}, {"CT_REGEN_MIN": "4", "CT_BURST_SCATTER": "64"},
    {"CT_REGEN_MIN": "4", "CT_MARCH_BURST": "1"}, {"CT_REGEN_MIN": "4", "CT_BURST_MARCH_MIN": "64"},
    {"CT_REGEN_MIN": "8", "CT_BURST_IDLE": "32"},
    {"CT_REGEN_MIN": "1"}, {"CT_REGEN_MIN": "64"},
    {"CT_BURST_SCATTER": "1"}, {"CT_BURST_SCATTER": "64"},
    {"CT_BURST_IDLE": "1"}, {"CT_BURST_IDLE": "64"},
    {"CT_BURST_MARCH_MIN": "1"}, {"CT_BURST_MARCH_MIN": "64"},
    {"CT_MARCH_BURST": "1"},
    {"CT_REGEN_MIN": "8", "CT_MARCH_BURST": "4", "CT_BURST_SCATTER": "34"},
    {"CT_REGEN_MIN": "0"}, {"CT_REGEN_MIN": "1000"},
]


@pytest.mark.gpu
@pytest.mark.parametrize("env", SETTINGS, ids=lambda e: "-".join(f"{k[3:]}={v}" for k, v in e.items()))
def test_thresholds_change_the_schedule_only(monkeypatch, env):
    for n, spp in ((48, 17), (32, 4)):
        t = tracer(monkeypatch, n, env=env)
        t.render_accumulate(1, spp)
        assert_same(result(t), default_run(monkeypatch, n, spp))
        t.close()


# ---- 3. continuation: three enqueued pieces against one waited-for launch ----------------------------------------------------------

@pytest.mark.gpu
@refill_cases
@pytest.mark.parametrize("n", VOLUMES)
@pytest.mark.parametrize("pieces", [(2, 1, 1), (6, 6, 5)], ids=lambda p: "+".join(map(str, p)))
def test_three_enqueued_pieces_equal_one_launch(monkeypatch, pieces, n, refill):
    spp = sum(pieces)
    t = tracer(monkeypatch, n, env=REFILLS[refill])
    first = 1
    for k in pieces:
        t.render_accumulate_async(first, k)
        first += k
    t.synchronize()
    print("suspended paths", t.debug_suspended())
    assert t.debug_suspended() > 0     # (the pieces did hand paths on: the suspend and resume blocks ran)
    assert_same(result(t), default_run(monkeypatch, n, spp))
    t.close()


# ---- 4. the kernel's other instantiations ------------------------------------------------------------------------------------------

@pytest.mark.gpu
@refill_cases
@pytest.mark.parametrize("spp", SUBFRAMES)
@pytest.mark.parametrize("n", VOLUMES)
def test_sparse_bricks_under_the_new_schedule(monkeypatch, n, spp, refill):
    t = tracer(monkeypatch, n, env={"CT_SPARSE": "1", **REFILLS[refill]})
    assert t.march_meta()["sparse"]
    t.render_accumulate(1, spp)
    assert_same(result(t)[:3] + (0,), reference(n, spp) + (0,))
    t.close()


@pytest.mark.gpu
@refill_cases
@pytest.mark.parametrize("spp", SUBFRAMES)
@pytest.mark.parametrize("n", VOLUMES)
def test_fixed8_filter_under_the_new_schedule(monkeypatch, n, spp, refill):
    t = tracer(monkeypatch, n, env=REFILLS[refill], flags=_lib.CT_FLAG_TEX_FIXED8)
    t.render_accumulate(1, spp)
    assert_same(result(t)[:3] + (0,), reference(n, spp, f8=True) + (0,))
    t.close()


# ---- 5. the diagnostics kernel and the mix it reports ---------------------------------------------------------------------------------

@pytest.mark.gpu
@refill_cases
def test_diagnostics_kernel_counts_every_burst_end(monkeypatch, refill):
    """The CT_STATS=1 kernel under the same schedule: the same frame, and every march burst ended by exactly one of the rules
    it reports (tools/march_stats.py divides by these).  (The printed regeneration figures show the two refill thresholds at
    work; they are not asserted: a job's last samples may be fewer than the idle lanes, at either threshold.)"""
    n, spp = 48, 17
    t = tracer(monkeypatch, n, env={"CT_STATS": "1", **REFILLS[refill]})
    t.render_accumulate(1, spp)
    assert_same(result(t), default_run(monkeypatch, n, spp))
    s = t.debug_stats()
    print({k: s[k] for k in ("scheduler_visits", "idle_lanes_at_visits", "march_bursts", "bursts_ended_by", "regen_phases", "regen_lanes")})
    assert s["march_bursts"] > 0 and sum(s["bursts_ended_by"].values()) == s["march_bursts"]
    assert s["scheduler_visits"] >= s["march_bursts"] and s["idle_lanes_at_visits"] <= 64 * s["scheduler_visits"]
    assert s["march_phases"] >= s["march_bursts"]
    t.close()
