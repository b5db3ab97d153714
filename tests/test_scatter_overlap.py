"""The MARCH kernel's scatter phase with its loads overlapped (run with -m gpu on an MI355X).

The scatter phase keeps the two loads of the NEE's shadow-volume footprint in flight until in_scattering_finish: the lane's
one-entry cache holds the footprint's raw words, which are combined after the new direction is sampled (the
cache of the combined footprint, which waited for the loads at once, was removed with its compile-time switch).
Only the order in which a wave issues and awaits its loads changes, so nothing may change by a bit: every case renders with
the product kernel and with the diagnostics kernel (CT_STATS=1, CT_DEBUG_INVARIANTS=1) and holds mean, M2 and the counters
of both against the oracle.

The scene is that of test_nee_skip.py: a thick 64^3 cloud of 20 km, where a wave's scatter phase has lanes of all three NEE
classes at once -- skipped (shadow-zero row), reused (the lane's cache holds the footprint) and fetched.
"""
import numpy as np
import pytest

import _oracle as O
import deepestscatter_amd as ds
from deepestscatter_amd import _lib

pytestmark = pytest.mark.gpu

W, H, SPP = 40, 32, 3
SCENE = dict(cloud_size_m=20000.0)
ORACLE_KEYS = ("mode", "cloud_size_m", "sample_step", "max_depth", "light_direction")
_REF = {}
_TEX = []


def tex():
    if not _TEX:
        t = ds.make_procedural_cloud(64)
        t.setflags(write=False)
        _TEX.append(t)
    return _TEX[0]


def reference(spp, f8=False, **kw):
    """(mean, M2, counters) of the oracle: computed once per case, shared, never modified."""
    key = repr((spp, f8, sorted(kw.items())))
    if key not in _REF:
        orc = O.Oracle(tex(), W, H, fast="fixed8" if f8 else True, **{k: v for k, v in {**SCENE, **kw}.items() if k in ORACLE_KEYS})
        mean, m2 = orc.render(spp)
        for a in (mean, m2):
            a.setflags(write=False)
        _REF[key] = (mean, m2, orc.counters.as_dict())
    return _REF[key]


def handles(monkeypatch, env=None, **kw):
    """The product kernel's handle and the diagnostics kernel's (statistics and invariants armed), created under `env`."""
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    tr = ds.CloudTracer(tex(), width=W, height=H, **SCENE, **kw)
    monkeypatch.setenv("CT_STATS", "1")
    monkeypatch.setenv("CT_DEBUG_INVARIANTS", "1")
    st = ds.CloudTracer(tex(), width=W, height=H, **SCENE, **kw)
    for k in ["CT_STATS", "CT_DEBUG_INVARIANTS"] + list(env or {}):
        monkeypatch.delenv(k)
    return tr, st


def check(tr, st, ref):
    mean, m2, counters = ref
    for t in (tr, st):
        assert np.array_equal(t.mean(), mean)
        assert np.array_equal(t.m2(), m2)
        assert t.counters() == counters
    iv = st.debug_invariants()
    assert iv["armed"] == 1 and iv["violations"] == 0 and iv["samples_without_alpha_1"] == 0, iv


def check_classes(st, several_events):
    """No case passes vacuously: lanes skipped their NEE, lanes reused their footprint, lanes fetched one."""
    stats, c, f = st.debug_stats(), st.counters(), st.fetch_counters()
    print({k: stats[k] for k in ("nee_lookups_skipped_shadow_zero", "nee_footprints_reused")}, c["inscatter_lookups"], f)
    assert stats["nee_lookups_skipped_shadow_zero"] > 0
    assert stats["nee_footprints_reused"] > 0
    # A skipped lookup counts as a reused footprint too.  An entry is really read again by the next event of the same path, a
    # mean free path further on, so wherever paths have several events (not in mode 2, not at max_depth = 2, where the first
    # event is the last) some of the reused ones must be cache hits.
    if several_events:
        assert stats["nee_footprints_reused"] > stats["nee_lookups_skipped_shadow_zero"]
    assert f["inscatter_fetches"] > 0
    assert f["inscatter_fetches"] == c["inscatter_lookups"] - stats["nee_footprints_reused"]


def run_case(monkeypatch, env=None, f8=False, flags=0, **kw):
    tr, st = handles(monkeypatch, env=env, flags=flags | (_lib.CT_FLAG_TEX_FIXED8 if f8 else 0), **kw)
    for t in (tr, st):
        t.render_accumulate(1, SPP)
    check(tr, st, reference(SPP, f8=f8, **kw))
    assert tr.fetch_counters() == st.fetch_counters()
    check_classes(st, several_events=kw.get("mode", 0) != 2 and kw.get("max_depth", 1000) > 2)
    mm = tr.march_meta()
    tr.close()
    st.close()
    return mm


# ---- 1. all three NEE classes in one wave --------------------------------------------------------------------------------------

@pytest.mark.parametrize("light", ["Front", "Side", "Back"])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_nee_classes(monkeypatch, mode, light):
    run_case(monkeypatch, mode=mode, light_direction=ds.LIGHT_DIRECTIONS[light])


# ---- 2. the kernel's other instantiations, and paths that end between the issue and the finish -------------------------------------

def test_fixed8_filter(monkeypatch):
    run_case(monkeypatch, f8=True)


def test_sparse_bricks(monkeypatch):
    assert run_case(monkeypatch, env={"CT_SPARSE": "1"})["sparse"]


def test_wide_offsets(monkeypatch):
    run_case(monkeypatch, env={"CT_WIDE_OFFSETS": "1"})


def test_depth_cap_between_issue_and_finish(monkeypatch):
    run_case(monkeypatch, max_depth=2)
    assert reference(SPP, max_depth=2)[2]["depth_capped"] > 0


# ---- 3. a cache entry outliving suspended paths ------------------------------------------------------------------------------------

def test_cache_entry_outlives_suspended_paths(monkeypatch):
    tr, st = handles(monkeypatch)
    for t in (tr, st):
        for k in range(12):
            t.render_accumulate_async(1 + k, 1)
        t.synchronize()
    waited = handles(monkeypatch)
    for t in waited:
        t.render_accumulate(1, 12)
    for t, v in zip((tr, st), waited):
        assert np.array_equal(t.mean(), v.mean()) and np.array_equal(t.m2(), v.m2())
        assert t.counters() == v.counters()
    check(tr, st, reference(12))
    check(*waited, reference(12))
    print("suspended", tr.debug_suspended(), st.debug_suspended())
    assert tr.debug_suspended() > 0 and st.debug_suspended() > 0
    iv = st.debug_invariants()
    assert iv["resumed"] == iv["suspended"] == st.debug_suspended(), iv
    for t in (tr, st) + tuple(waited):
        t.close()
