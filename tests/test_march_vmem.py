"""The MARCH kernel's vector-memory diet (run with -m gpu on an MI355X): both phase tables read from LDS, one start record per
slot of the pixel groups instead of the pixel / primary ray / prefix chain, 32-bit footprint offsets.

Each of the three moves a load to another address space, moves a per-pixel constant or re-expresses integer address
arithmetic, so nothing may change by a bit: every case renders with the product kernel and with the diagnostics kernel
(CT_STATS=1) and holds mean, M2 and the counters of both against the oracle, and the two kernels' fetch counters against
each other.  The cases are the places where one of the three could go wrong.
"""
import numpy as np
import pytest

import _oracle as O
import deepestscatter_amd as ds
from deepestscatter_amd import _lib

pytestmark = pytest.mark.gpu

F8 = _lib.CT_FLAG_TEX_FIXED8
SIZE_M = 20000.0
ORACLE_KEYS = ("mode", "cloud_size_m", "sample_step", "max_depth", "light_direction")
_CLOUD = {}
_REF = {}


def cloud(n=64):
    if n not in _CLOUD:
        _CLOUD[n] = ds.make_procedural_cloud(n)
        _CLOUD[n].setflags(write=False)
    return _CLOUD[n]


def pose(eye, lookat, w, h, fov=60.0):
    return (eye,) + tuple(ds.calculate_camera_variables(eye, lookat, (0, 1, 0), fov, w / h))


def reference(w, h, spp, camera=None, f8=False, **kw):
    """(mean, M2, counters) of the oracle for a frame: computed once per scene and pose, shared, never modified."""
    key = repr((w, h, spp, camera, f8, sorted(kw.items())))
    if key not in _REF:
        orc = O.Oracle(cloud(), w, h, fast="fixed8" if f8 else True, **{k: v for k, v in kw.items() if k in ORACLE_KEYS})
        if camera is not None:
            orc.set_camera(*pose(*camera, w, h))
        mean, m2 = orc.render(spp)
        for a in (mean, m2):
            a.setflags(write=False)
        _REF[key] = (mean, m2, orc.counters.as_dict())
    return _REF[key]


def handles(monkeypatch, w, h, env=None, camera=None, **kw):
    """The product kernel's handle and the diagnostics kernel's, created under `env`."""
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    tr = ds.CloudTracer(cloud(), width=w, height=h, **kw)
    monkeypatch.setenv("CT_STATS", "1")
    st = ds.CloudTracer(cloud(), width=w, height=h, **kw)
    monkeypatch.delenv("CT_STATS")
    for k in (env or {}):
        monkeypatch.delenv(k)
    if camera is not None:
        for t in (tr, st):
            t.set_camera(*pose(*camera, w, h))
    return tr, st


def check(tr, st, ref):
    """Both handles hold the reference's frame and counters; they fetched the same."""
    mean, m2, counters = ref
    for t in (tr, st):
        assert np.array_equal(t.mean(), mean)
        assert np.array_equal(t.m2(), m2)
        assert t.counters() == counters
    assert tr.fetch_counters() == st.fetch_counters()


def run_case(monkeypatch, w, h, spp, env=None, camera=None, f8=False, **kw):
    """One frame of spp subframes on both kernels against the oracle -> the product handle's fetch counters."""
    kw.setdefault("cloud_size_m", SIZE_M)
    tr, st = handles(monkeypatch, w, h, env=env, camera=camera, flags=F8 if f8 else 0, **kw)
    for t in (tr, st):
        t.render_accumulate(1, spp)
    check(tr, st, reference(w, h, spp, camera=camera, f8=f8, **kw))
    fetch = tr.fetch_counters()
    tr.close()
    st.close()
    return fetch


# ---- phase tables in LDS ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("f8", [False, True])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_phase_tables_every_mode_and_filter(monkeypatch, mode, f8):
    # mode 0 reads the un-chopped table at depth 1 and the chopped one after, mode 1 only the chopped, mode 2 only the un-chopped
    run_case(monkeypatch, 40, 32, 3, mode=mode, f8=f8)


@pytest.mark.parametrize("max_depth", [1, 2, 3])
def test_phase_tables_at_the_depth_cap(monkeypatch, max_depth):
    # 2: every path is capped after its first bounce, only the un-chopped table is ever read; 3: one read of each table
    if max_depth == 1:
        # (ct_create takes max_depth from 2: a path capped before its first march cannot be asked for)
        with pytest.raises(_lib.CloudTraceError) as e:
            ds.CloudTracer(cloud(), width=40, height=32, mode=0, max_depth=1, cloud_size_m=SIZE_M)
        assert e.value.code == _lib.CT_E_INVAL and "max_depth 2..65535" in e.value.message
        return
    run_case(monkeypatch, 40, 32, 3, mode=0, max_depth=max_depth)
    assert reference(40, 32, 3, mode=0, max_depth=max_depth, cloud_size_m=SIZE_M)[2]["depth_capped"] > 0


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_camera_ray_along_the_light(monkeypatch, sign):
    # Pixel (16, 16) of a 32 x 32 frame looks straight down +z (dx = dy = 0); with the light along -z / +z its first bounce has
    # cos = +1 / -1: texel coordinate 4095.5 / -0.5 of the un-chopped table, entries (4095, clamped 4096) / (clamped -1, 0).
    n = 64
    run_case(monkeypatch, 32, 32, 3, camera=((0.0, 0.0, -2.0), (0.0, 0.0, 0.0)), sample_step=1.0 / n,
             light_direction=(0.0, 0.0, -sign))


# ---- start records -----------------------------------------------------------------------------------------------------------

def test_partial_tiles_and_padded_slots(monkeypatch):
    w, h, spp = 37, 29, 3
    run_case(monkeypatch, w, h, spp)
    c = reference(w, h, spp, cloud_size_m=SIZE_M)[2]
    hits = c["box_hits"] // spp
    assert 0 < hits < w * h and hits % 64 != 0          # (the last group has padding slots)


def test_mode_without_a_prefix(monkeypatch):
    run_case(monkeypatch, 37, 29, 2, mode=1)


def test_camera_inside_the_box(monkeypatch):
    run_case(monkeypatch, 32, 24, 3, camera=((0.05, 0.1, -0.3), (0.0, 0.0, 0.0)))


def test_camera_looking_away(monkeypatch):
    # the box lies behind the camera: a quarter of the rays' LINES meet it, so those pixels are listed, but no sample starts
    cam = ((2.5, -0.4, 0.0), (5.0, -0.4, 0.0))
    run_case(monkeypatch, 40, 32, 2, camera=cam)
    c = reference(40, 32, 2, camera=cam, cloud_size_m=SIZE_M)[2]
    assert c["box_hits"] > 0 and c["density_lookups"] == 0


def test_no_hitting_pixel(monkeypatch):
    cam = ((2.5, -0.4, 0.0), (2.5, -0.4, 5.0))
    run_case(monkeypatch, 40, 32, 2, camera=cam)
    assert reference(40, 32, 2, camera=cam, cloud_size_m=SIZE_M)[2]["box_hits"] == 0


def test_second_pose_on_the_same_handle(monkeypatch):
    w, h = 40, 32
    far, near = ((0.4, 1.9, -1.2), (0.0, 0.0, 0.0)), ((1.2, 0.3, -0.8), (0.0, 0.0, 0.0))
    tr, st = handles(monkeypatch, w, h, camera=far, cloud_size_m=SIZE_M)
    for t in (tr, st):
        t.render_accumulate(1, 2)
    check(tr, st, reference(w, h, 2, camera=far, cloud_size_m=SIZE_M))
    for t in (tr, st):
        t.set_camera(*pose(*near, w, h))
        t.reset()
        t.render_accumulate(1, 2)
    check(tr, st, reference(w, h, 2, camera=near, cloud_size_m=SIZE_M))
    # (the second pose has more pixel groups than the first: the records were allocated again)
    assert reference(w, h, 2, camera=near, cloud_size_m=SIZE_M)[2]["box_hits"] > 2 * reference(w, h, 2, camera=far, cloud_size_m=SIZE_M)[2]["box_hits"]
    tr.close()
    st.close()


def test_new_light_on_the_same_handle(monkeypatch):
    w, h = 40, 32
    tr, st = handles(monkeypatch, w, h, cloud_size_m=SIZE_M, light_direction=ds.LIGHT_DIRECTIONS["Back"])
    for t in (tr, st):
        t.render_accumulate(1, 2)
        t.set_light(ds.LIGHT_DIRECTIONS["Side"])
        t.reset()
        t.render_accumulate(1, 3)
    check(tr, st, reference(w, h, 3, cloud_size_m=SIZE_M, light_direction=ds.LIGHT_DIRECTIONS["Side"]))
    tr.close()
    st.close()


def test_two_shards_make_the_unsharded_frame(monkeypatch):
    w, h = 40, 32
    mean, m2, counters = reference(w, h, 3, cloud_size_m=SIZE_M)
    for stats in (False, True):
        if stats:
            monkeypatch.setenv("CT_STATS", "1")
        total_mean, total_m2, ctr = np.zeros_like(mean), np.zeros_like(m2), None
        for i in range(2):
            with ds.CloudTracer(cloud(), width=w, height=h, cloud_size_m=SIZE_M, shard_index=i, shard_count=2) as sh:
                sh.render_accumulate(1, 3)
                m = sh.mean()
                assert np.all(m[~ds.shard_mask(w, h, i, 2)] == 0)
                total_mean += m
                total_m2 += sh.m2()
                c = sh.counters()
                ctr = c if ctr is None else {k: ctr[k] + c[k] for k in c}
        if stats:
            monkeypatch.delenv("CT_STATS")
        assert np.array_equal(total_mean, mean) and np.array_equal(total_m2, m2)
        assert ctr == counters


def test_three_batches_with_continuation(monkeypatch):
    # a thick medium and short batches: paths, and samples of jobs not yet started, cross the launch boundaries
    w, h = 64, 48
    kw = dict(cloud_size_m=30000.0, max_depth=300)
    tr, st = handles(monkeypatch, w, h, **kw)
    for t in (tr, st):
        t.render_accumulate_async(1, 2)
        t.render_accumulate_async(3, 1)
        t.render_accumulate_async(4, 2)
        t.synchronize()
    with ds.CloudTracer(cloud(), width=w, height=h, **kw) as sync:
        sync.render_accumulate(1, 5)
        for t in (tr, st):
            assert np.array_equal(t.mean(), sync.mean()) and np.array_equal(t.m2(), sync.m2())
            assert t.counters() == sync.counters()
    assert tr.debug_suspended() > 0
    tr.close()
    st.close()


def test_point_radiance_beside_an_image_on_one_handle(monkeypatch):
    # point tasks have no pixel groups and no prefix: their launches read the task's own ray, as before
    w, h = 40, 32
    rng = np.random.default_rng(5)
    pos = (rng.random((100, 3), dtype=np.float32) - 0.5) * 0.5
    d = rng.normal(size=(100, 3)).astype(np.float32)
    orc = O.Oracle(cloud(), w, h, fast=True, cloud_size_m=SIZE_M)
    want = orc.point_radiance_launch(ds.make_point_tasks(pos, d), 1, 3)
    tr, st = handles(monkeypatch, w, h, cloud_size_m=SIZE_M)
    for t in (tr, st):
        t.render_accumulate(1, 2)
        got = t.point_radiance_launch(ds.make_point_tasks(pos, d), 1, 3)
        assert got.tobytes() == want.tobytes()
        t.reset()
        t.render_accumulate(1, 2)
    check(tr, st, reference(w, h, 2, cloud_size_m=SIZE_M))
    tr.close()
    st.close()


def test_without_start_records(monkeypatch):
    # CT_START_RECORDS=0: image launches too go through pixel, primary ray and prefix
    assert run_case(monkeypatch, 37, 29, 3, env={"CT_START_RECORDS": "0"}) == run_case(monkeypatch, 37, 29, 3)


# ---- 32-bit footprint offsets ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sparse", [False, True])
def test_wide_offsets_equal_narrow_ones(monkeypatch, sparse):
    env = {"CT_SPARSE": "1"} if sparse else {}
    narrow = run_case(monkeypatch, 40, 32, 3, env={**env, "CT_WIDE_OFFSETS": "0"})
    wide = run_case(monkeypatch, 40, 32, 3, env={**env, "CT_WIDE_OFFSETS": "1"})
    assert narrow == wide
    assert narrow["density_fetches"] > 0 and narrow["inscatter_fetches"] > 0
