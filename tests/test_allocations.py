"""ct_debug_allocations: every device and pinned buffer of the library has one owner (deepestscatter_amd/csrc/ct_devmem.hpp),
which counts it when it allocates and when it frees.  So "nothing leaks" is exact: the four process-wide counters -- device
buffers, their bytes, pinned buffers, their bytes -- read the same before an object's life and after it.

Every GPU assertion is on the DIFFERENCE of two readings and asks for exactly zero in all four fields: other tests' fixtures may
hold handles in the same process, and free device memory moves under other people's work.  No tolerance of this file's own.

Scene: sphere_volume(32), a 64 x 48 frame, the (32, 1, 1) network of tests/test_network_render.py -- the smallest shapes that
still reach every growth path (a second pose with more listed pixels, enqueued batches, point launches of 64 and then 200 tasks,
a network render with and without the single-scatter temporary, every kind of bake)."""
import ctypes as C

import numpy as np
import pytest

import deepestscatter_amd as ds
from conftest import sphere_volume
from deepestscatter_amd import _lib
from deepestscatter_amd import cloudtrace as ct
from deepestscatter_amd import network as N
from test_network_render import LIGHT2, SID, SMALL, seeded_weights, weights

W, H = 64, 48
FIELDS = ("device_buffers", "device_bytes", "pinned_buffers", "pinned_bytes")
GRID = ((5, 5, 5), 4, 2)
# (129, 129, 129) is the grid of tests/test_network_bake_compact.py::test_a_grid_beyond_the_dense_limit; with 64 x 64 directions a
# node stores 4096 entries, so 16384 active nodes of its 2 146 689 already pass the 2^26 a table holds -- known only after the mask
GRID_REFUSED = ((129, 129, 129), 64, 64)


def readings():
    return ct.debug_allocations()


def since(before):
    now = readings()
    return {k: now[k] - before[k] for k in FIELDS}


ZERO = dict.fromkeys(FIELDS, 0)


def pose(eye):
    U, V, Wv = ds.calculate_camera_variables(eye, (0, 0, 0), (0, 1, 0), 30.0, W / H)
    return np.asarray(eye, np.float32), U, V, Wv


def point_tasks(n, seed):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.sqrt((d * d).sum(axis=1, keepdims=True))
    return ds.make_point_tasks(rng.uniform(-0.3, 0.3, (n, 3)).astype(np.float32), d)


def _code(fn, *a, **kw):
    with pytest.raises(_lib.CloudTraceError) as e:
        fn(*a, **kw)
    return e.value.code


# ---------------------------------------------------------------------------------------------------- CPU
def test_symbol_resolves_and_answers_a_null_argument(product_lib):
    assert hasattr(product_lib, "ct_debug_allocations") and "ct_debug_allocations" in _lib.EXPORTS
    assert product_lib.ct_debug_allocations(None) == _lib.CT_E_INVAL
    out = (C.c_uint64 * 4)(7, 7, 7, 7)
    assert product_lib.ct_debug_allocations(out) == _lib.CT_OK
    assert set(readings()) == set(FIELDS)


def test_a_create_refused_before_any_allocation_leaves_the_counters(product_lib):
    """abi_version off by one is refused before the device is opened.  Without a device nothing can have been allocated at all,
    so the counters read zero before and after; with one, other tests' handles may live, and they read the same."""
    from conftest import _has_gpu
    before = readings()
    if not _has_gpu():
        assert before == ZERO
    s, keep = ct.make_scene(sphere_volume(32), ct.SceneParams(width=W, height=H))
    s.abi_version = _lib.CT_ABI_VERSION + 1
    h = C.c_void_p()
    assert product_lib.ct_create(C.byref(s), C.byref(h)) == _lib.CT_E_INVAL and not h.value
    del keep
    assert readings() == before


# ---------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("estimator", [0, 1], ids=["MARCH", "DELTA"])
def test_the_full_life_of_a_handle(estimator, monkeypatch):
    monkeypatch.setenv("CT_STATS", "1")                       # (track_lines needs the diagnostics kernels)
    before = readings()
    tr = ds.CloudTracer(sphere_volume(32), width=W, height=H, estimator=estimator)
    try:
        tr.render_accumulate(1, 2)
        far = tr.debug_pixel_classes()["listed"]
        tr.set_camera(*pose((1.2, -0.2, 0.0)))
        near = tr.debug_pixel_classes()["listed"]
        assert near > far > 0                                 # the pixel list and the group arrays grow
        tr.reset()
        for k in range(3):
            tr.render_accumulate_async(1 + 2 * k, 2)          # the region ring and the continuation buffers are live
        tr.synchronize()
        assert tr.subframes == 6
        for n in (64, 200):                                   # the point buffers grow
            done = tr.point_radiance_launch(point_tasks(n, n), 1, 2)
            assert len(done) == n and np.isfinite(done["radiance"]).all()
        tr.track_lines(True)
        tr.track_lines(False)
        tr.tonemap(0.4)
        assert since(before)["device_buffers"] > 0
    finally:
        tr.close()
    assert since(before) == ZERO


def bakes_and_networks(tr, stale):
    """Every kind of bake and both network renders on tr; `stale`: the bakes are destroyed after a set_light."""
    net = N.Network(tr, weights(SMALL), 32, 1, 1)
    made = [net]
    try:
        for direct in (False, True):
            tr.network_render_subframe(net, SID, direct=direct)
        dense = tr.network_bake(net, *GRID)
        made.append(dense)
        made.append(tr.network_bake(net, *GRID, sparse=True))
        made.append(tr.network_bake(net, *GRID, compact=True))
        traced = tr.traced_bake(*GRID, 1)
        made.append(traced)
        dense.update(net)
        traced.retrace(1)
        traced.trace_more(1)
        assert traced.trace_info()["samples"] == 2
        if stale:
            tr.set_light(LIGHT2)
            assert not dense.info["current"]
    finally:
        for obj in reversed(made):                            # the bakes, then the network
            obj.close()


@pytest.mark.gpu
@pytest.mark.parametrize("stale", [False, True], ids=["current", "stale"])
def test_networks_and_bakes(stale):
    before = readings()
    with ds.CloudTracer(sphere_volume(32), width=W, height=H) as tr:
        bakes_and_networks(tr, stale)
    assert since(before) == ZERO


@pytest.mark.gpu
def test_refusals_that_come_after_memory_was_taken():
    """A refusal neither leaks nor drops anything: the difference while the handle lives is the same before and after the
    refused call, and zero once the handle is closed."""
    before = readings()
    with ds.CloudTracer(sphere_volume(32), width=W, height=H) as tr, N.Network(tr, weights(SMALL), 32, 1, 1) as net, \
            tr.network_bake(net, *GRID) as dense, tr.traced_bake(*GRID, 1) as traced:
        L, h = tr.L, tr.h
        tr.network_bake(net, *GRID, compact=True).close()     # (what a compact bake leaves with the handle is there already)
        no_aux = N.NetworkShape(32, 0, 1)
        with N.Network(tr, seeded_weights(no_aux, 2), 32, 0, 1) as other:
            live = since(before)
            # the stored table of a compact bake is counted by the mask: refused with the mask's buffers allocated
            assert _code(tr.network_bake, net, *GRID_REFUSED, compact=True) == _lib.CT_E_INVAL
            assert b"active nodes" in L.ct_last_error(h) and b"2^26" in L.ct_last_error(h)
            assert since(before) == live
            # ct_bake_update and ct_bake_retrace, refused by argument
            assert L.ct_bake_update(h, None, dense.b) == _lib.CT_E_INVAL and L.ct_bake_update(h, net.n, None) == _lib.CT_E_INVAL
            assert _code(dense.update, other) == _lib.CT_E_INVAL
            assert L.ct_bake_update(h, net.n, traced.b) == _lib.CT_E_INVAL
            assert _code(dense.retrace, 1) == _lib.CT_E_INVAL
            assert _code(traced.retrace, 0) == _lib.CT_E_INVAL and _code(traced.retrace, 65536) == _lib.CT_E_INVAL
            assert L.ct_bake_retrace(h, None, 1) == _lib.CT_E_INVAL
            assert since(before) == live
    assert since(before) == ZERO


@pytest.mark.gpu
def test_a_create_refused_after_the_first_layouts_frees_them():
    """The product's library refuses CT_FLAG_VMM_BRICKS in build_march_layouts, behind open_device, the Mie tables and the apron
    bricks: the one refusal of ct_create that arguments alone reach after memory was taken."""
    before = readings()
    with pytest.raises(_lib.CloudTraceError) as e:
        ds.CloudTracer(sphere_volume(32), width=W, height=H, flags=_lib.CT_FLAG_VMM_BRICKS)
    assert e.value.code == _lib.CT_E_INVAL and "experiments build" in e.value.message
    assert since(before) == ZERO


@pytest.mark.gpu
def test_a_group():
    before = readings()
    with ds.TracerGroup(sphere_volume(32), [0, 0], width=W, height=H) as g:
        g.render_accumulate(1, 2)
        g.merge()
        assert g.mean().any() and since(before)["device_buffers"] > 0
    assert since(before) == ZERO


@pytest.mark.gpu
def test_the_counters_count():
    """Device bytes: at least the buffers ct_buffer_bytes reports for the handle -- a lower bound from the library's own figures."""
    before = readings()
    with ds.CloudTracer(sphere_volume(32), width=W, height=H) as tr:
        reported = 0
        for which in range(6):
            n = C.c_size_t(0)
            assert tr.L.ct_buffer_bytes(tr.h, which, C.byref(n)) == _lib.CT_OK and n.value > 0
            reported += n.value
        live = since(before)
        assert live["device_buffers"] > 0 and live["pinned_buffers"] > 0 and live["pinned_bytes"] > 0
        assert live["device_bytes"] >= reported
    assert since(before) == ZERO
