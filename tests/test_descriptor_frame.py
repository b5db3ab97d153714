"""ct_descriptor_frame: per pixel of a rect the first scatter position of the primary ray and the hierarchical descriptor there,
compacted on the device in the rect's row-major order.

The reference is `restate` below: the first lines of the oracle's orc_render_subframe / radiance_of_ray and its
next_scattering_event, restated in np.float32 scalar arithmetic (one operation per rounding) on the oracle's exported
primitives (orc_tea4, orc_rnd, orc_expf, orc_logf, orc_tex3d, orc_derived_uniforms) -- never the code under test.  The CPU
tests tie it to the oracle itself: every pixel the oracle's single-scatter render lights is one the restatement calls valid.
A restated scene is computed once per process and shared by the tests that need it."""
import ctypes as C

import numpy as np
import pytest

import _oracle as O
import deepestscatter_amd as ds
from deepestscatter_amd import _lib
from conftest import sphere_volume

F = np.float32
EYE = (2.5, -0.4, 0.0)                 # the default pose of both the library and the oracle
EYE2 = (1.1, 1.6, -1.4)
LIGHT2 = (0.586, -0.766, -0.271)
MAIN = dict(cloud_size_m=700.0)        # the issue's scene: sphere_volume(32, seed=13), 24 x 16, default eye
COARSE = dict(cloud_size_m=700.0, sample_step=1.0 / 128.0)   # the compaction cases: a quarter of the march steps per flight


def _tex():
    return sphere_volume(32, seed=13)


# ------------------------------------------------------------------------------------------------ the restatement
def _norm(v):
    """optix::normalize: v * (1 / sqrtf(dot(v, v)))"""
    inv = F(1) / np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    return (v[0] * inv, v[1] * inv, v[2] * inv)


def restate(orc, subframe_id, rect=None, fast=False):
    """-> (pixels uint32 [n], positions float32 [n,3], directions float32 [n,3]) of the valid pixels of `rect` in its
    row-major order, for the oracle scene `orc` (its volume, camera and uniforms).  `fast` names the oracle build whose
    texture unit is used ("fixed8": 1.8 fixed-point weights)."""
    L = O.lib(fast)
    u = orc.derived_uniforms()
    bbox = (F(u[0]), F(u[1]), F(u[2]))
    dm, step = F(u[6]), F(u[15])
    s = orc.scene
    width, height = int(s.width), int(s.height)
    eye = tuple(F(v) for v in s.eye)
    U, V, W = (tuple(F(v) for v in a) for a in (s.U, s.V, s.W))
    nz, ny, nx = orc.density.shape
    dims = (C.c_uint32 * 3)(nx, ny, nz)
    texels = orc.density.ctypes.data_as(C.c_void_p)
    p3 = (C.c_float * 3)()
    lo, hi = F(-0.01), tuple(b + F(0.01) for b in bbox)
    half = tuple(b * F(0.5) for b in bbox)

    def in_box(p):
        return bool(p[0] >= lo and p[1] >= lo and p[2] >= lo and p[0] <= hi[0] and p[1] <= hi[1] and p[2] <= hi[2])

    def tex(p):
        p3[0], p3[1], p3[2] = float(p[0]), float(p[1]), float(p[2])
        return F(L.orc_tex3d(texels, dims, p3))

    def intersect_box(o, d):
        bmin = tuple(-b / F(2) for b in bbox)
        bmax = tuple(b / F(2) for b in bbox)
        with np.errstate(divide="ignore", invalid="ignore"):
            t0 = tuple((bmin[i] - o[i]) / d[i] for i in range(3))
            t1 = tuple((bmax[i] - o[i]) / d[i] for i in range(3))
        tmin = np.fmax(np.fmax(np.fmin(t0[0], t1[0]), np.fmin(t0[1], t1[1])), np.fmin(t0[2], t1[2]))
        tmax = np.fmin(np.fmin(np.fmax(t0[0], t1[0]), np.fmax(t0[1], t1[1])), np.fmax(t0[2], t1[2]))
        if tmin <= tmax:
            if tmin > F(0) and tmin < F(1e27):
                return F(tmin)
            return F(0.000001)
        return None

    def flight(xi, pos, d):
        """next_scattering_event: step, then sample; collide when xi > T"""
        sx, sy, sz = d[0] * step, d[1] * step, d[2] * step
        T = F(1)
        while in_box(pos):
            pos = (pos[0] + sx, pos[1] + sy, pos[2] + sz)
            density = tex(pos) * dm
            extinction = density * step
            T = T * F(L.orc_expf(-extinction))
            if xi > T:
                lg = F(L.orc_logf(xi / T))
                inv = F(1) / density
                return True, (pos[0] - d[0] * lg * inv, pos[1] - d[1] * lg * inv, pos[2] - d[2] * lg * inv)
        return False, pos

    x0, y0, x1, y1 = rect or (0, 0, width, height)
    pix, ps, ds_ = [], [], []
    for y in range(y0, y1):
        for x in range(x0, x1):
            dx = F(x) / F(width) * F(2) - F(1)
            dy = F(y) / F(height) * F(2) - F(1)
            d1 = _norm(tuple(U[i] * dx + V[i] * dy + W[i] for i in range(3)))
            t_hit = intersect_box(eye, d1)
            if t_hit is None:
                continue
            pos = tuple(eye[i] + d1[i] * t_hit + half[i] for i in range(3))
            d2 = _norm(d1)
            seed = C.c_uint32(L.orc_tea4((x * 4096 + y) & 0xFFFFFFFF, subframe_id))
            xi = F(L.orc_rnd(C.byref(seed)))
            scattered, sp = flight(xi, pos, d2)
            if scattered and in_box(sp):
                pix.append(y * width + x)
                ps.append(tuple(sp[i] - half[i] for i in range(3)))
                ds_.append(d2)
    return (np.array(pix, np.uint32), np.array(ps, np.float32).reshape(-1, 3), np.array(ds_, np.float32).reshape(-1, 3))


_CACHE = {}


def _oracle(w, h, fast=False, eye=EYE, light=None, **kw):
    key = ("orc", w, h, fast, eye, light, tuple(sorted(kw.items())))
    if key not in _CACHE:
        extra = {"light_direction": light} if light else {}
        _CACHE[key] = O.Oracle(_tex(), w, h, mode=2, fast=fast, eye=eye, **extra, **kw)
    return _CACHE[key]


def reference(w, h, subframe_id, rect=None, fast=False, eye=EYE, **kw):
    """The restatement of a scene, computed once (the light does not enter the flight)."""
    key = ("ref", w, h, subframe_id, rect, fast, eye, tuple(sorted(kw.items())))
    if key not in _CACHE:
        _CACHE[key] = restate(_oracle(w, h, fast=fast, eye=eye, **kw), subframe_id, rect, fast=fast)
    return _CACHE[key]


def _np(result):
    d, p, v, px = (t.cpu().numpy() for t in result)
    return d, p, v, px.astype(np.uint32)


def _filtered(full, rect, width):
    """The records of a whole-frame result whose pixel lies in `rect`, in the rect's row-major order (which is the frame's)."""
    d, p, v, px = full
    x, y = px % width, px // width
    keep = (x >= rect[0]) & (x < rect[2]) & (y >= rect[1]) & (y < rect[3])
    return d[keep], p[keep], v[keep], px[keep]


def _same(a, b):
    return all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("sid", [1, 7])
def test_restatement_holds_every_pixel_the_oracle_lights(sid):
    """Mode 2 adds radiance exactly where the first flight scattered inside the box; the in-scattered light there may still be
    zero (a fully shadowed point), so the lit pixels are a subset of the valid ones."""
    w, h = 24, 16
    orc = _oracle(w, h, **MAIN)
    lit = np.flatnonzero(orc.render_subframe(sid)[..., :3].any(axis=-1).reshape(-1))
    pix, pos, view = reference(w, h, sid, **MAIN)
    assert 100 < len(pix) < 300
    assert len(lit) > 100 and np.isin(lit, pix).all()
    assert np.all(np.diff(pix.astype(np.int64)) > 0)
    assert np.isfinite(pos).all() and np.allclose(np.linalg.norm(view, axis=1), 1.0, atol=1e-6)
    assert orc.collect_descriptors(pos, view).reshape(len(pix), -1).any(axis=1).all()   # every record sees the cloud


def test_null_handle_is_invalid(product_lib):
    n = C.c_uint32(7)
    assert product_lib.ct_descriptor_frame(None, 1, None, 0, None, None, None, None, C.byref(n)) == _lib.CT_E_INVAL
    assert product_lib.ct_debug_descriptor_frame_time(None, None, None) == _lib.CT_E_INVAL
    assert "ct_descriptor_frame" in _lib.EXPORTS


# ---------------------------------------------------------------------------------------------------- GPU
def _check_against_reference(tr, orc, ref, got):
    pix, pos, view = ref
    d, p, v, px = got
    assert len(px) == len(pix) and np.array_equal(px, pix)
    assert np.all(np.diff(px.astype(np.int64)) > 0)
    assert np.array_equal(p, pos) and np.array_equal(v, view)
    assert d.shape == (len(pix), 10, 9, 5, 5)
    assert np.array_equal(d, orc.collect_descriptors(pos, view))
    assert np.array_equal(d, tr.collect_descriptors(pos, view))


@pytest.mark.gpu
@pytest.mark.parametrize("sid", [1, 7])
def test_frame_equals_the_restatement_and_the_oracles_descriptors(sid):
    w, h = 24, 16
    with ds.CloudTracer(_tex(), width=w, height=h, **MAIN) as tr:
        got = _np(tr.descriptor_frame(sid))
        _check_against_reference(tr, _oracle(w, h, **MAIN), reference(w, h, sid, **MAIN), got)
        assert _same(got, _np(tr.descriptor_frame(sid)))            # the same call, the same bytes
        assert all(t >= 0 for t in tr.descriptor_frame_time())


@pytest.mark.gpu
def test_fixed8_frame_equals_the_fixed8_restatement():
    w, h, sid = 24, 16, 7
    ref = reference(w, h, sid, fast="fixed8", **MAIN)
    with ds.CloudTracer(_tex(), width=w, height=h, flags=_lib.CT_FLAG_TEX_FIXED8, **MAIN) as tr:
        _check_against_reference(tr, _oracle(w, h, fast="fixed8", **MAIN), ref, _np(tr.descriptor_frame(sid)))
    exact = reference(w, h, sid, **MAIN)
    assert not (np.array_equal(ref[0], exact[0]) and np.array_equal(ref[1], exact[1]))   # the flag changes the flight


@pytest.mark.gpu
def test_compaction_of_a_frame_that_is_no_multiple_of_a_wave():
    w, h, sid = 80, 3, 3          # 240 pixels: three full waves and one of 48 lanes
    pix, pos, view = reference(w, h, sid, **COARSE)
    assert 0 < len(pix) < w * h
    with ds.CloudTracer(_tex(), width=w, height=h, **COARSE) as tr:
        d, p, v, px = _np(tr.descriptor_frame(sid))
    assert np.array_equal(px, pix) and np.array_equal(p, pos) and np.array_equal(v, view)


BAND = (0, 18, 72, 22)   # four rows through the middle of the 72 x 40 frame


@pytest.mark.gpu
def test_compaction_across_blocks_and_rects_of_the_frame():
    """72 x 40 = 45 waves in 12 blocks.  The band of rows is held against the restatement; every other rect against the
    whole-frame result filtered to it, which for the band is the same thing."""
    w, h, sid = 72, 40, 5
    pix, pos, view = reference(w, h, sid, rect=BAND, **COARSE)
    assert 20 < len(pix) < 4 * w - 20
    with ds.CloudTracer(_tex(), width=w, height=h, **COARSE) as tr:
        full = _np(tr.descriptor_frame(sid))
        assert np.all(np.diff(full[3].astype(np.int64)) > 0) and 300 < len(full[3]) < w * h - 300
        band = _np(tr.descriptor_frame(sid, rect=BAND))
        assert np.array_equal(band[3], pix) and np.array_equal(band[1], pos) and np.array_equal(band[2], view)
        assert _same(band, _filtered(full, BAND, w))
        valid = set(int(v) for v in full[3])
        lit = int(full[3][len(full[3]) // 2])
        sky = next(q for q in range(w * h) if q not in valid)
        rects = [(0, 0, w, 1), (0, h - 1, w, h), (7, 3, 7 + 45, 31), (33, 11, 34, 40), (1, 0, 72, 40), (0, 0, 64, 40),
                 (lit % w, lit // w, lit % w + 1, lit // w + 1)]
        for r in rects:
            assert _same(_np(tr.descriptor_frame(sid, rect=r)), _filtered(full, r, w)), r
        one = _np(tr.descriptor_frame(sid, rect=rects[-1]))
        assert len(one[3]) == 1 and one[3][0] == lit
        none = tr.descriptor_frame(sid, rect=(sky % w, sky // w, sky % w + 1, sky // w + 1))     # CT_OK, no record
        assert [tuple(t.shape) for t in none] == [(0, 10, 9, 5, 5), (0, 3), (0, 3), (0,)]
        # a rect outside the frame or empty is refused, and the handle goes on working
        for r in [(0, 0, w + 1, h), (0, 0, w, h + 1), (5, 5, 5, 9), (5, 9, 8, 9), (9, 5, 8, 9), (w, 0, w + 1, 1)]:
            with pytest.raises(_lib.CloudTraceError) as e:
                tr.descriptor_frame(sid, rect=r)
            assert e.value.code == _lib.CT_E_INVAL, r
        assert _same(_np(tr.descriptor_frame(sid)), full)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,rows", [(320, 208, 104), (1024, 1024, 64)])
def test_scan_over_more_wave_counts_than_the_block_has_threads(w, h, rows):
    """Above 65536 pixels a thread of the scan owns 2 (here: 1040 waves) to 16 (2^20 pixels, the largest rect) wave counts.  Bands
    of rows of at most 65536 pixels take the one-count-per-thread path that the tests above hold against the restatement, and
    in row-major order the whole frame is its bands one after the other.  A distant eye keeps the records few."""
    import torch
    eye = (9.0, -1.5, 0.5)
    U, V, Wv = O.camera_variables(eye, aspect=w / h)
    with ds.CloudTracer(_tex(), width=w, height=h, **COARSE) as tr:
        tr.set_camera(eye, U, V, Wv)
        with pytest.raises(_lib.CloudTraceError) as e:
            tr.descriptor_frame(2, capacity=0)
        needed = e.value.needed
        assert e.value.code == _lib.CT_E_INVAL and 500 < needed < w * h // 8
        full = tr.descriptor_frame(2, capacity=needed)
        assert len(full[3]) == needed and bool((full[3][1:] > full[3][:-1]).all())
        bands = [tr.descriptor_frame(2, rect=(0, y, w, y + rows), capacity=needed) for y in range(0, h, rows)]
        for i in range(4):
            assert torch.equal(full[i], torch.cat([b[i] for b in bands]))
        if w * h > (1 << 20) - 1:       # the largest rect there is; one more pixel is refused
            with ds.CloudTracer(_tex(), width=w + 1, height=h, **COARSE) as wider:
                wider.set_camera(eye, U, V, Wv)     # (a new handle has the default pose, whose records are many)
                with pytest.raises(_lib.CloudTraceError) as e:
                    wider.descriptor_frame(2, capacity=needed)
                assert e.value.code == _lib.CT_E_INVAL and e.value.needed == 0      # refused for its area, nothing counted
                # its pixels are not the other frame's (x / 1025), so neither is its count: twice that is room enough
                assert needed // 2 < len(wider.descriptor_frame(2, rect=(1, 0, w + 1, h), capacity=2 * needed)[3]) < 2 * needed


@pytest.mark.gpu
def test_capacity_one_short_is_refused_with_the_needed_count():
    w, h, sid = 24, 16, 1
    pix = reference(w, h, sid, **MAIN)[0]
    with ds.CloudTracer(_tex(), width=w, height=h, **MAIN) as tr, ds.CloudTracer(_tex(), width=w, height=h, **MAIN) as fresh:
        with pytest.raises(_lib.CloudTraceError) as e:
            tr.descriptor_frame(sid, capacity=len(pix) - 1)
        assert e.value.code == _lib.CT_E_INVAL and e.value.needed == len(pix)
        got = _np(tr.descriptor_frame(sid, capacity=len(pix)))
        assert len(got[3]) == len(pix) and _same(got, _np(fresh.descriptor_frame(sid)))


def _state(tr):
    return tr.mean(), tr.m2(), tr.subframes, tr.counters(), tr.fetch_counters()


@pytest.mark.gpu
@pytest.mark.parametrize("ahead", [False, True])
def test_no_side_effects_on_a_progressive_render(ahead):
    w, h = 24, 16
    states = []
    for with_call in (True, False):
        with ds.CloudTracer(_tex(), width=w, height=h, **MAIN) as tr:
            if ahead:
                tr.set_render_ahead(8)
                tr.render_accumulate_async(1, 2)
            else:
                tr.render_accumulate(1, 2)
            if with_call:
                rendered = tr.rendered_subframes()
                assert len(tr.descriptor_frame(4)[3]) > 100
                assert tr.rendered_subframes() == rendered and tr.subframes == 2     # nothing rendered ahead was dropped
            if ahead:
                tr.render_accumulate_async(3, 2)
                tr.synchronize()
            else:
                tr.render_accumulate(3, 2)
            states.append(_state(tr))
    a, b = states
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[0].any()
    assert a[2:] == b[2:] and a[2] == 4


@pytest.mark.gpu
def test_delta_and_sparse_handles_return_the_march_handles_bytes():
    w, h, sid = 24, 16, 7
    with ds.CloudTracer(_tex(), width=w, height=h, **MAIN) as tr:
        want = _np(tr.descriptor_frame(sid))
    assert np.array_equal(want[3], reference(w, h, sid, **MAIN)[0])
    for kw in (dict(estimator=_lib.CT_EST_DELTA), dict(flags=_lib.CT_FLAG_SPARSE_BRICKS), dict(mode=2)):
        with ds.CloudTracer(_tex(), width=w, height=h, **kw, **MAIN) as tr:
            assert _same(_np(tr.descriptor_frame(sid)), want), kw


@pytest.mark.gpu
def test_after_set_camera_and_set_light():
    w, h, sid = 24, 16, 1
    with ds.CloudTracer(_tex(), width=w, height=h, **MAIN) as tr:
        first = _np(tr.descriptor_frame(sid))
        # a new light: the same flights, descriptors in the new light's frame
        tr.set_light(LIGHT2)
        lit = _np(tr.descriptor_frame(sid))
        _check_against_reference(tr, _oracle(w, h, light=LIGHT2, **MAIN), reference(w, h, sid, **MAIN), lit)
        assert _same(lit[1:], first[1:]) and not np.array_equal(lit[0], first[0])
        # a second eye
        U, V, W = O.camera_variables(EYE2, aspect=w / h)
        tr.set_camera(EYE2, U, V, W)
        ref = reference(w, h, sid, eye=EYE2, **MAIN)
        assert 50 < len(ref[0]) < w * h and not np.array_equal(ref[0], first[3])
        _check_against_reference(tr, _oracle(w, h, eye=EYE2, light=LIGHT2, **MAIN), ref, _np(tr.descriptor_frame(sid)))
        # a camera that looks away from the box
        U, V, W = O.camera_variables(EYE, lookat=(5.0, -0.8, 0.0), aspect=w / h)
        tr.set_camera(EYE, U, V, W)
        assert [len(t) for t in tr.descriptor_frame(sid)] == [0, 0, 0, 0]
