"""The MARCH estimator's shadow-zero NEE skip (run with -m gpu on an MI355X).

A collision in a march-brick row whose bit 6 ("shadow-zero") is set skips its NEE: every shadow-volume footprint the scatter
position can read is all zero, so the NEE would add +0.  Frames and counters must stay those of the oracle bit for bit in
every place where the flag could be wrong, and the flags themselves must be those of a numpy reference built from the
oracle's shadow volume.
"""
import math

import numpy as np
import pytest

import _oracle as O
import deepestscatter_amd as ds

pytestmark = pytest.mark.gpu

AXIS_LIGHT = (0.0, -1.0, 0.0)


def expected_radius(n_max: int, sample_step: float) -> int:
    """ct_api.cpp nee_skip_radius: the scatter position's base texel is within ceil(D) of the collision's."""
    s = float(np.float32(n_max))
    reach = float(np.float32(np.float32(sample_step) * np.float32(1.0 - 1.0 / 256.0)))
    d = reach * s * (1.0 + 2.0 ** -20) + 2.0 ** -22 * (s + 1.0)
    return max(1, math.ceil(d)) if d < 8 else 0


def reference_flags(shadow: np.ndarray, meta: np.ndarray, r: int, bias_x: int, bias: int) -> np.ndarray:
    """bit 6 of every row: clearance 0, and no base texel within Chebyshev distance r of the row's three bases has a
    non-zero clamped shadow footprint or lies outside the volume."""
    nz, ny, nx = shadow.shape
    s = shadow != 0
    # footprint of base b = texels b, min(b + 1, n - 1) on every axis
    f = s | np.concatenate([s[:, :, 1:], s[:, :, -1:]], axis=2)
    f = f | np.concatenate([f[:, 1:, :], f[:, -1:, :]], axis=1)
    f = f | np.concatenate([f[1:, :, :], f[-1:, :, :]], axis=0)
    pad = np.ones((nz + 2 * r, ny + 2 * r, nx + 2 * r), bool)     # outside the volume: blocked
    pad[r:r + nz, r:r + ny, r:r + nx] = f
    for axis in range(3):
        n = pad.shape[axis]
        acc = np.zeros_like(pad)
        for k in range(-r, r + 1):
            idx = np.clip(np.arange(n) + k, 0, n - 1)
            shifted = np.take(pad, idx, axis=axis)
            edge = (np.arange(n) + k < 0) | (np.arange(n) + k >= n)
            if edge.any():
                shape = [1, 1, 1]
                shape[axis] = n
                shifted = shifted | edge.reshape(shape)
            acc |= shifted
        pad = acc
    near = pad[r:r + nz, r:r + ny, r:r + nx]                        # a blocked base within r
    zr, yr, bx = meta.shape
    z = np.arange(zr) - bias
    y = np.arange(yr) - bias
    ok = np.ones(meta.shape, bool)
    zin = (z >= 0) & (z < nz)
    yin = (y >= 0) & (y < ny)
    for k in range(3):
        x = 3 * np.arange(bx) - bias_x + k
        xin = (x >= 0) & (x < nx)
        good = np.zeros(meta.shape, bool)
        zz, yy, xx = np.ix_(np.clip(z, 0, nz - 1), np.clip(y, 0, ny - 1), np.clip(x, 0, nx - 1))
        good[:] = ~near[zz, yy, xx]
        good &= zin[:, None, None] & yin[None, :, None] & xin[None, None, :]
        ok &= good
    return ok & ((meta & 0x3F) == 0)


def thick_cloud(n: int) -> np.ndarray:
    return ds.make_procedural_cloud(n)


def run_case(monkeypatch, tex, w, h, spp, window=None, camera=None, sparse=False, check_flags=True, **kw):
    """Renders with the product kernel and the diagnostics kernel; both against the oracle."""
    if sparse:
        monkeypatch.setenv("CT_SPARSE", "1")
    tr = ds.CloudTracer(tex, width=w, height=h, **kw)
    monkeypatch.setenv("CT_STATS", "1")
    st = ds.CloudTracer(tex, width=w, height=h, **kw)
    monkeypatch.delenv("CT_STATS")
    ins = tr.inscatter()
    okw = {k: v for k, v in kw.items() if k in ("mode", "cloud_size_m", "sample_step", "max_depth", "light_direction")}
    big = tex.size > 256 ** 3
    orc = O.Oracle(tex, w, h, fast=True, inscatter=ins if big else None, **okw)
    if not big:
        assert np.array_equal(ins, orc.inscatter)
    if camera is not None:
        eye, lookat = camera
        U, V, W = ds.calculate_camera_variables(eye, lookat, (0, 1, 0), 60.0, w / h)
        for t in (tr, st, orc):
            t.set_camera(eye, U, V, W)
    tr.render_accumulate(1, spp)
    st.render_accumulate(1, spp)
    ref_mean, ref_m2 = orc.render(spp, window=window)
    x0, y0, x1, y1 = window or (0, 0, w, h)
    for t in (tr, st):
        assert np.array_equal(t.mean()[y0:y1, x0:x1], ref_mean[y0:y1, x0:x1])
        assert np.array_equal(t.m2()[y0:y1, x0:x1], ref_m2[y0:y1, x0:x1])
        if window is None:
            assert t.counters() == orc.counters.as_dict()
    assert np.array_equal(tr.mean(), st.mean()) and tr.counters() == st.counters()
    assert tr.fetch_counters() == st.fetch_counters()
    stats = st.debug_stats()
    c, f = st.counters(), st.fetch_counters()
    assert f["inscatter_fetches"] == c["inscatter_lookups"] - stats["nee_footprints_reused"]
    mm = tr.march_meta()
    if check_flags and not mm["sparse"]:
        assert mm["radius"] == expected_radius(max(tex.shape), kw.get("sample_step", 1.0 / 512.0))
        want = reference_flags(ins, mm["meta"], mm["radius"], mm["bias_x"], mm["bias"])
        assert np.array_equal((mm["meta"] & 0x40) != 0, want)
    tr.close()
    st.close()
    return stats["nee_lookups_skipped_shadow_zero"], c["inscatter_lookups"], mm


@pytest.mark.parametrize("light", ["Front", "Side", "Back"])
def test_light_directions(monkeypatch, light):
    tex = thick_cloud(64)
    skipped, lookups, _ = run_case(monkeypatch, tex, 40, 32, 3, cloud_size_m=20000.0,
                                   light_direction=ds.LIGHT_DIRECTIONS[light])
    assert 0 < skipped < lookups


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_all_modes(monkeypatch, mode):
    tex = thick_cloud(64)
    skipped, lookups, _ = run_case(monkeypatch, tex, 40, 32, 3, mode=mode, cloud_size_m=20000.0)
    assert 0 < skipped < lookups


def test_long_step_gives_a_wider_flag(monkeypatch):
    tex = thick_cloud(128)
    skipped, lookups, mm = run_case(monkeypatch, tex, 40, 32, 2, sample_step=1.0 / 100.0, cloud_size_m=30000.0)
    assert mm["radius"] == 2
    assert 0 < skipped < lookups


def test_axis_aligned_light_and_camera_ray(monkeypatch):
    # one texel per step; the middle pixel of an odd-sized frame looks straight down the z axis
    n = 64
    tex = thick_cloud(n)
    skipped, lookups, mm = run_case(monkeypatch, tex, 33, 33, 3, camera=((0.0, 0.0, -2.0), (0.0, 0.0, 0.0)),
                                    sample_step=1.0 / n, cloud_size_m=20000.0, light_direction=AXIS_LIGHT)
    assert mm["radius"] == 1
    assert 0 < skipped < lookups


def test_camera_inside_the_box(monkeypatch):
    # (world coordinates: the box is [-0.5, 0.5]^3 around the origin)
    tex = thick_cloud(64)
    skipped, lookups, _ = run_case(monkeypatch, tex, 32, 24, 3, camera=((0.05, 0.1, -0.3), (0.0, 0.0, 0.0)),
                                   cloud_size_m=20000.0)
    assert 0 < skipped < lookups


def test_cloud_touching_the_volume_faces(monkeypatch):
    tex = thick_cloud(48)
    tex[0] = np.maximum(tex[0], 90)                  # z = 0 and y = ny-1 layers full, and a slab through x = 0
    tex[:, -1] = np.maximum(tex[:, -1], 90)
    tex[10:30, 10:30, :6] = 160
    skipped, lookups, _ = run_case(monkeypatch, tex, 40, 32, 3, cloud_size_m=20000.0,
                                   light_direction=ds.LIGHT_DIRECTIONS["Back"])
    assert 0 < skipped < lookups


def test_sparse_bricks(monkeypatch):
    tex = thick_cloud(64)
    skipped, lookups, mm = run_case(monkeypatch, tex, 40, 32, 3, sparse=True, cloud_size_m=20000.0)
    assert mm["sparse"]
    assert 0 < skipped < lookups


def test_window_of_a_1024_cube(monkeypatch):
    tex = ds.make_procedural_cloud(1024)
    w = h = 256
    win = (120, 120, 136, 136)
    skipped, lookups, _ = run_case(monkeypatch, tex, w, h, 2, window=win)
    assert 0 < skipped < lookups
