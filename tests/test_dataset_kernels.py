"""The dataset half of the library at its edges: the device mip pyramid, ct_collect_descriptors, ct_generate_scatter_samples and
ct_point_radiance_launch (the GPU cases run with -m gpu on an MI355X).

Every GPU result is held to the oracle bit for bit, as elsewhere.  What is new here is what the oracle itself is held to, and
what needs no oracle at all:
  * the mip pyramid (host and device) against a numpy integer restatement of Resources::generateMipmaps (Resources.cpp:169-209),
  * the oracle's descriptor bytes against a float64 numpy restatement of setupHierarchicalDescriptor (DisneyDescriptor.cuh:71-112,
    as include/cloudtrace.h describes it),
  * every finite scatter sample: a unit view direction, a position inside the box, density there,
  * ct_point_radiance_launch's fold and job cutting: K calls of one launch, folded in numpy float32 with
    PointRadianceTask::addExperimentResult (PointRadianceTask.h:40-51), against one call of K launches.
Volumes are given as numpy shapes, [Z, Y, X].
"""
import ctypes as C

import numpy as np
import pytest

import _oracle as O
import deepestscatter_amd as ds
from deepestscatter_amd import _lib
from conftest import sphere_volume

gpu = pytest.mark.gpu
f32 = np.float32

DEFAULT_LIGHT = ds.LIGHT_DIRECTIONS["Side"]
LIGHTS = {"default": DEFAULT_LIGHT, "down": (0.0, -1.0, 0.0), "x": (1.0, 0.0, 0.0), "oblique": (0.41, -0.77, -0.52)}
MARCH, DELTA = 0, 1
KINDS = {"march": dict(estimator=MARCH), "delta": dict(estimator=DELTA),
         "sparse": dict(estimator=MARCH, flags=_lib.CT_FLAG_SPARSE_BRICKS), "simple": dict(estimator=MARCH, flags=_lib.CT_FLAG_SIMPLE_KERNEL)}

_CACHE = {}


def cached(key, make):
    """Volumes and references are computed once, shared between the tests and never modified."""
    if key not in _CACHE:
        v = make()
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        _CACHE[key] = v
    return _CACHE[key]


def random_bytes(shape, seed):
    """Dense random bytes without a zero border; one texel in eight is 255, so that sums of eight reach past a byte."""
    def make():
        rng = np.random.default_rng(seed)
        t = rng.integers(0, 256, shape, dtype=np.uint8)
        t[rng.random(shape) < 0.125] = 255
        return t
    return cached(("random", shape, seed), make)


def sphere(shape, seed):
    return cached(("sphere", shape, seed), lambda: sphere_volume(dims=shape, seed=seed))


def half_box(shape):
    """Half the box's edges in world coordinates, (x, y, z): bboxSize = dims / maxDim (VDBCloud.cpp:98-111)."""
    nz, ny, nx = shape
    return np.array([nx, ny, nz], np.float64) / max(shape) / 2


def tracer(tex, **kw):
    kw.setdefault("width", 8)
    kw.setdefault("height", 8)
    kw.setdefault("light_direction", DEFAULT_LIGHT)
    return ds.CloudTracer(tex, **kw)


def oracle(tex, **kw):
    """The oracle for the same keywords.  The dataset kernels that read no shadow volume get inscatter="none"."""
    kw = {k: v for k, v in kw.items() if k != "flags"}
    kw.setdefault("light_direction", DEFAULT_LIGHT)
    return O.Oracle(tex, 8, 8, fast=True, **kw)


# ======================================================================================================================
# 1. the mip pyramid
# ======================================================================================================================
def np_mipmaps(level0):
    """Resources::generateMipmaps, Resources.cpp:169-209, in integers: floor(log2(maxDim)) + 1 levels of max(1, n >> l) texels
    per axis; a texel is the uint16 sum of its up-to-8 children 2i + {0, 1} -- those at or past the parent's size count as
    zero, and the child that n >> 1 drops at an odd size is simply never read -- divided by 8, truncating."""
    levels = [np.asarray(level0, np.uint8)]
    count = int(np.floor(np.log2(max(level0.shape)))) + 1
    for l in range(1, count):
        prev = levels[-1]
        cz, cy, cx = (max(1, n >> l) for n in level0.shape)
        kids = np.zeros((2 * cz, 2 * cy, 2 * cx), np.uint16)
        pz, py, px = (min(p, 2 * c) for p, c in zip(prev.shape, (cz, cy, cx)))
        kids[:pz, :py, :px] = prev[:pz, :py, :px]
        total = kids.reshape(cz, 2, cy, 2, cx, 2).sum(axis=(1, 3, 5), dtype=np.uint16)
        levels.append((total // 8).astype(np.uint8))
    return levels


def level_offsets(shape):
    """Level count, per-level shapes and byte offsets, derived here from the level-0 size alone."""
    count = 1
    while max(shape) >> count:
        count += 1
    shapes = [tuple(max(1, n >> l) for n in shape) for l in range(count)]
    sizes = [int(np.prod(s)) for s in shapes]
    return count, shapes, [sum(sizes[:l]) for l in range(count)], sum(sizes)


MIP_SHAPES = [(37, 53, 45), (8, 48, 20), (5, 3, 2), (33, 2, 2), (64, 64, 64)]   # ct_create refuses an axis of one texel: (33, 2, 2)


def test_np_mipmaps_on_cases_done_by_hand():
    a = np.array([[[255, 255], [255, 254]], [[255, 255], [255, 255]]], np.uint8)            # 2039 / 8 = 254, not 2039 % 256
    assert [l.tolist() for l in np_mipmaps(a)] == [a.tolist(), [[[254]]]]
    b = np.full((1, 1, 5), 200, np.uint8)                                                  # x: 5 -> 2 -> 1; y, z stay 1
    assert [l.ravel().tolist() for l in np_mipmaps(b)] == [[200] * 5, [50, 50], [12]]      # two children each, the fifth dropped
    assert level_offsets((1, 1, 5)) == (3, [(1, 1, 5), (1, 1, 2), (1, 1, 1)], [0, 5, 7], 8)


@pytest.mark.parametrize("shape", MIP_SHAPES + [(33, 1, 1)])
def test_host_mipmaps_equal_the_numpy_reference(shape, product_lib):
    tex = random_bytes(shape, 5)
    ref = np_mipmaps(tex)
    count, shapes, offsets, total = level_offsets(shape)
    assert [l.shape for l in ref] == shapes
    dims = np.array(shape[::-1], np.uint32)
    levels, nbytes = C.c_uint32(0), C.c_size_t(0)
    offs = (C.c_size_t * 32)()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert product_lib.ct_generate_mipmaps(p(tex), p(dims), None, 0, C.byref(levels), C.byref(nbytes), offs) == _lib.CT_OK
    assert (levels.value, nbytes.value) == (count, total)
    buf = np.full(total, 0xAB, np.uint8)
    assert product_lib.ct_generate_mipmaps(p(tex), p(dims), p(buf), total - 1, C.byref(levels), C.byref(nbytes), offs) == _lib.CT_E_INVAL
    assert product_lib.ct_generate_mipmaps(p(tex), p(dims), p(buf), total, C.byref(levels), C.byref(nbytes), offs) == _lib.CT_OK
    assert list(offs[:count]) == offsets
    assert np.array_equal(buf, np.concatenate([l.ravel() for l in ref]))
    # ... and the oracle's pyramid, which its descriptors sample
    for a, b in zip(O.generate_mipmaps(tex), ref):
        assert np.array_equal(a, b)


@gpu
@pytest.mark.parametrize("shape", MIP_SHAPES)
def test_device_pyramid_equals_the_numpy_reference(shape):
    tex = random_bytes(shape, 5)
    ref = np_mipmaps(tex)
    count, shapes, offsets, total = level_offsets(shape)
    with tracer(tex) as tr:
        raw, g = tr.layout("mip_pyramid")                      # builds the pyramid: no descriptor call has run
        assert g == {"levels": count, "dims": shape[::-1]} and raw.size == total
        for l in range(count):
            got = raw[offsets[l]:offsets[l] + ref[l].size].reshape(shapes[l])
            assert np.array_equal(got, ref[l]), l
        # the pyramid a descriptor call leaves behind is the same one
        tr.collect_descriptors(np.zeros((1, 3), f32), np.array([[0, 1, 0]], f32))
        assert np.array_equal(tr.layout(_lib.CT_LAYOUT_MIP_PYRAMID)[0], raw)
        n = C.c_size_t(0)
        geom, small = np.zeros(16, np.uint32), np.full(total, 0xAB, np.uint8)
        rc = tr.L.ct_debug_layout(tr.h, _lib.CT_LAYOUT_MIP_PYRAMID, geom.ctypes.data_as(C.c_void_p), small.ctypes.data_as(C.c_void_p),
                                  total - 1, C.byref(n))
        assert rc == _lib.CT_E_INVAL and (small == 0xAB).all()


# ======================================================================================================================
# 2. descriptors
# ======================================================================================================================
def np_descriptors(tex, positions, views, light, cloud_size_m, mean_free_path_m):
    """setupHierarchicalDescriptor<DisneyDescriptor, uint8_t>, DisneyDescriptor.cuh:71-112, in float64: density * 255 BEFORE the
    truncation, [count, 10, 9, 5, 5] (layer, z, y, x).
    Frame: eZ = normalize(-light), eX = normalize(eZ x view), eY = eX x eZ.  Layer l samples origin + (x eX + y eY + z eZ) * scale,
    x, y in -2..2, z in -2..6, scale = 2^l * 0.5 / densityMultiplier (half a free path in box units), at LOD level0 + l with
    level0 = -log2(voxel size in free paths) - 1.  rtTex3DLod is mip-linear over trilinear, clamp-to-edge levels in normalised
    coordinates; the value fades linearly to zero over one mip voxel outside the box (distanceToBox, :47-55)."""
    nz, ny, nx = tex.shape
    dims = np.array([nx, ny, nz], np.float64)
    maxdim = dims.max()
    bbox = dims / maxdim
    pyramid = [l.astype(np.float64) / 255.0 for l in np_mipmaps(tex)]
    light = np.asarray(light, np.float64)
    ez = -light / np.linalg.norm(light)
    views = np.asarray(views, np.float64)
    ex = np.cross(ez[None, :], views)
    ex /= np.linalg.norm(ex, axis=1, keepdims=True)
    ey = np.cross(ex, ez[None, :])
    origin = np.asarray(positions, np.float64) + bbox / 2
    voxel_m = cloud_size_m / maxdim
    level0 = -np.log2(voxel_m / mean_free_path_m) - 1
    gz, gy, gx = np.meshgrid(np.arange(-2, 7), np.arange(-2, 3), np.arange(-2, 3), indexing="ij")
    offsets = (gx[None, ..., None] * ex[:, None, None, None, :] + gy[None, ..., None] * ey[:, None, None, None, :]
               + gz[None, ..., None] * ez[None, None, None, None, :])                                     # [count, 9, 5, 5, 3]

    def level(l, pos):
        t = pyramid[l]
        n = np.array(t.shape[::-1], np.float64)
        c = pos / bbox * n - 0.5                       # normalised coordinate (pos * textureScale) times the level's size
        i0 = np.floor(c)
        w = c - i0
        i0 = i0.astype(np.int64)
        lo = [np.clip(i0[..., a], 0, int(n[a]) - 1) for a in range(3)]
        hi = [np.clip(i0[..., a] + 1, 0, int(n[a]) - 1) for a in range(3)]
        wx, wy, wz = w[..., 0], w[..., 1], w[..., 2]
        out = 0.0
        for z, fz in ((lo[2], 1 - wz), (hi[2], wz)):
            for y, fy in ((lo[1], 1 - wy), (hi[1], wy)):
                for x, fx in ((lo[0], 1 - wx), (hi[0], wx)):
                    out = out + t[z, y, x] * fz * fy * fx
        return out

    out = np.empty((len(origin), 10, 9, 5, 5), np.float64)
    for layer in range(10):
        scale = 0.5 / (cloud_size_m / mean_free_path_m) * 2.0 ** layer
        lod = level0 + layer
        pos = origin[:, None, None, None, :] + offsets * scale
        lc = min(max(lod, 0.0), len(pyramid) - 1.0)
        l0 = int(np.floor(lc))
        w = lc - l0
        density = level(l0, pos)
        if w > 0:
            density = density + w * (level(min(l0 + 1, len(pyramid) - 1), pos) - density)
        mip_voxel = 2.0 ** lod * voxel_m / cloud_size_m
        dist = np.abs(pos - bbox / 2) - np.maximum(bbox / 2 - mip_voxel / 2, 0.0)
        distance = np.linalg.norm(np.maximum(dist, 0.0), axis=-1)
        fade = np.clip(distance / mip_voxel, 0.0, 1.0)
        out[:, layer] = (density * (1 - fade)) * 255.0
    return out


DESC_VOLUMES = {"odd": lambda: sphere((37, 53, 45), 31), "thin": lambda: sphere((8, 48, 20), 32), "dense": lambda: random_bytes((16, 16, 16), 33),
                "cube32": lambda: sphere((32, 32, 32), 34)}
# cloud_size_m, mean_free_path_m.  "coarse": level0 > 0, so the last layers clamp at levels - 1.  "integral": a voxel of exactly four
# free paths, level0 = -3, every layer takes the w == 0 branch (one level fetch).
DESC_SCENES = {"default": lambda maxdim: (7000.0, 10.0), "coarse": lambda maxdim: (30.0, 10.0), "integral": lambda maxdim: (100.0 * maxdim, 25.0)}
DESC_CASES = [(v, s) for v in ("odd", "thin", "dense") for s in ("default", "coarse", "integral")] + [("cube32", "integral")]


def oracle_level0(tex, cloud_size_m, mean_free_path_m):
    """level0 as the oracle and the library compute it: float32, ct_log2f(x) = ct_logf(x) * (1 / ln 2)."""
    voxel_fp = f32(f32(f32(cloud_size_m) / f32(max(tex.shape))) / f32(mean_free_path_m))
    return -f32(f32(O.lib(True).orc_logf(float(voxel_fp))) * f32(1.44269504088896341)) - f32(1)


def rotated(v, angle, seed):
    """The unit vector v turned by `angle` radians towards a random perpendicular, float32."""
    v = np.asarray(v, np.float64) / np.linalg.norm(v)
    r = np.random.default_rng(seed).normal(size=3)
    r -= r.dot(v) * v
    r /= np.linalg.norm(r)
    return (np.cos(angle) * v + np.sin(angle) * r).astype(f32)


def descriptor_samples(vname, sname, lname):
    """24 (position, view) samples: 12 first-scatter samples of the oracle's generator, then points on and just outside the faces
    and corners and at +-0.75, four of them seen from within 1e-3 rad of the light and of its opposite (never exactly parallel)."""
    def make():
        tex = DESC_VOLUMES[vname]()
        size_m, mfp = DESC_SCENES[sname](max(tex.shape))
        light = LIGHTS[lname]
        orc = oracle(tex, cloud_size_m=size_m, mean_free_path_m=mfp, light_direction=light, inscatter="none")
        pos, view = orc.generate_scatter_samples(12, batch_seed=5)
        assert np.isfinite(pos).all()
        hx, hy, hz = half_box(tex.shape)
        out1 = np.nextafter(f32(1), f32(2))
        extra = np.array([(hx, 0.1 * hy, -0.3 * hz), (hx * out1, 0.1 * hy, -0.3 * hz), (0.2 * hx, -hy, 0.4 * hz), (0.2 * hx, -hy - 0.01, 0.4 * hz),
                          (-0.5 * hx, 0.3 * hy, hz), (-0.5 * hx, 0.3 * hy, hz + 0.003), (hx, hy, hz), (-hx * out1, -hy * out1, -hz * out1),
                          (hx + 0.02, -hy - 0.02, hz + 0.02), (0.75, 0.75, 0.75), (-0.75, 0.75, -0.75), (0.0, 0.0, 0.0)], f32)
        rng = np.random.default_rng(9)
        extra_v = rng.normal(size=(12, 3))
        extra_v = (extra_v / np.linalg.norm(extra_v, axis=1, keepdims=True)).astype(f32)
        extra_v[0], extra_v[6] = rotated(light, 9e-4, 1), rotated(light, 3e-4, 2)
        extra_v[3], extra_v[11] = rotated(np.negative(light), 9e-4, 3), rotated(np.negative(light), 3e-4, 4)
        pos, view = np.concatenate([pos, extra]), np.concatenate([view, extra_v])
        ref = orc.collect_descriptors(pos, view)
        for a in (pos, view, ref):
            a.setflags(write=False)
        return pos, view, ref
    return cached(("desc", vname, sname, lname), make)


def test_the_integral_scene_has_an_integral_level0():
    for vname in DESC_VOLUMES:
        tex = DESC_VOLUMES[vname]()
        assert oracle_level0(tex, *DESC_SCENES["integral"](max(tex.shape))) == f32(-3.0), vname
    assert oracle_level0(DESC_VOLUMES["cube32"](), 3200.0, 25.0) == f32(-3.0)
    tex = DESC_VOLUMES["odd"]()
    assert oracle_level0(tex, *DESC_SCENES["coarse"](53)) > 0 and oracle_level0(tex, *DESC_SCENES["default"](53)) < -3


# Share of bytes by which the oracle (float32) may differ from the float64 restatement: twice the share measured over DESC_CASES x
# LIGHTS (see the docstring below); float32 and float64 only disagree where the value sits at a truncation boundary.
DESC_MEASURED_SHARE = 1.125e-4      # 243 of 2 160 000 bytes
# How near an integer the float64 value of a differing byte must be, in byte units.  float32 carries a grid point's position to
# ~2^-22 box units; the fade divides a distance by one mip voxel (>= 2^level0 / maxDim, 7e-4 box units on these scenes) and the
# trilinear weights multiply it by <= 64 texels, so the value moves by < 255 * (2^-22 / 7e-4 + 3 * 64 * 2^-22) < 0.1.  A view at an
# angle t to the light divides the rounding of eZ x view (3 * 2^-24 per component) by sin t before normalising: the frame
# turns by <= 3e-7 / sin t, a grid point at up to 2 sqrt(2) spacings of 2 mip texels moves by 5.7 times that in mip texels, and
# neighbouring texels differ by up to 255: 255 * 3 * 5.7 * 3e-7 / sin t = 1.3e-3 / sin t.
def desc_window(views, light):
    l = np.asarray(light, np.float64) / np.linalg.norm(light)
    v = np.asarray(views, np.float64)
    sin_t = np.linalg.norm(np.cross(l[None, :], v), axis=1) / np.linalg.norm(v, axis=1)
    return 0.1 + 1.3e-3 / sin_t


def desc_compare(vname, sname, lname):
    """-> (differing bytes, bytes, largest |difference|, differing bytes whose float64 value is not next to an integer)."""
    tex = DESC_VOLUMES[vname]()
    size_m, mfp = DESC_SCENES[sname](max(tex.shape))
    pos, view, ref = descriptor_samples(vname, sname, lname)
    v64 = np_descriptors(tex, pos, view, LIGHTS[lname], size_m, mfp)
    want = np.floor(v64).astype(np.int64)
    diff = ref.astype(np.int64) - want
    to_integer = np.abs(v64 - np.rint(v64))
    window = desc_window(view, LIGHTS[lname])[:, None, None, None, None]
    return int((diff != 0).sum()), diff.size, int(np.abs(diff).max()), int(((diff != 0) & (to_integer > window)).sum()), ref


def test_oracle_descriptors_against_the_float64_restatement():
    """The oracle's bytes over DESC_CASES x LIGHTS x 24 samples against floor(np_descriptors): no byte differs by more than 1, a
    differing byte's float64 value lies next to an integer (desc_window), and the share of differing bytes stays below twice
    the share measured when this test was written.
    Measured (x86-64, the oracle's FMA build): 243 of 2 160 000 bytes differ, each by 1, a share of 1.125e-4 -- none at all on most
    sphere cases, up to 42 of 54 000 on the dense random volume, whose neighbouring texels differ most."""
    differing = total = 0
    for vname, sname in DESC_CASES:
        for lname in LIGHTS:
            d, n, worst, far, ref = desc_compare(vname, sname, lname)
            print(f"{vname:7s} {sname:9s} {lname:8s} differing {d:6d} of {n}  max |diff| {worst}  not at a boundary {far}  nonzero {(ref > 0).mean():.3f}")
            assert worst <= 1 and far == 0, (vname, sname, lname)
            assert ref.any()
            differing += d
            total += n
    share = differing / total
    print(f"share of differing bytes {share:.3e}")
    assert share <= 2 * DESC_MEASURED_SHARE


def parallel_views(orc):
    """Six samples at the box's centre.  0, 1, 2: views exactly antiparallel, parallel and (twice as long) antiparallel to the light
    -- to eZ as the frame computes it, normalize(-light) in float32 in optix::normalize's operation order, so that eZ x view is
    exactly zero; 4, 5: a NaN view and an infinite position; 3: an ordinary sample between them."""
    a = -orc.derived_uniforms()[7:10].astype(f32)
    inv = f32(1) / np.sqrt(f32(f32(a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]))
    ez = (a * inv).astype(f32)
    assert not np.cross(ez.astype(np.float64), (f32(2) * ez).astype(np.float64)).any()
    pos = np.zeros((6, 3), f32)
    pos[5] = (np.inf, 0, 0)
    return pos, np.array([ez, -ez, f32(2) * ez, (0, 1, 0.5), (np.nan, 0, 1), (0, 1, 0.5)], f32)


def test_oracle_descriptor_of_a_view_parallel_to_the_light_is_all_zero():
    """eX = normalize(0): no frame, no grid point, 2250 zero bytes by definition (include/cloudtrace.h) -- and the same for a
    sample whose position or view is not finite.  The sample next to them in the batch is not disturbed."""
    tex = DESC_VOLUMES["dense"]()
    for lname, light in LIGHTS.items():
        orc = oracle(tex, light_direction=light, inscatter="none")
        pos, view = parallel_views(orc)
        got = orc.collect_descriptors(pos, view)
        assert not got[[0, 1, 2, 4, 5]].any(), lname
        assert got[3].any() and np.array_equal(got[3], orc.collect_descriptors(pos[3:4], view[3:4])[0])


@gpu
@pytest.mark.parametrize("vname,sname", DESC_CASES)
def test_descriptors_bit_exact_over_volumes_scenes_and_lights(vname, sname):
    tex = DESC_VOLUMES[vname]()
    size_m, mfp = DESC_SCENES[sname](max(tex.shape))
    for lname, light in LIGHTS.items():
        pos, view, ref = descriptor_samples(vname, sname, lname)
        with tracer(tex, cloud_size_m=size_m, mean_free_path_m=mfp, light_direction=light) as tr:
            got = tr.collect_descriptors(pos, view)
        assert np.array_equal(got, ref), lname
        assert got[:12].any()


@gpu
@pytest.mark.parametrize("vname", ["odd", "thin", "dense"])
def test_descriptors_after_set_light_use_the_new_frame_and_the_old_pyramid(vname):
    tex = DESC_VOLUMES[vname]()
    size_m, mfp = DESC_SCENES["default"](max(tex.shape))
    with tracer(tex, cloud_size_m=size_m, mean_free_path_m=mfp) as tr:
        pos, view, ref = descriptor_samples(vname, "default", "default")
        assert np.array_equal(tr.collect_descriptors(pos, view), ref)        # the pyramid exists from here on
        pyramid = tr.layout("mip_pyramid")[0]
        for lname in ("down", "x", "oblique", "default"):
            tr.set_light(LIGHTS[lname])
            pos, view, ref = descriptor_samples(vname, "default", lname)
            assert np.array_equal(tr.collect_descriptors(pos, view), ref), lname
        assert np.array_equal(tr.layout("mip_pyramid")[0], pyramid)


@gpu
def test_descriptor_of_a_view_parallel_to_the_light_is_all_zero_on_gpu():
    tex = DESC_VOLUMES["dense"]()
    for lname, light in LIGHTS.items():
        orc = oracle(tex, light_direction=light, inscatter="none")
        pos, view = parallel_views(orc)
        with tracer(tex, light_direction=light) as tr:
            got = tr.collect_descriptors(pos, view)
        assert not got[[0, 1, 2, 4, 5]].any() and got[3].any(), lname
        assert np.array_equal(got, orc.collect_descriptors(pos, view)), lname


# ======================================================================================================================
# 3. scatter samples
# ======================================================================================================================
def corner_blob():
    """(48, 20, 28): a blob of radius 3 texels (<= 1/6 of the shortest side) in one corner; most rays miss it or pass through."""
    def make():
        z, y, x = np.mgrid[0:48, 0:20, 0:28].astype(np.float32)
        r = np.sqrt((x - 22.5) ** 2 + (y - 4.5) ** 2 + (z - 5.5) ** 2)
        return (np.clip(1.0 - r / 3.0, 0.0, 1.0) * 90).astype(np.uint8)
    return cached("corner_blob", make)


def one_texel():
    def make():
        t = np.zeros((16, 16, 16), np.uint8)
        t[9, 4, 11] = 255
        return t
    return cached("one_texel", make)


SCATTER_VOLUMES = {"blob": corner_blob, "dense": lambda: random_bytes((9, 7, 11), 41), "texel": one_texel}
SCATTER_COUNTS = (1, 63, 64, 65, 130)
SCATTER_SEEDS = (0, 77, 0xFFFFFFF0)             # the last: batch_seed + attempt wraps after 16 attempts


def scatter_reference(vname, seed):
    """The oracle's 130 samples; sample i does not depend on the count, so the shorter calls compare with a prefix."""
    def make():
        pos, d = oracle(SCATTER_VOLUMES[vname](), inscatter="none").generate_scatter_samples(max(SCATTER_COUNTS), seed)
        return np.concatenate([pos, d], axis=1)
    return cached(("scatter", vname, seed), make)


def check_scatter_properties(tex, pos, d, step=1.0 / 512.0):
    """What holds for a finite sample whatever produced it: the view is a unit vector; the position passes isInBox (cloud.cuh:40-44,
    0.01 of slack); and there is density where the flight collided -- getNextScatteringEvent (cloud.cuh:77-114) steps back from
    the sample point that collided by log(xi / T) / density <= one step, so the sample point is within a step ahead of the position
    (where the ray enters a footprint the position itself can lie just before the first non-zero texel weight)."""
    finite = np.isfinite(pos).all(axis=1)
    assert np.array_equal(finite, np.isfinite(d).all(axis=1)) and not np.isnan(pos[finite]).any()
    h = half_box(tex.shape)
    p, v = pos[finite].astype(np.float64), d[finite].astype(np.float64)
    assert np.all(np.abs(np.linalg.norm(v, axis=1) - 1) <= 1e-5)
    assert np.all(np.abs(p) <= h + 0.01 + 1e-6)
    for a, b in zip(p, v):
        dens = max(O.tex3d(tex, a + h + b * t) for t in np.linspace(0.0, step * 1.001, 9))
        assert dens > 0, (a, b)
    return int(finite.sum())


@pytest.mark.parametrize("vname", list(SCATTER_VOLUMES))
def test_oracle_scatter_samples_have_the_properties(vname):
    tex = SCATTER_VOLUMES[vname]()
    for seed in SCATTER_SEEDS:
        ref = scatter_reference(vname, seed)
        assert check_scatter_properties(tex, ref[:, :3], ref[:, 3:]) == len(ref)      # nothing runs out of attempts on these


@gpu
@pytest.mark.parametrize("vname", list(SCATTER_VOLUMES))
def test_scatter_samples_bit_exact_at_the_wave_edges_and_a_wrapping_seed(vname):
    tex = SCATTER_VOLUMES[vname]()
    with tracer(tex) as tr:
        for seed in SCATTER_SEEDS:
            ref = scatter_reference(vname, seed)
            for count in SCATTER_COUNTS:
                pos, d = tr.generate_scatter_samples(count, seed)
                assert np.concatenate([pos, d], axis=1).tobytes() == ref[:count].tobytes(), (seed, count)
                if count == max(SCATTER_COUNTS):
                    check_scatter_properties(tex, pos, d)


@gpu
def test_scatter_samples_of_an_empty_volume_stay_nan():
    tex = np.zeros((16, 16, 16), np.uint8)
    want = np.full((3, 3), 0x7FC00000, np.uint32)
    with tracer(tex, sample_step=1.0 / 64.0) as tr:
        pos, d = tr.generate_scatter_samples(3, 77)                  # CT_OK: 4096 attempts each, none scatters
    assert np.array_equal(pos.view(np.uint32), want) and np.array_equal(d.view(np.uint32), want)
    rp, rd = oracle(tex, sample_step=1.0 / 64.0, inscatter="none").generate_scatter_samples(3, 77)
    assert pos.tobytes() == rp.tobytes() and d.tobytes() == rd.tobytes()


def test_oracle_scatter_samples_of_an_empty_volume_stay_nan():
    rp, rd = oracle(np.zeros((16, 16, 16), np.uint8), sample_step=1.0 / 64.0, inscatter="none").generate_scatter_samples(3, 77)
    assert np.isnan(rp).all() and np.isnan(rd).all()


@gpu
@pytest.mark.parametrize("kind", ["delta", "sparse", "simple"])
def test_scatter_samples_do_not_depend_on_the_handle_kind(kind):
    """The header: a DELTA handle makes the same march flight."""
    for vname, seed in (("blob", 77), ("dense", 0xFFFFFFF0)):
        tex = SCATTER_VOLUMES[vname]()
        ref = scatter_reference(vname, seed)
        with tracer(tex, **KINDS[kind]) as tr:
            pos, d = tr.generate_scatter_samples(65, seed)
        assert np.concatenate([pos, d], axis=1).tobytes() == ref[:65].tobytes(), vname


# ======================================================================================================================
# 4. point radiance
# ======================================================================================================================
POINT_VOLUMES = {"sphere": lambda: sphere((36, 52, 44), 51), "dense": lambda: random_bytes((9, 7, 11), 52),
                 "empty": lambda: cached("empty", lambda: np.zeros((12, 16, 20), np.uint8))}
THICK = dict(mean_free_path_m=0.5, max_depth=8)
# volume, mode, kind, count, launches, scene: every mode, kind, count and number of launches at least twice
POINT_CASES = [
    ("sphere", 0, "march", 65, 9, {}),
    ("sphere", 1, "delta", 257, 8, {}),
    ("sphere", 2, "sparse", 1000, 1, {}),
    ("dense", 0, "delta", 64, 40, dict(cloud_size_m=40.0)),
    ("dense", 1, "sparse", 1, 8, dict(cloud_size_m=40.0)),
    ("dense", 2, "march", 257, 9, dict(cloud_size_m=40.0)),
    ("empty", 0, "sparse", 1000, 1, {}),
    ("empty", 1, "march", 1, 40, {}),
    ("empty", 2, "delta", 64, 1, {}),
    ("sphere", 0, "march", 65, 9, THICK),
    ("dense", 1, "delta", 64, 40, dict(cloud_size_m=40.0, **THICK)),
    ("sphere", 1, "sparse", 130, 8, THICK),
]


def point_rays(shape, n, seed):
    """n rays: random ones from inside the box and, from the second on, the contrived ones."""
    hx, hy, hz = half_box(shape)
    rng = np.random.default_rng(seed)
    pos = ((rng.random((n, 3)) - 0.5) * 1.6 * np.array([hx, hy, hz])).astype(f32)
    d = rng.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
    special = [
        ((hx, 0.1 * hy, 0.05 * hz), (-1, 0.2, 0.1)), ((hx, 0.1 * hy, 0.05 * hz), (1, 0.2, 0.1)),            # on a face: in, out
        ((-0.2 * hx, -hy, 0.3 * hz), (0.1, 1, 0.1)), ((0.3 * hx, 0.2 * hy, hz), (0.1, -0.3, 1)),
        ((hx, hy, 0.1 * hz), (-1, -1, 0.1)), ((hx, hy, 0.1 * hz), (1, 1, 0)),                               # on an edge
        ((hx, hy, hz), (-1, -1, -1)), ((hx, hy, hz), (1, 1, 1)), ((-hx, -hy, -hz), (1, 0.5, 0.25)),         # on a corner
        ((2, 0.01, 0.02), (-1, 0, 0)), ((0.01, -2, 0.02), (0, 1, 0)), ((0.01, 0.02, 2), (0, 0, -1)),        # along each axis exactly
        ((0.02, 0.01, -0.03), (0, 0, 1)),
        ((2, hy, hz), (-1, 0, 0)), ((2, hy * (1 - 1e-6), -hz * (1 - 1e-6)), (-1, 0, 0)),                    # grazing an edge
        ((2 * hx, 2 * hy, 0), (-1, -1, 0.001)),
        ((0.1 * hx, 0.1 * hy, 0.1 * hz), (6e-4, -5e-4, 6e-4)), ((2, 0, 0), (-1e3, 10, 5)),                  # |direction| 1e-3, 1e3
        ((50, 0.1 * hy, -0.1 * hz), (-1, -0.002 * hy, 0.002 * hz)), ((0, 50, 0), (0, -1, 0)),               # far away
        ((3, 0, 0), (1, 0, 0)),                                                                             # misses
    ]
    for i, (p, v) in enumerate(special):
        if 1 + i < n:
            pos[1 + i], d[1 + i] = p, v
    return pos, d


def point_pair(vname, mode, kind, scene):
    tex = POINT_VOLUMES[vname]()
    kw = dict(mode=mode, **KINDS[kind], **scene)
    return tracer(tex, **kw), oracle(tex, **kw)


def same_point_counters(tr, orc):
    c, o = tr.counters(), orc.counters.as_dict()
    for k in ("density_lookups", "scatter_events", "depth_capped"):
        assert c[k] == o[k], k
    return c


@gpu
@pytest.mark.parametrize("vname,mode,kind,count,launches,scene", POINT_CASES)
def test_point_radiance_bit_exact_over_volumes_modes_and_handle_kinds(vname, mode, kind, count, launches, scene):
    pos, d = point_rays(POINT_VOLUMES[vname]().shape, count, seed=count + launches)
    tr, orc = point_pair(vname, mode, kind, scene)
    with tr:
        got = tr.point_radiance_launch(ds.make_point_tasks(pos, d), 3, launches)
        ref = orc.point_radiance_launch(ds.make_point_tasks(pos, d), 3, launches)
        assert got.tobytes() == ref.tobytes()
        assert np.all(got["experimentCount"] == launches)
        c = same_point_counters(tr, orc)
        if vname == "empty":
            assert not got["radiance"].any() and c["scatter_events"] == 0
        elif count >= 64:
            assert c["scatter_events"] > 0 and (got["radiance"].any() or "max_depth" in scene)
        if "max_depth" in scene and mode != 2:
            assert c["depth_capped"] > 0


@gpu
@pytest.mark.parametrize("vname,kind", [("sphere", "march"), ("dense", "delta")])
def test_point_radiance_tasks_that_arrive_with_state(vname, kind):
    """experimentCount 1 and 2^24 - 3 with a mean and an M2: five launches take the second across 2^24, where (float)N stops being
    exact and the weight (float)(1.0 / (double)N) repeats."""
    shape = POINT_VOLUMES[vname]().shape
    pos, d = point_rays(shape, 65, seed=7)
    tr, orc = point_pair(vname, 1, kind, dict(cloud_size_m=40.0) if vname == "dense" else {})
    tasks = ds.make_point_tasks(pos, d)
    tasks["experimentCount"] = np.where(np.arange(65) % 2 == 0, 1, 2 ** 24 - 3)
    tasks["radiance"] = np.random.default_rng(3).random(65, dtype=f32) * 40 + f32(0.37)
    tasks["runningVariance"] = np.random.default_rng(4).random(65, dtype=f32) * 1e4 + f32(2.5)
    with tr:
        got = tr.point_radiance_launch(tasks.copy(), 11, 5)
        ref = orc.point_radiance_launch(tasks.copy(), 11, 5)
        assert got.tobytes() == ref.tobytes()
        assert sorted(set(got["experimentCount"].tolist())) == [6, 2 ** 24 + 2]
        assert not np.array_equal(got["radiance"], tasks["radiance"])
        same_point_counters(tr, orc)


def np_fold(results):
    """PointRadianceTask::addExperimentResult (PointRadianceTask.h:40-51) over results[k] (float32 [K, n]) from zero state, every
    operation rounded to float32 in the reference's order; newWeight = (float)(1.0 / (double)(float)N)."""
    rad = np.zeros(results.shape[1], f32)
    var = np.zeros(results.shape[1], f32)
    for k, x in enumerate(results):
        n = f32(k + 1)
        weight = f32(1.0 / np.float64(n))
        prev = rad
        rad = prev + (x - prev) * weight
        var = var + (x - prev) * (x - rad)
    return rad, var


@gpu
@pytest.mark.parametrize("launches", [9, 40])
@pytest.mark.parametrize("estimator", [MARCH, DELTA])
def test_point_radiance_fold_and_job_cutting_without_the_oracle(estimator, launches, monkeypatch):
    """K calls of one launch on fresh tasks give the K frames' results (the mean of one sample is the sample); folded here, they must
    be, bit for bit, what one call of K launches returns -- however that call was cut into jobs: single frames from one queue, or
    (CT_POINT_ORDER=0) jobs of 8 frames and a remainder over 8 queues."""
    tex = POINT_VOLUMES["sphere"]()
    first = 21
    for count in (65, 257):
        pos, d = point_rays(tex.shape, count, seed=count)
        with tracer(tex, mode=1, estimator=estimator) as single, tracer(tex, mode=1, estimator=estimator) as whole:
            monkeypatch.setenv("CT_POINT_ORDER", "0")
            with tracer(tex, mode=1, estimator=estimator) as chunked:
                monkeypatch.delenv("CT_POINT_ORDER")
                frames = np.stack([single.point_radiance_launch(ds.make_point_tasks(pos, d), first + k, 1)["radiance"]
                                   for k in range(launches)])
                assert frames.dtype == f32 and np.isfinite(frames).all() and frames.any()
                rad, var = np_fold(frames)
                for tr in (whole, chunked):
                    got = tr.point_radiance_launch(ds.make_point_tasks(pos, d), first, launches)
                    assert got["radiance"].tobytes() == rad.tobytes()
                    assert got["runningVariance"].tobytes() == var.tobytes()
                    assert np.all(got["experimentCount"] == launches)
                    assert tr.counters() == single.counters()


def test_np_fold_on_a_case_done_by_hand():
    rad, var = np_fold(np.array([[1.0], [2.0], [6.0]], f32))
    assert rad[0] == f32(3.0) and var[0] == f32(14.0)            # mean 3, M2 = 4 + 1 + 9


@gpu
def test_point_radiance_refuses_rays_that_are_zero_or_not_finite():
    tex = POINT_VOLUMES["sphere"]()
    pos, d = point_rays(tex.shape, 65, seed=1)
    with tracer(tex, mode=1) as tr:
        for bad in ((0, 0, 0), (np.nan, 0, 1), (np.inf, 0, 0), (0, -np.inf, 1)):
            tasks = ds.make_point_tasks(pos, d)
            tasks["direction"][64] = bad
            before = tasks.copy()
            with pytest.raises(_lib.CloudTraceError) as e:
                tr.point_radiance_launch(tasks, 1, 2)
            assert e.value.code == _lib.CT_E_INVAL and "task 64" in e.value.message
            assert tasks.tobytes() == before.tobytes()
        tasks = ds.make_point_tasks(pos, d)
        tasks["position"][5] = (np.nan, 0, 0)
        with pytest.raises(_lib.CloudTraceError) as e:
            tr.point_radiance_launch(tasks, 1, 2)
        assert e.value.code == _lib.CT_E_INVAL and "task 5" in e.value.message
        assert tr.counters()["paths"] == 0
        # the handle is as it was
        got = tr.point_radiance_launch(ds.make_point_tasks(pos, d), 1, 2)
        ref = oracle(tex, mode=1).point_radiance_launch(ds.make_point_tasks(pos, d), 1, 2)
        assert got.tobytes() == ref.tobytes()
