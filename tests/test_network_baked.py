"""ct_network_bake / ct_baked_render_*: the scattering network baked into a probe table and rendered from it
(include/cloudtrace.h, "the network baked into a probe table").

Everything is compared BIT FOR BIT unless a bound is stated: the table against Network.eval on collect_descriptors of the bake's
own probes, the lookup against network.bake_lookup_reference (numpy float32), a frame against the numpy composition of
descriptor_frame's records, that reference and render_values, the fused accumulation against the loop.

Scene and weights: those of tests/test_network_render.py -- make_procedural_cloud(64), 24 x 16, the default pose, the seeded
(32, 1, 1) and (200, 1, 3) weights and their negated last layer.

The azimuth is periodic: t = 0 and t = 4 are the same direction, and the node j = 0 of a frame that is not axis-aligned has
py = u . b of the size of a rounding error, of either sign.  Where a test holds an azimuth to a node's t_j it therefore measures
min(|dt|, 4 - |dt|); the CPU test uses an axis-aligned frame, where py is exactly 0, and the plain distance."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import deepestscatter_amd as ds
from deepestscatter_amd import _lib
from deepestscatter_amd import network as N
from test_network_render import FLAGSHIP, H, LIGHT2, SCALE, SID, SMALL, W, cloud, weights

GRID_A = ((5, 4, 3), 8, 3)      # the small network's table
GRID_B = ((3, 3, 3), 4, 2)      # the (200, 1, 3) network's


def node_directions(nphi, a, b):
    """u_j of the definition for j < nphi, in float64, rounded once."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    out = []
    for j in range(nphi):
        t = j / (nphi // 4)
        p = 1 - t if t <= 2 else t - 3
        q = 1 - abs(p) if t <= 2 else -(1 - abs(p))
        u = p * a + q * b
        out.append(u / np.sqrt((u * u).sum()))
    return np.array(out).astype(np.float32)


def circular(t, want):
    d = np.abs(t.astype(np.float64) - want)
    return np.minimum(d, 4 - d)


# ---------------------------------------------------------------------------------------------------- CPU
def test_symbols_resolve_and_answer_null_arguments(product_lib):
    names = ["ct_network_bake", "ct_bake_update", "ct_bake_destroy", "ct_bake_info", "ct_bake_probes", "ct_bake_download",
             "ct_debug_bake_lookup", "ct_baked_render_subframe", "ct_baked_render_accumulate", "ct_baked_render_shard_subframe",
             "ct_baked_render_shard_accumulate", "ct_debug_baked_render_time"]
    for name in names:
        assert hasattr(product_lib, name) and name in _lib.EXPORTS
    L = product_lib
    p = _lib.CtNetworkRender(_lib.CT_ABI_VERSION, _lib.CT_NET_OUT_LINEAR, (C.c_float * 3)(1, 1, 1), 0)
    d = _lib.CtBakeDesc(_lib.CT_ABI_VERSION, (C.c_uint32 * 3)(2, 2, 2), 4, 2)
    out = C.c_void_p()
    assert L.ct_network_bake(None, None, C.byref(d), C.byref(out)) == _lib.CT_E_INVAL
    assert L.ct_network_bake(None, None, None, None) == _lib.CT_E_INVAL
    assert L.ct_bake_update(None, None, None) == _lib.CT_E_INVAL
    assert L.ct_bake_destroy(None) == _lib.CT_OK
    assert L.ct_bake_info(None, None) == _lib.CT_E_INVAL
    assert L.ct_bake_probes(None, 0, 0, None, None) == _lib.CT_E_INVAL
    assert L.ct_bake_download(None, None, 0) == _lib.CT_E_INVAL
    assert L.ct_debug_bake_lookup(None, None, None, None, 0, None) == _lib.CT_E_INVAL
    for entry in (L.ct_baked_render_subframe, L.ct_baked_render_shard_subframe):
        assert entry(None, None, C.byref(p), 1, None) == _lib.CT_E_INVAL
        assert entry(None, None, None, 1, None) == _lib.CT_E_INVAL
    for entry in (L.ct_baked_render_accumulate, L.ct_baked_render_shard_accumulate):
        assert entry(None, None, C.byref(p), 1, 1) == _lib.CT_E_INVAL
        assert entry(None, None, None, 1, 1) == _lib.CT_E_INVAL
    assert L.ct_debug_baked_render_time(None, None) == _lib.CT_E_INVAL
    assert C.sizeof(_lib.CtBakeDesc) == 24 and C.sizeof(_lib.CtBakeInfo) == 344
    assert _lib.CtBakeInfo.entries.offset == 24 and _lib.CtBakeInfo.cosine.offset == 68 and _lib.CtBakeInfo.gather_ms.offset == 328


def frame_info(grid, nphi, nc, light=(0, 0, 1), a=(1, 0, 0), b=(0, 1, 0)):
    return {"grid": grid, "azimuths": nphi, "cosines": nc, "entries": int(np.prod(grid)) * nphi * nc,
            "light": np.array(light, np.float32), "axis_a": np.array(a, np.float32), "axis_b": np.array(b, np.float32)}


def test_reference_lookup_of_a_constant_table_is_the_constant():
    rng = np.random.default_rng(5)
    info = frame_info((4, 3, 5), 8, 3)
    table = np.full(info["entries"], np.float32(0.37))
    pos = rng.uniform(-0.8, 0.8, (200, 3)).astype(np.float32)           # inside and outside the box
    d = rng.normal(size=(200, 3))
    d = (d / np.sqrt((d * d).sum(axis=1, keepdims=True))).astype(np.float32)
    d[:2] = [[0, 0, 1], [0, 0, -1]]                                      # along the light: t = 0
    got = N.bake_lookup_reference(table, info, (1.0, 0.75, 0.5), pos, d)
    assert got.dtype == np.float32 and got.shape == (200,) and np.all(got == np.float32(0.37))


def test_the_azimuth_of_every_node_direction_is_its_node():
    for nphi in (4, 8, 16, 64):
        u = node_directions(nphi, (1, 0, 0), (0, 1, 0))
        t = N.bake_azimuth(u, (1, 0, 0), (0, 1, 0))
        want = np.arange(nphi) / (nphi // 4)
        err = np.abs(t.astype(np.float64) - want).max()
        print(f"azimuths {nphi}: largest |t(u_j) - t_j| = {err:.3g}")
        assert t.dtype == np.float32 and err <= 1e-6
    # a frame that is not axis-aligned: the same, up to the period
    a = np.array([2.0, -1.0, 0.5])
    a /= np.sqrt((a * a).sum())
    b = np.cross([0.3, 0.4, -1.0], a)
    b /= np.sqrt((b * b).sum())
    for nphi in (4, 8, 16, 64):
        t = N.bake_azimuth(node_directions(nphi, a, b), a.astype(np.float32), b.astype(np.float32))
        assert circular(t, np.arange(nphi) / (nphi // 4)).max() <= 1e-6
    # s == 0 and a direction that is not finite give t = 0
    assert np.all(N.bake_azimuth(np.array([[0, 0, 1], [np.inf, 0, 0], [np.nan, 1, 0]], np.float32), (1, 0, 0), (0, 1, 0)) == 0)


# ---------------------------------------------------------------------------------------------------- GPU
def small_net(tr, negated=False):
    return N.Network(tr, weights(SMALL, negated), 32, 1, 1)


@pytest.fixture(scope="module")
def scene():
    """The module's tracer as it is created (default pose and light, nothing accumulated), its small network with the negated one
    and their (5, 4, 3) x 8 x 3 bakes.  No test changes its light or accumulates on it."""
    with ds.CloudTracer(cloud(), width=W, height=H) as tr:
        made = []
        try:
            s = {"tr": tr}
            for key, negated in (("net", False), ("neg", True)):
                s[key] = small_net(tr, negated)
                made.append(s[key])
                s["bake_" + key] = tr.network_bake(s[key], *GRID_A)
                made.append(s["bake_" + key])
            yield s
        finally:
            for obj in reversed(made):
                obj.close()


def box_of(tr):
    d = np.array(tr.dims, np.float32)
    return d / d.max()


def table_by_definition(tr, net, bake):
    """Network.eval(collect_descriptors(probes), aux = cosine[k]) for every polar node -> the table's shape."""
    import torch
    info = bake.info
    pos, d = bake.probes()
    desc = torch.from_numpy(tr.collect_descriptors(pos, d)).cuda()
    n = len(pos)
    out = torch.empty((n,), dtype=torch.float32, device=desc.device)
    cols = []
    for c in info["cosine"]:
        aux = torch.full((n,), float(c), dtype=torch.float32, device=desc.device)
        torch.cuda.synchronize()
        net.eval(desc.data_ptr(), aux.data_ptr(), n, out.data_ptr())
        cols.append(out.cpu().numpy().copy())
    nx, ny, nz = info["grid"]
    return np.stack(cols, axis=1).reshape(nz, ny, nx, info["azimuths"], info["cosines"])


@pytest.mark.gpu
def test_probes_are_the_grid_of_the_definition(scene):
    tr, bake = scene["tr"], scene["bake_net"]
    info = bake.info
    (nx, ny, nz), nphi, nc = GRID_A
    assert info["grid"] == (nx, ny, nz) and info["azimuths"] == nphi and info["cosines"] == nc and info["entries"] == nx * ny * nz * nphi * nc
    assert info["current"] and info["gather_ms"] > 0 and info["network_ms"] > 0
    l, a, b = (info[k].astype(np.float64) for k in ("light", "axis_a", "axis_b"))
    assert np.array_equal(info["light"], tr.light_direction())
    for u, v in ((a, b), (a, l), (b, l)):
        assert abs(np.dot(u, v)) <= 1e-6
    for u in (a, b, l):
        assert abs(np.dot(u, u) - 1) <= 1e-6
    pos, d = bake.probes()
    assert pos.shape == d.shape == (nx * ny * nz * nphi, 3)
    box = box_of(tr).astype(np.float64)
    idx = np.arange(len(pos))
    j, x, y, z = idx % nphi, idx // nphi % nx, idx // (nphi * nx) % ny, idx // (nphi * nx * ny)
    want = np.stack([-box[0] / 2 + box[0] * x / (nx - 1), -box[1] / 2 + box[1] * y / (ny - 1), -box[2] / 2 + box[2] * z / (nz - 1)], axis=1)
    assert np.all(np.abs(pos.astype(np.float64) - want) <= 2 * np.spacing(np.abs(want).astype(np.float32)))
    d64 = d.astype(np.float64)
    assert np.abs((d64 * d64).sum(axis=1) - 1).max() <= 1e-6 and np.abs(d64 @ l).max() <= 1e-6
    assert circular(N.bake_azimuth(d, info["axis_a"], info["axis_b"]), j / (nphi // 4)).max() <= 1e-6
    assert info["cosine"][0] == -1 and info["cosine"][-1] == 1 and np.array_equal(info["cosine"], np.array([-1, 0, 1], np.float32))
    part = bake.probes(7, 11)                                       # a range is the same floats
    assert np.array_equal(part[0], pos[7:18]) and np.array_equal(part[1], d[7:18])


@pytest.mark.gpu
def test_table_is_the_network_on_the_probes(scene, monkeypatch):
    tr = scene["tr"]
    want = table_by_definition(tr, scene["net"], scene["bake_net"])
    got = scene["bake_net"].table()
    assert got.shape == (3, 4, 5, 8, 3) and np.array_equal(got, want)
    assert np.ptp(got) > 0 and np.isfinite(got).all()
    assert np.array_equal(scene["bake_neg"].table(), -want)        # the negated last layer negates every output exactly
    with N.Network(tr, weights(FLAGSHIP), 200, 1, 3) as net, tr.network_bake(net, *GRID_B) as bake:
        assert np.array_equal(bake.table(), table_by_definition(tr, net, bake))
    # in pieces of 16 records (480 probes: 30 pieces), and with fixed-point texture weights
    monkeypatch.setenv("CT_NET_DESC_RECORDS", "16")
    with ds.CloudTracer(cloud(), width=W, height=H) as t2, small_net(t2) as net, t2.network_bake(net, *GRID_A) as bake:
        assert t2.network_scratch()["desc_cap"] == 16
        assert np.array_equal(bake.table(), want)
    monkeypatch.delenv("CT_NET_DESC_RECORDS")
    with ds.CloudTracer(cloud(), width=W, height=H, flags=_lib.CT_FLAG_TEX_FIXED8) as t3, small_net(t3) as net, \
            t3.network_bake(net, *GRID_A) as bake:
        fixed = bake.table()
        assert np.array_equal(fixed, table_by_definition(t3, net, bake)) and not np.array_equal(fixed, want)


def lookup_inputs(info, box):
    """Synthetic records that reach every edge of the lookup -> (positions, directions, {case: mask})."""
    rng = np.random.default_rng(11)
    nx, ny, nz = info["grid"]
    nphi, nc = info["azimuths"], info["cosines"]
    l, a, b = (info[k].astype(np.float64) for k in ("light", "axis_a", "axis_b"))
    box = box.astype(np.float64)
    pos, d = [], []
    nodes = [np.array([-box[k] / 2 + box[k] * i / (n - 1) for i in range(n)]) for k, n in enumerate((nx, ny, nz))]
    ang = rng.uniform(0, 2 * np.pi, 64)
    cs = rng.uniform(-0.95, 0.95, 64)
    views = [np.cos(t) * np.sqrt(1 - c * c) * a + np.sin(t) * np.sqrt(1 - c * c) * b + c * l for t, c in zip(ang, cs)]
    # the wrap cell: azimuths just below a full turn
    views += [np.cos(t) * 0.8 * a + np.sin(t) * 0.8 * b + 0.6 * l for t in (-0.05, -0.2, -0.01)]
    # along the light (d . l = +-1: fc at both clamps, no azimuth left but rounding noise), beyond the unit length, which passes the
    # clamps, and the null direction, whose s is 0 (t = 0)
    views += [l, -l, 1.5 * l, -1.5 * l, 0 * l]
    views += list(node_directions(nphi, a, b).astype(np.float64))          # on the azimuth nodes
    n_views = len(views)
    for i in range(400):
        v = views[i % n_views]
        if i < 60:
            p = np.array([nodes[k][rng.integers(len(nodes[k]))] for k in range(3)])     # on nodes
        elif i < 300:
            p = rng.uniform(-0.5, 0.5, 3) * box                                          # between nodes
        else:
            p = rng.uniform(-0.5, 0.5, 3) * box                                          # outside the box, each side of each axis
            axis, side = (i // 2) % 3, i % 2
            p[axis] = (0.5 + rng.uniform(0.01, 0.4)) * box[axis] * (1 if side else -1)
        pos.append(p)
        d.append(v)
    return np.array(pos, np.float32), np.array(d, np.float32)


@pytest.mark.gpu
def test_lookup_equals_its_numpy_definition(scene):
    import torch
    tr, bake = scene["tr"], scene["bake_net"]
    info, box = bake.info, box_of(tr)
    table = bake.table()
    pos, d = lookup_inputs(info, box)
    # every case occurs among the inputs (measured with the definition's own float32 arithmetic)
    f32 = np.float32
    (nx, ny, nz), nphi, nc = info["grid"], info["azimuths"], info["cosines"]
    for axis, n in enumerate((nx, ny, nz)):
        f = (pos[:, axis] + f32(0.5) * box[axis]) * f32(f32(n - 1) / box[axis])
        assert (f < 0).any() and (f > n - 1).any()                                   # outside on each side
        assert ((f > 0) & (f < n - 1) & (f != np.floor(f))).any()                    # between nodes
    on_node = np.ones(len(pos), bool)
    for axis, n in enumerate((nx, ny, nz)):
        f = (pos[:, axis].astype(np.float64) + 0.5 * box[axis]) * (n - 1) / box[axis]
        on_node &= np.abs(f - np.round(f)) < 1e-5
    assert on_node.sum() >= 50
    l = info["light"]
    c = (d[:, 0] * l[0] + d[:, 1] * l[1]) + d[:, 2] * l[2]
    fc = (c + f32(1)) * f32(f32(0.5) * f32(nc - 1))
    assert (fc <= 0).any() and (fc >= nc - 1).any() and (fc < 0).any() and (fc > nc - 1).any()      # both clamps, reached and passed
    t = N.bake_azimuth(d, info["axis_a"], info["axis_b"])
    along = np.abs(np.abs(c) - 1) < 1e-6
    assert along.sum() >= 2 and (c[along] > 0).any() and (c[along] < 0).any()
    null = np.abs(d).sum(axis=1) == 0
    assert null.any() and np.all(t[null] == 0)                                       # s == 0: t = 0
    for quadrant in range(4):
        assert ((t > quadrant) & (t < quadrant + 1)).any()
    j0 = np.floor(t * f32(f32(nphi) * f32(0.25))).astype(np.int64)
    assert ((j0 % nphi) == nphi - 1).any()                                          # the wrap cell
    want = N.bake_lookup_reference(table, info, box, pos, d)
    got = tr.bake_lookup(bake, torch.from_numpy(pos).cuda(), torch.from_numpy(d).cuda()).cpu().numpy()
    assert np.array_equal(got, want) and np.ptp(want) > 0
    assert np.abs(want).max() <= np.abs(table).max()                                 # interpolation stays inside the table's range
    empty = tr.bake_lookup(bake, torch.empty((0, 3), device="cuda"), torch.empty((0, 3), device="cuda"))
    assert tuple(empty.shape) == (0,)


def baked_definition(tr, bake, sid, transform="linear", scale=SCALE, expf=None, direct_frame=None):
    """The frame from descriptor_frame's records, bake_lookup_reference and render_values (D: the mode-2 frame at the records)."""
    _, pos, view, pix = tr.descriptor_frame(sid)
    p = pix.cpu().numpy().astype(np.int64)
    o = N.bake_lookup_reference(bake.table(), bake.info, box_of(tr), pos.cpu().numpy(), view.cpu().numpy())
    frame = np.zeros((tr.height * tr.width, 4), np.float32)
    frame[:, 3] = 1
    direct = None if direct_frame is None else direct_frame.reshape(-1, 4)[p, :3]
    frame[p] = N.render_values(o, transform, scale, expf=expf, direct=direct)
    return frame.reshape(tr.height, tr.width, 4), o, p


@pytest.fixture(scope="module")
def single_frame():
    """ct_render_subframe(SID) of a CT_MODE_SUN_SINGLE_SCATTER handle: D, as tests/test_network_direct.py takes it."""
    with ds.CloudTracer(cloud(), width=W, height=H, mode=_lib.CT_MODE_SUN_SINGLE_SCATTER, estimator=_lib.CT_EST_MARCH) as single:
        single.render_subframe(SID)
        return single.frame()


@pytest.mark.gpu
@pytest.mark.parametrize("direct", [False, True], ids=["plain", "direct"])
@pytest.mark.parametrize("transform", ["linear", "expm1"])
def test_frame_equals_its_definition(scene, oracle_lib, single_frame, transform, direct):
    import torch
    tr = scene["tr"]
    expf = lambda v: oracle_lib.orc_expf(v)
    positive = []
    for key in ("bake_net", "bake_neg"):
        bake = scene[key]
        want, out, pix = baked_definition(tr, bake, SID, transform, SCALE, expf, single_frame if direct else None)
        assert 0 < len(pix) < W * H
        got = tr.baked_render_subframe(bake, SID, transform=transform, rgb_scale=SCALE, direct=direct)
        assert got.shape == (H, W, 4) and got.dtype == torch.float32
        assert np.array_equal(got.cpu().numpy(), want)
        assert np.array_equal(tr.download(_lib.CT_BUF_FRAME), want)
        mine = torch.full((H, W, 4), -7.0, dtype=torch.float32, device=got.device)
        assert tr.baked_render_subframe(bake, SID, transform=transform, rgb_scale=SCALE, direct=direct, out=mine) is mine
        assert np.array_equal(mine.cpu().numpy(), want)
        positive.append(out > 0)
        assert positive[-1].any()
        miss = np.ones(W * H, bool)
        miss[pix] = False
        assert np.all(want.reshape(-1, 4)[miss] == np.array([0, 0, 0, 1], np.float32))
        if direct:
            assert single_frame.reshape(-1, 4)[pix, :3].any()
    assert np.all(positive[0] ^ positive[1] | (out == 0))            # the table of the negated network is the negated table


@pytest.mark.gpu
def test_frame_of_the_flagship_network_equals_its_definition(scene, oracle_lib):
    tr = scene["tr"]
    expf = lambda v: oracle_lib.orc_expf(v)
    for negated in (False, True):
        with N.Network(tr, weights(FLAGSHIP, negated), 200, 1, 3) as net, tr.network_bake(net, *GRID_B) as bake:
            for transform in ("linear", "expm1"):
                want = baked_definition(tr, bake, SID, transform, SCALE, expf)[0]
                got = tr.baked_render_subframe(bake, SID, transform=transform, rgb_scale=SCALE).cpu().numpy()
                assert np.array_equal(got, want), (negated, transform)


@pytest.mark.gpu
def test_shard_frames_are_the_unsharded_frame_cut_by_tiles():
    w, h, count = 27, 13, 3
    total = np.zeros((h, w, 4), np.float32)
    with ds.CloudTracer(cloud(), width=w, height=h) as tr, small_net(tr) as net, tr.network_bake(net, *GRID_A) as bake:
        whole = baked_definition(tr, bake, SID)[0]
        assert np.array_equal(tr.baked_render_subframe(bake, SID, rgb_scale=SCALE).cpu().numpy(), whole)
        assert np.array_equal(tr.baked_render_shard_subframe(bake, SID, rgb_scale=SCALE).cpu().numpy(), whole)    # shard_count == 1
        assert whole[..., :3].any()
        tr.baked_render_accumulate(bake, 1, 3, rgb_scale=SCALE)
        whole_mean, whole_m2 = tr.mean(), tr.m2()
    ys, xs = np.mgrid[0:h, 0:w]
    sums = [np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)]
    for index in range(count):
        own = np.vectorize(lambda x, y: ds.tile_owner(int(x) // 8, int(y) // 8, count) == index)(xs, ys)
        with ds.CloudTracer(cloud(), width=w, height=h, shard_index=index, shard_count=count) as tr, small_net(tr) as net, \
                tr.network_bake(net, *GRID_A) as bake:
            for band in (0, 64):
                got = tr.baked_render_shard_subframe(bake, SID, rgb_scale=SCALE, band_pixels=band).cpu().numpy()
                assert np.array_equal(got[own], whole[own]) and not got[~own].any(), (index, band)
            total += got
            tr.baked_render_shard_accumulate(bake, 1, 3, rgb_scale=SCALE, band_pixels=128)
            mean, m2 = tr.mean(), tr.m2()
            assert tr.subframes == 3 and not mean[~own].any() and not m2[~own].any()
            sums[0] += mean
            sums[1] += m2
    assert np.array_equal(total, whole)
    assert np.array_equal(sums[0], whole_mean) and np.array_equal(sums[1], whole_m2) and whole_m2.any()


@pytest.mark.gpu
def test_a_constant_network_renders_the_network_renderers_image():
    """All weights 0 and the output bias 0.37: every table entry and every network output is 0.37, so the two routes agree."""
    w = np.zeros(SMALL.weight_count(), np.float32)
    w[-1] = np.float32(0.37)
    tex = cloud()
    with ds.CloudTracer(tex, width=W, height=H) as a, ds.CloudTracer(tex, width=W, height=H) as b:
        with N.Network(a, w, 32, 1, 1) as na, N.Network(b, w, 32, 1, 1) as nb, a.network_bake(na, (3, 2, 4), 4, 2) as bake:
            assert np.all(bake.table() == np.float32(0.37))
            for direct in (False, True):
                for transform in ("linear", "expm1"):
                    kw = dict(transform=transform, rgb_scale=SCALE, direct=direct)
                    got = a.baked_render_subframe(bake, SID, **kw).cpu().numpy()
                    assert np.array_equal(got, b.network_render_subframe(nb, SID, **kw).cpu().numpy()) and got[..., :3].any()
                a.reset()
                b.reset()
                a.baked_render_accumulate(bake, 1, 5, rgb_scale=SCALE, direct=direct)
                b.network_render_accumulate(nb, 1, 5, rgb_scale=SCALE, direct=direct)
                assert a.subframes == b.subframes == 5
                assert np.array_equal(a.mean(), b.mean()) and np.array_equal(a.m2(), b.m2()) and a.m2().any()


@pytest.mark.gpu
@pytest.mark.parametrize("stop", [False, True])
def test_fused_equals_the_unfused_loop(stop):
    tex = cloud()
    kw = dict(transform="linear", rgb_scale=SCALE, direct=True)
    with ds.CloudTracer(tex, width=W, height=H) as a, ds.CloudTracer(tex, width=W, height=H) as b:
        with small_net(a) as na, small_net(b) as nb, a.network_bake(na, *GRID_A) as ba, b.network_bake(nb, *GRID_A) as bb:
            if stop:
                a.set_stop_when_converged(2, 2)
                b.set_stop_when_converged(2, 2)
            a.baked_render_accumulate(ba, 1, 5, band_pixels=48, **kw)
            for sid in range(1, 6):
                b.baked_render_subframe(bb, sid, out=False, **kw)
                b.accumulate(sid)
            assert np.array_equal(a.mean(), b.mean()) and np.array_equal(a.m2(), b.m2()) and a.subframes == b.subframes == 5
            assert a.mean()[..., :3].any() and a.m2().any()
            assert a.converged_at() == b.converged_at()
            if stop:
                assert a.converged_at()[:2] == (2, 2)
            assert a.baked_render_time() > 0
            want = b.mean()
            # in two calls
            a.reset()
            if stop:
                a.set_stop_when_converged(2, 2)
            a.baked_render_accumulate(ba, 1, 2, **kw)
            assert a.subframes == 2
            a.baked_render_accumulate(ba, 3, 3, band_pixels=24, **kw)
            assert np.array_equal(a.mean(), want) and a.subframes == 5 and a.converged_at() == b.converged_at()


@pytest.mark.gpu
def test_the_image_does_not_depend_on_the_bands(scene):
    tr, bake = scene["tr"], scene["bake_net"]
    want = baked_definition(tr, bake, SID)[0]
    for band in (1, 25, 120, 0):
        got = tr.baked_render_subframe(bake, SID, rgb_scale=SCALE, band_pixels=band)
        assert np.array_equal(got.cpu().numpy(), want), band


@pytest.mark.gpu
def test_a_baked_call_leaves_the_network_renderers_times(scene):
    """The two routes share one driver but not their clocks: the four stage times are the last network call's, and a baked call
    sets its own time only."""
    tr, net, bake = scene["tr"], scene["net"], scene["bake_net"]
    tr.network_render_subframe(net, SID, rgb_scale=SCALE)
    want = tr.network_render_time()
    assert len(want) == 4 and all(ms > 0 for ms in want)
    tr.baked_render_subframe(bake, SID, rgb_scale=SCALE)
    assert tr.network_render_time() == want
    assert tr.baked_render_time() > 0


@pytest.mark.gpu
def test_render_subframe_touches_nothing_but_the_frame():
    tex = cloud()
    states = []
    for with_call in (True, False):
        with ds.CloudTracer(tex, width=W, height=H) as tr, small_net(tr) as net, tr.network_bake(net, *GRID_A) as bake:
            tr.render_accumulate(1, 2)
            if with_call:
                frame = tr.baked_render_subframe(bake, SID, rgb_scale=SCALE, band_pixels=48)
                assert bool((frame[..., :3] != 0).any()) and tr.subframes == 2
                before = tr.network_scratch()
                tr.baked_render_subframe(bake, SID, rgb_scale=SCALE, band_pixels=48)          # a warm call allocates nothing
                tr.baked_render_subframe(bake, 1, rgb_scale=SCALE, band_pixels=24)
                assert tr.network_scratch() == before and before["found"] != 0
            tr.render_accumulate(3, 2)
            states.append((tr.mean(), tr.m2(), tr.subframes, tr.counters(), tr.fetch_counters()))
    x, y = states
    assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and x[0].any() and x[2:] == y[2:] and x[2] == 4


def _code(fn, *a, **kw):
    with pytest.raises(_lib.CloudTraceError) as e:
        fn(*a, **kw)
    return e.value.code


@pytest.mark.gpu
def test_a_new_light_makes_the_bake_stale_until_it_is_updated():
    import torch
    with ds.CloudTracer(cloud(), width=W, height=H) as tr, small_net(tr) as net, tr.network_bake(net, *GRID_A) as bake:
        old = bake.table()
        tr.set_light(LIGHT2)
        assert not bake.info["current"]
        assert _code(tr.baked_render_subframe, bake, SID) == _lib.CT_E_STATE
        assert b"ct_bake_update" in tr.L.ct_last_error(tr.h)
        assert _code(tr.baked_render_accumulate, bake, 1, 1) == _lib.CT_E_STATE
        z = torch.zeros((1, 3), device="cuda")
        assert _code(tr.bake_lookup, bake, z, z) == _lib.CT_E_STATE
        assert tr.subframes == 0 and np.array_equal(bake.table(), old)       # the old table is still there
        bake.update(net)
        info = bake.info
        assert info["current"] and np.array_equal(info["light"], tr.light_direction())
        with ds.CloudTracer(cloud(), width=W, height=H, light_direction=LIGHT2) as fresh, small_net(fresh) as n2, \
                fresh.network_bake(n2, *GRID_A) as b2:
            assert np.array_equal(bake.table(), b2.table()) and not np.array_equal(b2.table(), old)
            for k in ("light", "axis_a", "axis_b"):
                assert np.array_equal(info[k], b2.info[k])
            want = fresh.baked_render_subframe(b2, SID, rgb_scale=SCALE).cpu().numpy()
        assert np.array_equal(tr.baked_render_subframe(bake, SID, rgb_scale=SCALE).cpu().numpy(), want)
        lit = bake.table()
        with small_net(tr, negated=True) as neg:                              # ... and for another network
            bake.update(neg)
            assert np.array_equal(bake.table(), -lit) and lit.any()


@pytest.mark.gpu
def test_errors_leave_the_handle_usable(scene):
    import torch
    tr, net, bake = scene["tr"], scene["net"], scene["bake_net"]
    L, h = tr.L, tr.h
    want = baked_definition(tr, bake, SID)[0]

    def still_renders():
        assert np.array_equal(tr.baked_render_subframe(bake, SID, rgb_scale=SCALE).cpu().numpy(), want)

    def desc(grid=(2, 2, 2), nphi=4, nc=2, abi=_lib.CT_ABI_VERSION):
        return _lib.CtBakeDesc(abi, (C.c_uint32 * 3)(*grid), nphi, nc)

    out = C.c_void_p()
    bad_sizes = [dict(grid=(1, 2, 2)), dict(grid=(2, 257, 2)), dict(grid=(2, 2, 0)), dict(nphi=0), dict(nphi=6), dict(nphi=68), dict(nc=1),
                 dict(nc=65), dict(grid=(256, 256, 256), nphi=4, nc=2), dict(abi=_lib.CT_ABI_VERSION + 1)]
    for kw in bad_sizes:
        d = desc(**kw)
        assert L.ct_network_bake(h, net.n, C.byref(d), C.byref(out)) == _lib.CT_E_INVAL and not out.value, kw
    d = desc()
    assert L.ct_network_bake(h, None, C.byref(d), C.byref(out)) == _lib.CT_E_INVAL
    assert L.ct_network_bake(h, net.n, None, C.byref(out)) == _lib.CT_E_INVAL
    assert L.ct_network_bake(h, net.n, C.byref(d), None) == _lib.CT_E_INVAL
    assert L.ct_bake_update(h, None, bake.b) == _lib.CT_E_INVAL and L.ct_bake_update(h, net.n, None) == _lib.CT_E_INVAL
    for shape in (N.NetworkShape(32, 0, 1), N.NetworkShape(16, 2, 1)):                       # aux 0, aux 2
        from test_network_render import seeded_weights
        with N.Network(tr, seeded_weights(shape, 2), shape.width, shape.aux, shape.head_layers) as other:
            assert _code(tr.network_bake, other, (2, 2, 2), 4, 2) == _lib.CT_E_INVAL
            assert _code(bake.update, other) == _lib.CT_E_INVAL
    still_renders()
    # ranges of probes and table
    info = bake.info
    probes = info["entries"] // info["cosines"]
    assert _code(bake.probes, probes, 1) == _lib.CT_E_INVAL and _code(bake.probes, 0, probes + 1) == _lib.CT_E_INVAL
    buf = np.empty(info["entries"] + 1, np.float32)
    for count in (info["entries"] - 1, info["entries"] + 1, 0):
        assert L.ct_bake_download(bake.b, buf.ctypes.data_as(C.c_void_p), count) == _lib.CT_E_INVAL
    assert L.ct_bake_download(bake.b, None, info["entries"]) == _lib.CT_E_INVAL
    assert L.ct_bake_info(bake.b, None) == _lib.CT_E_INVAL
    # the render calls
    for bad in (dict(transform=2), dict(transform=-1), dict(transform="log"), dict(rgb_scale=(1, np.nan, 1)), dict(rgb_scale=(np.inf, 1, 1))):
        for sub, acc in ((tr.baked_render_subframe, tr.baked_render_accumulate), (tr.baked_render_shard_subframe, tr.baked_render_shard_accumulate)):
            assert _code(sub, bake, SID, **bad) == _lib.CT_E_INVAL, bad
            assert _code(acc, bake, 1, 1, **bad) == _lib.CT_E_INVAL, bad
    p = _lib.CtNetworkRender(_lib.CT_ABI_VERSION + 1, 0, (C.c_float * 3)(1, 1, 1), 0)
    assert L.ct_baked_render_subframe(h, bake.b, C.byref(p), SID, None) == _lib.CT_E_INVAL and b"abi_version" in L.ct_last_error(h)
    p = _lib.CtNetworkRender(_lib.CT_ABI_VERSION, 0, (C.c_float * 3)(1, 1, 1), 0)
    assert L.ct_baked_render_subframe(h, None, C.byref(p), SID, None) == _lib.CT_E_INVAL
    assert L.ct_baked_render_subframe(h, bake.b, None, SID, None) == _lib.CT_E_INVAL
    assert L.ct_baked_render_accumulate(h, None, C.byref(p), 1, 1) == _lib.CT_E_INVAL
    assert L.ct_baked_render_accumulate(h, bake.b, None, 1, 1) == _lib.CT_E_INVAL
    assert _code(tr.baked_render_subframe, bake, 0) == _lib.CT_E_INVAL
    assert _code(tr.baked_render_accumulate, bake, 0, 1) == _lib.CT_E_INVAL
    assert _code(tr.baked_render_accumulate, bake, 1, 0) == _lib.CT_E_INVAL
    assert _code(tr.baked_render_accumulate, bake, 2, 1) == _lib.CT_E_STATE                  # first != subframes + 1
    assert b"subframes are accumulated" in L.ct_last_error(h)
    assert L.ct_debug_baked_render_time(h, None) == _lib.CT_E_INVAL
    z = torch.zeros((2, 3), device="cuda")
    assert L.ct_debug_bake_lookup(h, bake.b, None, C.c_void_p(z.data_ptr()), 2, C.c_void_p(z.data_ptr())) == _lib.CT_E_INVAL
    assert L.ct_debug_bake_lookup(h, None, C.c_void_p(z.data_ptr()), C.c_void_p(z.data_ptr()), 2, C.c_void_p(z.data_ptr())) == _lib.CT_E_INVAL
    assert tr.subframes == 0 and not tr.mean().any()
    still_renders()
    # a bake made on another handle; a sharded handle on the unsharded entry points
    with ds.CloudTracer(cloud(), width=W, height=H, shard_index=0, shard_count=2) as shard, small_net(shard) as sn, \
            shard.network_bake(sn, (2, 2, 2), 4, 2) as sb:
        assert _code(tr.baked_render_subframe, sb, SID) == _lib.CT_E_INVAL and b"another handle" in L.ct_last_error(h)
        assert _code(tr.baked_render_accumulate, sb, 1, 1) == _lib.CT_E_INVAL
        assert _code(tr.bake_lookup, sb, z, z) == _lib.CT_E_INVAL
        assert L.ct_bake_update(h, net.n, sb.b) == _lib.CT_E_INVAL
        assert _code(shard.baked_render_subframe, sb, SID) == _lib.CT_E_INVAL and b"shard" in shard.L.ct_last_error(shard.h)
        assert _code(shard.baked_render_accumulate, sb, 1, 1) == _lib.CT_E_INVAL
        shard.baked_render_shard_accumulate(sb, 1, 1)
        assert shard.subframes == 1 and shard.mean().any()
    still_renders()


@pytest.mark.gpu
def test_cli_renders_from_the_baked_table(tmp_path):
    """cloudtrace --network F --net-baked 5,4,3,8,3: the written images are Python's mean after baked_render_accumulate(1, 4) under
    the same light and pose, for both of the job's suns (the second after a re-bake)."""
    from deepestscatter_amd import build
    cli = build.build_cli()
    N.save_weights(tmp_path / "w.bin", weights(SMALL), SMALL)
    r = subprocess.run([str(cli), "procedural:64", "--network", str(tmp_path / "w.bin"), "--net-baked", "5,4,3,8,3", "--size", f"{W}x{H}",
                        "--spp", "4", "--format", "pfm", "--net-scale", "0.5,2,3", "--out", str(tmp_path)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    with ds.CloudTracer(cloud(), width=W, height=H, light_direction=ds.LIGHT_DIRECTIONS["Side"]) as tr, small_net(tr) as net:
        images = {}
        with tr.network_bake(net, *GRID_A) as bake:
            for light in ("Side", "Back"):
                tr.set_light(ds.LIGHT_DIRECTIONS[light])
                bake.update(net)
                tr.reset()
                tr.baked_render_accumulate(bake, 1, 4, rgb_scale=SCALE)
                images[light] = tr.mean()[..., :3]
    assert not np.array_equal(images["Side"], images["Back"])
    for light, want in images.items():
        raw = (tmp_path / f"procedural_64.{light}.PT.pfm").read_bytes()
        header_end = 0
        for _ in range(3):
            header_end = raw.index(b"\n", header_end) + 1
        img = np.frombuffer(raw[header_end:], "<f4").reshape(H, W, 3)
        assert want.any() and np.array_equal(img, want), light
    # with --gpus the baked renderer is refused with a message
    r = subprocess.run([str(cli), "procedural:16", "--network", str(tmp_path / "w.bin"), "--net-baked", "5,4,3,8,3", "--gpus", "2", "--out",
                        str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--net-baked" in r.stdout + r.stderr
