"""ct_network_bake_sparse: the probe table baked only where a first flight can look it up (include/cloudtrace.h, "the sparse
bake").

The mask is an integer definition -- per-axis texel ranges of the grid's cells, "any non-zero texel in the box", corners of
occupied cells -- restated in numpy (network.bake_mask_reference); the device's cells, nodes and list are held to it BYTE FOR
BYTE.  The sparse table is held to the dense table bit for bit on the mask and to 0.0f off it, and every frame to the dense
bake's frame bit for bit.  The safety property -- every lookup a flight can make touches active nodes only -- is checked on the
records of descriptor_frame with the lookup's own float32 cell arithmetic.

Scene and weights: those of tests/test_network_render.py, as tests/test_network_baked.py takes them.

An all-zero volume: ct_create accepts one (its bounding box of non-zero texels is empty), so the zero-active path runs here."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import deepestscatter_amd as ds
from deepestscatter_amd import _lib
from deepestscatter_amd import network as N
from test_network_render import H, LIGHT2, SCALE, SID, SMALL, W, cloud, weights

GRID = ((9, 8, 7), 8, 3)        # 504 nodes, 314 of them active on cloud(): 2512 probes
COARSE_STEP = 1.0 / 32.0        # S = 2 texels on the 64^3 cloud: M = 5
CLOSE_POSE = ((0.45, 0.3, -0.95), (0.0, 0.0, 0.0), 40.0)


def brute_force_mask(shape, texels, grid, M):
    """The definition with Python integers, for a volume whose non-zero texels are `texels` = [(z, y, x)]."""
    dz, dy, dx = shape
    nx, ny, nz = grid

    def ranges(n, d):
        return [(max(0, (c * d) // (n - 1) - M), min(d - 1, -((-(c + 1) * d) // (n - 1)) + M)) for c in range(n - 1)]

    rx, ry, rz = ranges(nx, dx), ranges(ny, dy), ranges(nz, dz)
    cells = np.zeros((nz - 1, ny - 1, nx - 1), np.uint8)
    nodes = np.zeros((nz, ny, nx), np.uint8)
    for cz, (zl, zh) in enumerate(rz):
        for cy, (yl, yh) in enumerate(ry):
            for cx, (xl, xh) in enumerate(rx):
                if any(zl <= z <= zh and yl <= y <= yh and xl <= x <= xh for z, y, x in texels):
                    cells[cz, cy, cx] = 1
                    nodes[cz:cz + 2, cy:cy + 2, cx:cx + 2] = 1
    return cells, nodes


# ---------------------------------------------------------------------------------------------------- CPU
def test_symbols_resolve_and_answer_null_arguments(product_lib):
    L = product_lib
    for name in ("ct_network_bake_sparse", "ct_bake_sparse_info", "ct_bake_mask", "ct_debug_bake_mask"):
        assert hasattr(L, name) and name in _lib.EXPORTS
    d = _lib.CtBakeDesc(_lib.CT_ABI_VERSION, (C.c_uint32 * 3)(2, 2, 2), 4, 2)
    out = C.c_void_p()
    assert L.ct_network_bake_sparse(None, None, C.byref(d), C.byref(out)) == _lib.CT_E_INVAL
    assert L.ct_network_bake_sparse(None, None, None, None) == _lib.CT_E_INVAL
    assert L.ct_bake_sparse_info(None, None) == _lib.CT_E_INVAL
    assert L.ct_bake_mask(None, None, 0) == _lib.CT_E_INVAL
    grid, n = (C.c_uint32 * 3)(2, 2, 2), C.c_uint32(7)
    assert L.ct_debug_bake_mask(None, grid, None, None, None, 0, C.byref(n)) == _lib.CT_E_INVAL
    assert L.ct_debug_bake_mask(None, None, None, None, None, 0, None) == _lib.CT_E_INVAL
    assert C.sizeof(_lib.CtBakeSparseInfo) == 40
    assert _lib.CtBakeSparseInfo.nodes.offset == 8 and _lib.CtBakeSparseInfo.mask_ms.offset == 32


def test_reference_mask_of_the_procedural_cloud():
    tex = cloud()
    for grid, active in (((5, 4, 3), 60), ((9, 8, 7), 314), ((17, 17, 17), 1889)):
        cells, nodes, M = N.bake_mask_reference(tex, grid, ds.SceneParams().sample_step)
        nx, ny, nz = grid
        assert M == 4 and cells.shape == (nz - 1, ny - 1, nx - 1) and nodes.shape == (nz, ny, nx)
        assert cells.dtype == nodes.dtype == np.uint8 and int(nodes.sum()) == active, grid
    assert N.bake_mask_reference(tex, (9, 8, 7), COARSE_STEP)[2] == 5


def test_reference_mask_of_one_texel_is_the_cells_whose_ranges_hold_it():
    shape, grid = (61, 40, 56), (9, 8, 7)
    for texel in ((40, 20, 10), (0, 39, 55), (60, 0, 0)):
        tex = np.zeros(shape, np.uint8)
        tex[texel] = 3
        cells, nodes, M = N.bake_mask_reference(tex, grid, ds.SceneParams().sample_step)
        want_cells, want_nodes = brute_force_mask(shape, [texel], grid, 4)
        assert M == 4 and np.array_equal(cells, want_cells) and np.array_equal(nodes, want_nodes)
        assert 0 < nodes.sum() < nodes.size and 0 < cells.sum() < cells.size
    assert not N.bake_mask_reference(np.zeros(shape, np.uint8), grid, 1 / 512)[1].any()


# ---------------------------------------------------------------------------------------------------- GPU
def small_net(tr, negated=False):
    return N.Network(tr, weights(SMALL, negated), 32, 1, 1)


def crop():
    """56 x 40 x 61 texels (z, y, x): non-cubic, rows of 61 bytes -- no multiple of 4 -- and the cloud's zero border kept (its non-zero
    texels are z 11 .. 51, y 16 .. 47, x 8 .. 54)."""
    return np.ascontiguousarray(cloud()[4:60, 12:52, 1:62])


def check_mask(tr, tex, grid, step=None):
    step = ds.SceneParams().sample_step if step is None else step
    want_cells, want_nodes, _ = N.bake_mask_reference(tex, grid, step)
    cells, nodes, active = tr.bake_mask(grid)
    assert np.array_equal(cells, want_cells), grid
    assert np.array_equal(nodes, want_nodes), grid
    assert active.dtype == np.uint32 and np.array_equal(active, np.flatnonzero(want_nodes.reshape(-1))), grid
    assert np.all(np.diff(active.astype(np.int64)) > 0)
    return int(want_nodes.sum())


@pytest.fixture(scope="module")
def scene():
    """The module's tracer on cloud() as it is created, its small network, and the dense and the sparse bake of GRID.  No test
    changes its light or accumulates on it."""
    with ds.CloudTracer(cloud(), width=W, height=H) as tr:
        made = []
        try:
            s = {"tr": tr, "net": small_net(tr)}
            made.append(s["net"])
            for key, sparse in (("dense", False), ("sparse", True)):
                s[key] = tr.network_bake(s["net"], *GRID, sparse=sparse)
                made.append(s[key])
            yield s
        finally:
            for obj in reversed(made):
                obj.close()


@pytest.mark.gpu
@pytest.mark.parametrize("grid", [(2, 2, 2), (9, 8, 7), (17, 17, 17), (256, 2, 3), (48, 48, 48)], ids=str)
def test_mask_of_the_cloud_equals_its_numpy_definition(scene, grid):
    """(256, 2, 3): cells narrower than a texel.  (48, 48, 48): 110 592 nodes are 1728 waves, more than one per thread of the scan."""
    active = check_mask(scene["tr"], cloud(), grid)
    assert 0 < active and (active < np.prod(grid) or grid == (2, 2, 2))


@pytest.mark.gpu
def test_mask_of_a_crop_with_ragged_rows():
    tex = crop()
    assert tex.shape == (56, 40, 61) and tex.any() and not tex[[0, -1]].any() and not tex[:, [0, -1]].any() and not tex[:, :, [0, -1]].any()
    with ds.CloudTracer(tex, width=W, height=H) as tr:
        assert tr.dims == (61, 40, 56)
        for grid in ((9, 8, 7), (7, 5, 11)):
            assert 0 < check_mask(tr, tex, grid) < np.prod(grid)


@pytest.mark.gpu
def test_mask_with_a_coarse_march_step():
    with ds.CloudTracer(cloud(), width=W, height=H, sample_step=COARSE_STEP) as tr:
        fine = N.bake_mask_reference(cloud(), (17, 17, 17), ds.SceneParams().sample_step)[1]
        active = check_mask(tr, cloud(), (17, 17, 17), COARSE_STEP)
        assert active > fine.sum()                                    # M = 5 reaches further than M = 4


@pytest.mark.gpu
def test_mask_in_slabs_of_z(monkeypatch):
    """CT_BAKE_MASK_BYTES caps the first temporary: 64 planes of 64 x 8 bytes go through in slabs of 5 (the last one of 4) and of 1,
    the crop's 56 planes of 40 x 6 bytes in slabs of 4."""
    for tex, cap, grid in ((cloud(), "3000", (9, 8, 7)), (cloud(), "1", (9, 8, 7)), (crop(), "1000", (7, 5, 11))):
        monkeypatch.setenv("CT_BAKE_MASK_BYTES", cap)
        with ds.CloudTracer(tex, width=W, height=H) as tr:
            check_mask(tr, tex, grid)


@pytest.mark.gpu
def test_mask_of_single_texel_volumes_and_of_an_empty_one():
    shape, grid = (20, 33, 45), (6, 5, 4)
    for texel in ((7, 30, 44), (19, 0, 0), (0, 32, 17)):               # the last byte of a row, the first, the first plane
        tex = np.zeros(shape, np.uint8)
        tex[texel] = 200
        with ds.CloudTracer(tex, width=W, height=H) as tr:
            cells, nodes, active = tr.bake_mask(grid)
            want_cells, want_nodes = brute_force_mask(shape, [texel], grid, 4)
            assert np.array_equal(cells, want_cells) and np.array_equal(nodes, want_nodes)
            assert np.array_equal(active, np.flatnonzero(want_nodes.reshape(-1))) and 0 < len(active) < nodes.size
    empty = np.zeros(shape, np.uint8)
    with ds.CloudTracer(empty, width=W, height=H) as tr, small_net(tr) as net:
        cells, nodes, active = tr.bake_mask(grid)
        assert not cells.any() and not nodes.any() and len(active) == 0
        with tr.network_bake(net, grid, 4, 2, sparse=True) as bake:    # no active node: an all-zero table, nothing evaluated
            info, sp = bake.info, bake.sparse_info
            assert sp["sparse"] and sp["active_nodes"] == 0 and sp["probes_baked"] == 0 and sp["nodes"] == 120
            assert info["gather_ms"] == 0 and info["network_ms"] == 0 and info["current"]
            assert not bake.table().any() and not bake.mask().any()
            frame = tr.baked_render_subframe(bake, SID).cpu().numpy()
            assert np.all(frame == np.array([0, 0, 0, 1], np.float32))


def assert_sparse_of(sparse_table, dense_table, mask):
    on = mask.astype(bool)
    assert np.array_equal(sparse_table[on], dense_table[on])
    off = sparse_table[~on]
    assert np.all(off == 0) and not np.signbit(off).any()            # exactly 0.0f
    assert dense_table[~on].any() and dense_table[on].any()           # the dense bake has numbers there: the zeros are the sparse bake's


def check_sparse_bake(sparse, dense, want_mask):
    """The sparse bake of GRID against the dense one of the same tracer: info, mask, table and probes."""
    (nx, ny, nz), nphi, nc = GRID
    sp, di = sparse.sparse_info, sparse.info
    assert sp == {**sp, "sparse": True, "margin_texels": 4, "nodes": 504, "active_nodes": 314, "probes_baked": 2512} and sp["mask_ms"] > 0
    assert di["grid"] == (nx, ny, nz) and di["entries"] == 504 * nphi * nc and di["current"] and di["gather_ms"] > 0 and di["network_ms"] > 0
    assert np.array_equal(sparse.mask(), want_mask)
    assert_sparse_of(sparse.table(), dense.table(), want_mask)
    for a, b in zip(sparse.probes(), dense.probes()):
        assert np.array_equal(a, b)


@pytest.mark.gpu
def test_sparse_table_is_the_dense_table_on_the_mask(scene, monkeypatch):
    dense, sparse = scene["dense"], scene["sparse"]
    (nx, ny, nz), nphi, nc = GRID
    want_mask = N.bake_mask_reference(cloud(), GRID[0], ds.SceneParams().sample_step)[1]
    check_sparse_bake(sparse, dense, want_mask)
    table = dense.table()
    # a dense bake answers the same questions
    dd = dense.sparse_info
    assert dd == {**dd, "sparse": False, "margin_texels": 0, "nodes": 504, "active_nodes": 504, "probes_baked": 504 * nphi}
    assert dense.mask().all() and dense.mask().shape == (nz, ny, nx)
    # in pieces of 48 records (2512 = 52 x 48 + 16: a partial last piece), and with fixed-point texture weights
    monkeypatch.setenv("CT_NET_DESC_RECORDS", "48")
    with ds.CloudTracer(cloud(), width=W, height=H) as t2, small_net(t2) as net, t2.network_bake(net, *GRID) as d2, \
            t2.network_bake(net, *GRID, sparse=True) as s2:
        assert t2.network_scratch()["desc_cap"] == 48
        check_sparse_bake(s2, d2, want_mask)
        assert np.array_equal(s2.table(), sparse.table())             # the pieces change nothing
    monkeypatch.delenv("CT_NET_DESC_RECORDS")
    with ds.CloudTracer(cloud(), width=W, height=H, flags=_lib.CT_FLAG_TEX_FIXED8) as t3, small_net(t3) as net, \
            t3.network_bake(net, *GRID) as d3, t3.network_bake(net, *GRID, sparse=True) as s3:
        assert not np.array_equal(d3.table(), table)
        check_sparse_bake(s3, d3, want_mask)


def lookup_corners_are_active(tr, nodes, positions):
    """The lookup's x0, y0, z0 in float32, as network.bake_lookup_reference makes them -> every one of the eight corners is active."""
    f32 = np.float32
    nz, ny, nx = nodes.shape
    box = (np.array(tr.dims, f32) / f32(max(tr.dims))).astype(f32)
    w = np.ascontiguousarray(positions, f32).reshape(-1, 3)
    base = []
    for axis, n in enumerate((nx, ny, nz)):
        scale = f32(f32(n - 1) / box[axis])
        f = ((w[:, axis] + f32(0.5) * box[axis]).astype(f32) * scale).astype(f32)
        f = np.minimum(np.maximum(f, f32(0)), f32(n - 1)).astype(f32)
        base.append(np.minimum(f.astype(np.int64), n - 2))
    x0, y0, z0 = base
    ok = np.ones(len(w), bool)
    for q in range(8):
        ok &= nodes[z0 + (q >> 2), y0 + ((q >> 1) & 1), x0 + (q & 1)] != 0
    return ok


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["default pose", "close pose", "coarse step"])
def test_every_lookup_of_a_flight_touches_active_nodes_only(case):
    step = COARSE_STEP if case == "coarse step" else ds.SceneParams().sample_step
    with ds.CloudTracer(cloud(), width=W, height=H, sample_step=step) as tr:
        if case == "close pose":
            eye, lookat, fov = CLOSE_POSE
            tr.set_camera(eye, *ds.calculate_camera_variables(eye, lookat, (0, 1, 0), fov, W / H))
        positions = np.concatenate([tr.descriptor_frame(sid)[1].cpu().numpy() for sid in range(1, 9)])
        print(f"{case}: {len(positions)} records")
        assert len(positions) >= 50
        for grid in ((9, 8, 7), (17, 17, 17), (33, 33, 33)):
            nodes = tr.bake_mask(grid)[1]
            assert np.array_equal(nodes, N.bake_mask_reference(cloud(), grid, step)[1])
            ok = lookup_corners_are_active(tr, nodes, positions)
            assert ok.all(), (case, grid, int((~ok).sum()))
            assert not nodes.all()                                    # the property is not trivial: there are inactive nodes


@pytest.mark.gpu
@pytest.mark.parametrize("pose", ["default", "close"])
def test_frames_are_the_dense_bakes_frames(pose):
    with ds.CloudTracer(cloud(), width=W, height=H) as tr, small_net(tr) as net, tr.network_bake(net, *GRID) as dense, \
            tr.network_bake(net, *GRID, sparse=True) as sparse:
        if pose == "close":
            eye, lookat, fov = CLOSE_POSE
            tr.set_camera(eye, *ds.calculate_camera_variables(eye, lookat, (0, 1, 0), fov, W / H))
        for transform in ("linear", "expm1"):
            for direct in (False, True):
                kw = dict(transform=transform, rgb_scale=SCALE, direct=direct)
                want = tr.baked_render_subframe(dense, SID, **kw).cpu().numpy()
                got = tr.baked_render_subframe(sparse, SID, **kw).cpu().numpy()
                assert np.array_equal(got, want) and want[..., :3].any(), (transform, direct)
        tr.baked_render_accumulate(dense, 1, 8, rgb_scale=SCALE, direct=True)
        mean, m2 = tr.mean(), tr.m2()
        tr.reset()
        tr.baked_render_accumulate(sparse, 1, 8, rgb_scale=SCALE, direct=True)
        assert tr.subframes == 8 and np.array_equal(tr.mean(), mean) and np.array_equal(tr.m2(), m2) and m2.any()


@pytest.mark.gpu
def test_a_shards_frame_is_the_dense_bakes():
    with ds.CloudTracer(cloud(), width=27, height=13, shard_index=1, shard_count=3) as tr, small_net(tr) as net, \
            tr.network_bake(net, *GRID) as dense, tr.network_bake(net, *GRID, sparse=True) as sparse:
        want = tr.baked_render_shard_subframe(dense, SID, rgb_scale=SCALE).cpu().numpy()
        got = tr.baked_render_shard_subframe(sparse, SID, rgb_scale=SCALE).cpu().numpy()
        assert np.array_equal(got, want) and want[..., :3].any()


def _code(fn, *a, **kw):
    with pytest.raises(_lib.CloudTraceError) as e:
        fn(*a, **kw)
    return e.value.code


@pytest.mark.gpu
def test_update_of_a_sparse_bake_stays_sparse():
    want_mask = N.bake_mask_reference(cloud(), GRID[0], ds.SceneParams().sample_step)[1]
    with ds.CloudTracer(cloud(), width=W, height=H) as tr, small_net(tr) as net, tr.network_bake(net, *GRID, sparse=True) as bake:
        old = bake.table()
        tr.set_light(LIGHT2)
        assert not bake.info["current"]
        assert _code(tr.baked_render_subframe, bake, SID) == _lib.CT_E_STATE
        with ds.CloudTracer(cloud(), width=W, height=H) as other, small_net(other) as foreign:   # a failing update changes nothing:
            assert tr.L.ct_bake_update(other.h, foreign.n, bake.b) == _lib.CT_E_INVAL            # another handle and its network
        shape = N.NetworkShape(16, 2, 1)
        from test_network_render import seeded_weights
        with N.Network(tr, seeded_weights(shape, 2), shape.width, shape.aux, shape.head_layers) as two_aux:
            assert _code(bake.update, two_aux) == _lib.CT_E_INVAL
        assert np.array_equal(bake.table(), old) and not bake.info["current"] and bake.sparse_info["active_nodes"] == 314
        bake.update(net)
        info, sp = bake.info, bake.sparse_info
        assert info["current"] and np.array_equal(info["light"], tr.light_direction())
        assert sp["sparse"] and sp["active_nodes"] == 314 and sp["probes_baked"] == 2512 and sp["mask_ms"] > 0
        assert np.array_equal(bake.mask(), want_mask)
        with ds.CloudTracer(cloud(), width=W, height=H, light_direction=LIGHT2) as fresh, small_net(fresh) as n2, \
                fresh.network_bake(n2, *GRID) as dense:
            table = dense.table()
            assert_sparse_of(bake.table(), table, want_mask)
            assert not np.array_equal(bake.table(), old)
            want = fresh.baked_render_subframe(dense, SID, rgb_scale=SCALE).cpu().numpy()
        assert np.array_equal(tr.baked_render_subframe(bake, SID, rgb_scale=SCALE).cpu().numpy(), want)


@pytest.mark.gpu
def test_errors_leave_the_handle_usable(scene):
    tr, net, dense, sparse = scene["tr"], scene["net"], scene["dense"], scene["sparse"]
    L, h = tr.L, tr.h
    want = tr.baked_render_subframe(dense, SID, rgb_scale=SCALE).cpu().numpy()

    def still_renders():
        assert np.array_equal(tr.baked_render_subframe(sparse, SID, rgb_scale=SCALE).cpu().numpy(), want)

    def desc(grid=(2, 2, 2), nphi=4, nc=2, abi=_lib.CT_ABI_VERSION):
        return _lib.CtBakeDesc(abi, (C.c_uint32 * 3)(*grid), nphi, nc)

    out = C.c_void_p()
    bad_sizes = [dict(grid=(1, 2, 2)), dict(grid=(2, 257, 2)), dict(grid=(2, 2, 0)), dict(nphi=0), dict(nphi=6), dict(nphi=68), dict(nc=1),
                 dict(nc=65), dict(grid=(256, 256, 256), nphi=4, nc=2), dict(abi=_lib.CT_ABI_VERSION + 1)]
    for kw in bad_sizes:
        d = desc(**kw)
        assert L.ct_network_bake_sparse(h, net.n, C.byref(d), C.byref(out)) == _lib.CT_E_INVAL and not out.value, kw
    d = desc()
    assert L.ct_network_bake_sparse(h, None, C.byref(d), C.byref(out)) == _lib.CT_E_INVAL
    assert L.ct_network_bake_sparse(h, net.n, None, C.byref(out)) == _lib.CT_E_INVAL
    assert L.ct_network_bake_sparse(h, net.n, C.byref(d), None) == _lib.CT_E_INVAL
    from test_network_render import seeded_weights
    shape = N.NetworkShape(32, 0, 1)
    with N.Network(tr, seeded_weights(shape, 2), shape.width, shape.aux, shape.head_layers) as no_aux:
        assert _code(tr.network_bake, no_aux, (2, 2, 2), 4, 2, sparse=True) == _lib.CT_E_INVAL
    still_renders()
    # ct_bake_mask and ct_bake_sparse_info
    buf = np.empty(505, np.uint8)
    for count in (503, 505, 0):
        assert L.ct_bake_mask(sparse.b, buf.ctypes.data_as(C.c_void_p), count) == _lib.CT_E_INVAL
        assert L.ct_bake_mask(dense.b, buf.ctypes.data_as(C.c_void_p), count) == _lib.CT_E_INVAL
    assert L.ct_bake_mask(sparse.b, None, 504) == _lib.CT_E_INVAL
    assert L.ct_bake_sparse_info(sparse.b, None) == _lib.CT_E_INVAL
    # ct_debug_bake_mask
    n = C.c_uint32(7)
    for grid in ((1, 2, 2), (2, 257, 2), (2, 2, 0)):
        assert _code(tr.bake_mask, grid) == _lib.CT_E_INVAL
        assert L.ct_debug_bake_mask(h, (C.c_uint32 * 3)(*grid), None, None, None, 0, C.byref(n)) == _lib.CT_E_INVAL and n.value == 0
    grid = (C.c_uint32 * 3)(*GRID[0])
    assert L.ct_debug_bake_mask(h, None, None, None, None, 0, C.byref(n)) == _lib.CT_E_INVAL
    assert L.ct_debug_bake_mask(h, grid, None, None, None, 0, None) == _lib.CT_E_INVAL
    active = np.full(400, 0xFFFFFFFF, np.uint32)
    n.value = 7
    assert L.ct_debug_bake_mask(h, grid, None, None, active.ctypes.data_as(C.c_void_p), 313, C.byref(n)) == _lib.CT_E_INVAL
    assert n.value == 314 and np.all(active == 0xFFFFFFFF)            # the count is answered, nothing is written
    assert L.ct_debug_bake_mask(h, grid, None, None, active.ctypes.data_as(C.c_void_p), 314, C.byref(n)) == _lib.CT_OK
    assert n.value == 314 and np.all(active[314:] == 0xFFFFFFFF) and np.array_equal(active[:314], np.flatnonzero(sparse.mask().reshape(-1)))
    n.value = 7
    assert L.ct_debug_bake_mask(h, grid, None, None, None, 0, C.byref(n)) == _lib.CT_OK and n.value == 314      # the count alone
    still_renders()


@pytest.mark.gpu
def test_cli_writes_the_same_image_with_a_sparse_bake(tmp_path):
    from deepestscatter_amd import build
    cli = build.build_cli()
    N.save_weights(tmp_path / "w.bin", weights(SMALL), SMALL)
    common = [str(cli), "procedural:64", "--network", str(tmp_path / "w.bin"), "--size", f"{W}x{H}", "--spp", "4", "--net-scale", "0.5,2,3"]
    images = {}
    for name, extra in (("dense", []), ("sparse", ["--net-bake-sparse"])):
        (tmp_path / name).mkdir()
        r = subprocess.run(common + ["--net-baked", "9,8,7,8,3"] + extra + ["--out", str(tmp_path / name)], capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        images[name] = {p.name: p.read_bytes() for p in sorted((tmp_path / name).glob("*.exr"))}
    assert len(images["dense"]) >= 2 and images["dense"].keys() == images["sparse"].keys()
    for name, data in images["dense"].items():
        assert data == images["sparse"][name] and len(data) > 0, name
    # the flag alone is refused
    r = subprocess.run(common + ["--net-bake-sparse", "--out", str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--net-bake-sparse" in r.stdout + r.stderr
