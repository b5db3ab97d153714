"""ct_network_bake_compact: the sparse bake with only the active nodes stored, behind a slot index (include/cloudtrace.h, "the
compact bake").

The slot index is an integer definition -- 0 off the mask, 1 + the rank in ascending node index on it -- restated in numpy
(network.bake_slots_reference); the device's slots are held to it word for word.  The stored table is held to the dense bake's
blocks of the active nodes bit for bit, the lookup to the SPARSE bake's lookup bit for bit on every input (positions no flight
can produce, a zero direction and a NaN included), and every frame, mean and M2 to the dense bake's.  There are no tolerances:
every comparison is np.array_equal on the bits.

Scene and weights: those of tests/test_network_render.py, as tests/test_network_bake_sparse.py takes them.  The active-node
counts (314, 1889, 78 150, 600 319, 4 802 552) are network.bake_mask_reference's on cloud() at the default step (M = 4)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import deepestscatter_amd as ds
from deepestscatter_amd import _lib
from deepestscatter_amd import network as N
from test_network_render import H, LIGHT2, SCALE, SID, SMALL, W, cloud, weights

GRID = ((9, 8, 7), 8, 3)        # 504 nodes, 314 of them active on cloud()
CLOSE_POSE = ((0.45, 0.3, -0.95), (0.0, 0.0, 0.0), 40.0)
STEP = ds.SceneParams().sample_step

_MASKS = {}


def reference_nodes(grid):
    """The reference mask's node bytes of cloud() at the default step, computed once per grid and left unchanged."""
    if grid not in _MASKS:
        _MASKS[grid] = N.bake_mask_reference(cloud(), grid, STEP)[1]
        _MASKS[grid].setflags(write=False)
    return _MASKS[grid]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------- CPU
def test_symbols_resolve_and_answer_null_arguments(product_lib):
    L = product_lib
    for name in ("ct_network_bake_compact", "ct_bake_storage_info", "ct_bake_slots", "ct_bake_download_stored"):
        assert hasattr(L, name) and name in _lib.EXPORTS
    d = _lib.CtBakeDesc(_lib.CT_ABI_VERSION, (C.c_uint32 * 3)(2, 2, 2), 4, 2)
    out = C.c_void_p()
    assert L.ct_network_bake_compact(None, None, C.byref(d), C.byref(out)) == _lib.CT_E_INVAL
    assert L.ct_network_bake_compact(None, None, None, None) == _lib.CT_E_INVAL
    assert L.ct_bake_storage_info(None, None) == _lib.CT_E_INVAL
    assert L.ct_bake_slots(None, None, 0) == _lib.CT_E_INVAL
    assert L.ct_bake_download_stored(None, None, 0) == _lib.CT_E_INVAL
    assert C.sizeof(_lib.CtBakeStorageInfo) == 40
    assert _lib.CtBakeStorageInfo.stored_entries.offset == 16 and _lib.CtBakeStorageInfo.index_bytes.offset == 32


def test_struct_layout_matches_the_header():
    import tempfile
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "cloudtrace.h"\nint main(){printf("%zu %zu %zu", sizeof(CtBakeStorageInfo), '
           'offsetof(CtBakeStorageInfo, stored_entries), offsetof(CtBakeStorageInfo, index_bytes));return 0;}')
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "p.c").write_text(src)
        subprocess.run(["gcc", "-I", str(root / "include"), "-o", f"{d}/p", f"{d}/p.c"], check=True)
        out = subprocess.run([f"{d}/p"], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [40, 16, 32]


@pytest.mark.parametrize("grid, active", [((9, 8, 7), 314), ((17, 17, 17), 1889), ((65, 65, 65), 78150)], ids=str)
def test_reference_slots_of_the_procedural_cloud(grid, active):
    nodes = reference_nodes(grid)
    slots = N.bake_slots_reference(nodes)
    assert slots.dtype == np.uint32 and slots.shape == nodes.shape and int(slots.max()) == active
    flat, on = slots.reshape(-1), nodes.reshape(-1) != 0
    assert np.array_equal(flat[on], np.arange(1, active + 1, dtype=np.uint32))   # 1, 2, 3, ... in index order
    assert not flat[~on].any() and (~on).any()


def test_reference_slots_of_an_empty_mask_and_of_a_full_one():
    assert not N.bake_slots_reference(N.bake_mask_reference(np.zeros((20, 33, 45), np.uint8), (6, 5, 4), STEP)[1]).any()
    full = N.bake_slots_reference(np.ones((3, 2, 2), np.uint8))
    assert np.array_equal(full.reshape(-1), np.arange(1, 13, dtype=np.uint32))


def test_the_active_nodes_of_65_are_active_at_the_even_nodes_of_129():
    """Node 2i of a 129 axis is node i of a 65 axis; every active node of (65, 65, 65) is active there in (129, 129, 129)."""
    coarse, fine = reference_nodes((65, 65, 65)), reference_nodes((129, 129, 129))
    assert int(coarse.sum()) == 78150 and int(fine.sum()) == 600319
    assert fine[::2, ::2, ::2][coarse != 0].all()
    assert 129 ** 3 * 4 * 8 == 68694048 > 2 ** 26 >= 600320 * 32


def test_sparse_and_compact_together_are_refused():
    with pytest.raises(ValueError):
        N.Bake(None, None, (2, 2, 2), 4, 2, sparse=True, compact=True)
    with pytest.raises(ValueError):
        ds.CloudTracer.network_bake(None, None, (2, 2, 2), 4, 2, sparse=True, compact=True)


# ---------------------------------------------------------------------------------------------------- GPU
def small_net(tr, negated=False):
    return N.Network(tr, weights(SMALL, negated), 32, 1, 1)


def crop():
    """The sparse file's recipe: 56 x 40 x 61 texels (z, y, x), rows of 61 bytes."""
    return np.ascontiguousarray(cloud()[4:60, 12:52, 1:62])


def _code(fn, *a, **kw):
    with pytest.raises(_lib.CloudTraceError) as e:
        fn(*a, **kw)
    return e.value.code


@pytest.fixture(scope="module")
def scene():
    """The module's tracer on cloud() as it is created, its small network, and the dense, the sparse and the compact bake of GRID.
    No test changes its light or accumulates on it."""
    with ds.CloudTracer(cloud(), width=W, height=H) as tr:
        made = []
        try:
            s = {"tr": tr, "net": small_net(tr)}
            made.append(s["net"])
            for key, kw in (("dense", {}), ("sparse", {"sparse": True}), ("compact", {"compact": True})):
                s[key] = tr.network_bake(s["net"], *GRID, **kw)
                made.append(s[key])
            yield s
        finally:
            for obj in reversed(made):
                obj.close()


def check_slots(bake, nodes):
    """The bake's slots, mask and sizes against the reference node bytes."""
    want = N.bake_slots_reference(nodes)
    got = bake.slots()
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    active, st, info = int(nodes.sum()), bake.storage_info, bake.info
    block = info["azimuths"] * info["cosines"]
    assert st == {"compact": True, "slots": active + 1, "stored_entries": (active + 1) * block,
                  "table_bytes": 4 * (active + 1) * block, "index_bytes": 4 * nodes.size}
    assert info["entries"] == nodes.size * block                      # the virtual count
    sp = bake.sparse_info
    assert sp["sparse"] and sp["active_nodes"] == active and sp["nodes"] == nodes.size and sp["margin_texels"] == 4
    assert np.array_equal(bake.mask(), nodes)
    return active


@pytest.mark.gpu
@pytest.mark.parametrize("grid", [(2, 2, 2), (9, 8, 7), (17, 17, 17), (48, 48, 48), (256, 2, 3)], ids=str)
def test_slots_equal_their_numpy_definition(scene, grid):
    """(2, 2, 2): every node active.  (48, 48, 48): 1728 waves, more than one per thread of the scan.  (256, 2, 3): cells narrower
    than a texel."""
    with scene["tr"].network_bake(scene["net"], grid, 4, 2, compact=True) as bake:
        active = check_slots(bake, reference_nodes(grid))
        assert 0 < active and (active < np.prod(grid) or grid == (2, 2, 2))


@pytest.mark.gpu
def test_slots_of_a_crop_with_ragged_rows():
    tex = crop()
    assert tex.shape == (56, 40, 61)
    with ds.CloudTracer(tex, width=W, height=H) as tr, small_net(tr) as net:
        for grid in ((9, 8, 7), (7, 5, 11)):
            with tr.network_bake(net, grid, 4, 2, compact=True) as bake:
                assert 0 < check_slots(bake, N.bake_mask_reference(tex, grid, STEP)[1]) < np.prod(grid)


def check_compact_bake(compact, sparse, dense):
    """stored_table() against the dense bake's blocks, table() against the sparse bake's table."""
    nodes = reference_nodes(GRID[0])
    assert check_slots(compact, nodes) == 314
    stored, table = compact.stored_table(), dense.table()
    assert stored.shape == (315, GRID[1], GRID[2]) and stored.dtype == np.float32
    assert not bits(stored[0]).any()                                  # 0.0f, not -0.0f
    rows = table.reshape(-1, GRID[1], GRID[2])[np.flatnonzero(nodes.reshape(-1))]
    assert np.array_equal(bits(stored[1:]), bits(rows)) and rows.any()
    assert np.array_equal(bits(compact.table()), bits(sparse.table()))
    for a, b in zip(compact.probes(), dense.probes()):
        assert np.array_equal(a, b)
    info = compact.info
    assert info["current"] and info["gather_ms"] > 0 and info["network_ms"] > 0


@pytest.mark.gpu
def test_stored_table_is_the_dense_bakes_blocks_of_the_active_nodes(scene, monkeypatch):
    check_compact_bake(scene["compact"], scene["sparse"], scene["dense"])
    for bake in (scene["dense"], scene["sparse"]):                    # every kind of bake answers ct_bake_storage_info
        assert bake.storage_info == {"compact": False, "slots": 504, "stored_entries": 504 * 24, "table_bytes": 4 * 504 * 24, "index_bytes": 0}
    # in pieces of 48 records (2512 = 52 x 48 + 16: a partial last piece), and with fixed-point texture weights
    monkeypatch.setenv("CT_NET_DESC_RECORDS", "48")
    with ds.CloudTracer(cloud(), width=W, height=H) as t2, small_net(t2) as net, t2.network_bake(net, *GRID) as d2, \
            t2.network_bake(net, *GRID, sparse=True) as s2, t2.network_bake(net, *GRID, compact=True) as c2:
        assert t2.network_scratch()["desc_cap"] == 48
        check_compact_bake(c2, s2, d2)
        assert np.array_equal(bits(c2.stored_table()), bits(scene["compact"].stored_table()))   # the pieces change nothing
    monkeypatch.delenv("CT_NET_DESC_RECORDS")
    with ds.CloudTracer(cloud(), width=W, height=H, flags=_lib.CT_FLAG_TEX_FIXED8) as t3, small_net(t3) as net, \
            t3.network_bake(net, *GRID) as d3, t3.network_bake(net, *GRID, sparse=True) as s3, t3.network_bake(net, *GRID, compact=True) as c3:
        assert not np.array_equal(d3.table(), scene["dense"].table())
        check_compact_bake(c3, s3, d3)


@pytest.mark.gpu
def test_lookup_is_the_sparse_bakes_everywhere(scene):
    import torch
    tr, dense, sparse, compact = scene["tr"], scene["dense"], scene["sparse"], scene["compact"]
    rng = np.random.default_rng(12)
    n = 4096
    box = np.array(tr.dims, np.float32) / np.float32(max(tr.dims))
    pos = (rng.uniform(-0.5, 0.5, (n, 3)) * (box + 0.02)).astype(np.float32)      # the box enlarged by 0.01 per side
    d = rng.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    d[0] = compact.info["light"]                                      # exactly along the light: the azimuth has no direction
    d[1] = 0                                                          # a zero direction
    pos[2] = np.nan                                                   # a NaN position
    dev = tr.descriptor_frame(1)[1].device
    p_dev, d_dev = torch.from_numpy(pos).to(dev), torch.from_numpy(d).to(dev)
    got = tr.bake_lookup(compact, p_dev, d_dev).cpu().numpy()
    want = tr.bake_lookup(sparse, p_dev, d_dev).cpu().numpy()
    assert np.array_equal(bits(got), bits(want))
    full = tr.bake_lookup(dense, p_dev, d_dev).cpu().numpy()
    assert not np.array_equal(bits(got), bits(full)) and want.any()   # most positions lie far from the cloud: zeros are interpolated
    # at the records of a flight the three agree
    for sid in range(1, 5):
        _, rp, rd, _ = tr.descriptor_frame(sid)
        assert len(rp) >= 50
        got = tr.bake_lookup(compact, rp, rd).cpu().numpy()
        assert np.array_equal(bits(got), bits(tr.bake_lookup(dense, rp, rd).cpu().numpy())), sid
        assert np.array_equal(bits(got), bits(tr.bake_lookup(sparse, rp, rd).cpu().numpy())), sid
        assert (got > 0).any() and (got < 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("pose", ["default", "close"])
def test_frames_are_the_dense_bakes_frames(pose):
    with ds.CloudTracer(cloud(), width=W, height=H) as tr, small_net(tr) as net, tr.network_bake(net, *GRID) as dense, \
            tr.network_bake(net, *GRID, compact=True) as compact:
        if pose == "close":
            eye, lookat, fov = CLOSE_POSE
            tr.set_camera(eye, *ds.calculate_camera_variables(eye, lookat, (0, 1, 0), fov, W / H))
        for transform in ("linear", "expm1"):
            for direct in (False, True):
                for band in (0, W):                                   # the whole frame at once, and one row per band
                    kw = dict(transform=transform, rgb_scale=SCALE, direct=direct, band_pixels=band)
                    want = tr.baked_render_subframe(dense, SID, **kw).cpu().numpy()
                    got = tr.baked_render_subframe(compact, SID, **kw).cpu().numpy()
                    assert np.array_equal(bits(got), bits(want)) and want[..., :3].any(), (transform, direct, band)
        tr.baked_render_accumulate(dense, 1, 4, rgb_scale=SCALE, direct=True)
        mean, m2 = tr.mean(), tr.m2()
        tr.reset()
        tr.baked_render_accumulate(compact, 1, 4, rgb_scale=SCALE, direct=True)
        assert tr.subframes == 4 and np.array_equal(bits(tr.mean()), bits(mean)) and np.array_equal(bits(tr.m2()), bits(m2)) and m2.any()


@pytest.mark.gpu
def test_a_shards_frame_is_the_dense_bakes():
    with ds.CloudTracer(cloud(), width=27, height=13, shard_index=1, shard_count=3) as tr, small_net(tr) as net, \
            tr.network_bake(net, *GRID) as dense, tr.network_bake(net, *GRID, compact=True) as compact:
        want = tr.baked_render_shard_subframe(dense, SID, rgb_scale=SCALE).cpu().numpy()
        got = tr.baked_render_shard_subframe(compact, SID, rgb_scale=SCALE).cpu().numpy()
        assert np.array_equal(bits(got), bits(want)) and want[..., :3].any()
        tr.baked_render_shard_accumulate(dense, 1, 3, rgb_scale=SCALE)
        mean, m2 = tr.mean(), tr.m2()
        tr.reset()
        tr.baked_render_shard_accumulate(compact, 1, 3, rgb_scale=SCALE)
        assert np.array_equal(bits(tr.mean()), bits(mean)) and np.array_equal(bits(tr.m2()), bits(m2)) and mean.any()


@pytest.mark.gpu
def test_update_of_a_compact_bake_stays_compact():
    with ds.CloudTracer(cloud(), width=W, height=H) as tr, small_net(tr) as net, tr.network_bake(net, *GRID, compact=True) as bake:
        old, slots, storage = bake.stored_table(), bake.slots(), bake.storage_info
        tr.set_light(LIGHT2)
        assert not bake.info["current"]
        assert _code(tr.baked_render_subframe, bake, SID) == _lib.CT_E_STATE
        with ds.CloudTracer(cloud(), width=W, height=H) as other, small_net(other) as foreign:   # a failing update changes nothing
            assert tr.L.ct_bake_update(other.h, foreign.n, bake.b) == _lib.CT_E_INVAL
        assert np.array_equal(bits(bake.stored_table()), bits(old)) and not bake.info["current"]
        bake.update(net)
        assert bake.info["current"] and np.array_equal(bake.info["light"], tr.light_direction())
        assert np.array_equal(bake.slots(), slots) and bake.storage_info == storage and storage["compact"]
        assert bake.sparse_info["active_nodes"] == 314
        with ds.CloudTracer(cloud(), width=W, height=H, light_direction=LIGHT2) as fresh, small_net(fresh) as n2, \
                fresh.network_bake(n2, *GRID) as dense, fresh.network_bake(n2, *GRID, compact=True) as again:
            assert np.array_equal(bits(bake.stored_table()), bits(again.stored_table()))
            assert not np.array_equal(bits(bake.stored_table()), bits(old))
            want = fresh.baked_render_subframe(dense, SID, rgb_scale=SCALE).cpu().numpy()
        assert np.array_equal(bits(tr.baked_render_subframe(bake, SID, rgb_scale=SCALE).cpu().numpy()), bits(want)) and want[..., :3].any()


@pytest.mark.gpu
def test_a_grid_beyond_the_dense_limit():
    """(129, 129, 129) x 4 x 8 has 68 694 048 virtual entries, more than 2^26: no dense or sparse bake of it exists, the compact
    one stores 600 320 x 32.  (With 4 x 2 polar nodes the grid would have 17 173 512 entries and a dense bake: 68 694 048 is
    129^3 x 32.)  Node 2i of a 129 axis is node i of a 65 axis with the same float, and every active node of (65, 65, 65) is
    active there (the CPU test above), so the stored blocks of the even nodes are the (65, 65, 65) compact bake's, bit for bit.
    A lit pixel is a pixel with a record of the flight (descriptor_frame's pixel list): every other pixel holds the miss value."""
    fine_grid, coarse_grid = (129, 129, 129), (65, 65, 65)
    with ds.CloudTracer(cloud(), width=W, height=H) as tr, small_net(tr) as net:      # (its own tracer: the bake grows the scratch)
        frames, lit = beyond_the_dense_limit(tr, net, fine_grid, coarse_grid)
    assert 50 <= lit.sum() < W * H
    for frame in frames:
        assert np.isfinite(frame).all() and frame[..., :3].any()
        assert np.all(frame[~lit] == np.array([0, 0, 0, 1], np.float32)) and np.all(frame[lit][:, 3] == 1)


def beyond_the_dense_limit(tr, net, fine_grid, coarse_grid):
    d = _lib.CtBakeDesc(_lib.CT_ABI_VERSION, (C.c_uint32 * 3)(*fine_grid), 4, 8)
    out = C.c_void_p()
    for entry in (tr.L.ct_network_bake, tr.L.ct_network_bake_sparse):
        assert entry(tr.h, net.n, C.byref(d), C.byref(out)) == _lib.CT_E_INVAL and not out.value
    with tr.network_bake(net, fine_grid, 4, 8, compact=True) as fine, tr.network_bake(net, coarse_grid, 4, 8, compact=True) as coarse:
        assert fine.info["entries"] == 68694048 > 2 ** 26
        st = fine.storage_info
        assert st["compact"] and st["slots"] == 600320 and st["stored_entries"] == 600320 * 32 and st["index_bytes"] == 4 * 129 ** 3
        assert fine.sparse_info["active_nodes"] == 600319 and coarse.sparse_info["active_nodes"] == 78150
        fine_slots, coarse_slots = fine.slots(), coarse.slots()
        assert np.array_equal(fine_slots, N.bake_slots_reference(reference_nodes(fine_grid)))
        assert np.array_equal(coarse_slots, N.bake_slots_reference(reference_nodes(coarse_grid)))
        on = coarse_slots != 0
        at_even = fine_slots[::2, ::2, ::2][on]
        assert at_even.all() and len(at_even) == 78150
        fine_blocks, coarse_blocks = fine.stored_table()[at_even], coarse.stored_table()[coarse_slots[on]]
        assert np.array_equal(bits(fine_blocks), bits(coarse_blocks)) and coarse_blocks.any()
        frames = [tr.baked_render_subframe(b, SID, rgb_scale=SCALE).cpu().numpy() for b in (fine, coarse)]
    lit = np.zeros(W * H, bool)
    lit[tr.descriptor_frame(SID)[3].cpu().numpy()] = True
    return frames, lit.reshape(H, W)


@pytest.mark.gpu
def test_errors_leave_the_handle_usable(scene):
    tr, net, dense, sparse, compact = scene["tr"], scene["net"], scene["dense"], scene["sparse"], scene["compact"]
    L, h = tr.L, tr.h
    want = tr.baked_render_subframe(compact, SID, rgb_scale=SCALE).cpu().numpy()
    assert np.array_equal(bits(want), bits(tr.baked_render_subframe(dense, SID, rgb_scale=SCALE).cpu().numpy()))
    scratch = tr.network_scratch()

    def unchanged():
        assert np.array_equal(bits(tr.baked_render_subframe(compact, SID, rgb_scale=SCALE).cpu().numpy()), bits(want))
        assert tr.network_scratch() == scratch

    def desc(grid=(2, 2, 2), nphi=4, nc=2, abi=_lib.CT_ABI_VERSION):
        return _lib.CtBakeDesc(abi, (C.c_uint32 * 3)(*grid), nphi, nc)

    def message():
        return L.ct_last_error(h).decode()

    # more stored entries than a table holds: (4 802 552 + 1) x 16 = 76 840 848 > 2^26, known only after the mask
    out = C.c_void_p(1)
    d = desc((256, 256, 256), 4, 4)
    assert L.ct_network_bake_compact(h, net.n, C.byref(d), C.byref(out)) == _lib.CT_E_INVAL and not out.value
    assert "76840848" in message() and "67108864" in message() and "4802552" in message()
    unchanged()
    # bake_create's argument errors, in their order: abi, grid, azimuths, cosines, network
    for kw, word in ((dict(abi=_lib.CT_ABI_VERSION + 1, grid=(1, 2, 2), nphi=6, nc=1), "abi_version"),
                     (dict(grid=(1, 2, 2), nphi=6, nc=1), "grid[0]"), (dict(grid=(2, 257, 2), nphi=6, nc=1), "grid[1]"),
                     (dict(grid=(2, 2, 0), nphi=0), "grid[2]"), (dict(nphi=6, nc=1), "azimuths"), (dict(nphi=0, nc=65), "azimuths"),
                     (dict(nphi=68), "azimuths"), (dict(nc=1), "cosines"), (dict(nc=65), "cosines")):
        d, out = desc(**kw), C.c_void_p(1)
        assert L.ct_network_bake_compact(h, net.n, C.byref(d), C.byref(out)) == _lib.CT_E_INVAL and not out.value, kw
        assert word in message() and "ct_network_bake_compact" in message(), (kw, message())
    d = desc()
    assert L.ct_network_bake_compact(h, None, C.byref(d), C.byref(out)) == _lib.CT_E_INVAL
    assert L.ct_network_bake_compact(h, net.n, None, C.byref(out)) == _lib.CT_E_INVAL
    assert L.ct_network_bake_compact(h, net.n, C.byref(d), None) == _lib.CT_E_INVAL
    from test_network_render import seeded_weights
    shape = N.NetworkShape(32, 0, 1)
    with N.Network(tr, seeded_weights(shape, 2), shape.width, shape.aux, shape.head_layers) as no_aux:
        assert _code(tr.network_bake, no_aux, (2, 2, 2), 4, 2, compact=True) == _lib.CT_E_INVAL
    unchanged()
    # ct_bake_slots and ct_bake_download_stored: only on a compact bake, and only with the exact count
    words, floats = np.empty(505, np.uint32), np.empty(504 * 24 + 1, np.float32)
    for bake in (dense, sparse):
        assert L.ct_bake_slots(bake.b, words.ctypes.data_as(C.c_void_p), 504) == _lib.CT_E_INVAL
        assert L.ct_bake_download_stored(bake.b, floats.ctypes.data_as(C.c_void_p), 504 * 24) == _lib.CT_E_INVAL
        assert _code(bake.slots) == _lib.CT_E_INVAL and _code(bake.stored_table) == _lib.CT_E_INVAL
    for count in (503, 505, 0):
        assert L.ct_bake_slots(compact.b, words.ctypes.data_as(C.c_void_p), count) == _lib.CT_E_INVAL
    for count in (315 * 24 - 1, 315 * 24 + 1, 504 * 24, 0):
        assert L.ct_bake_download_stored(compact.b, floats.ctypes.data_as(C.c_void_p), count) == _lib.CT_E_INVAL
    for count in (315 * 24, 504 * 24 - 1, 0):                          # ct_bake_download takes the virtual count
        assert L.ct_bake_download(compact.b, floats.ctypes.data_as(C.c_void_p), count) == _lib.CT_E_INVAL
    assert L.ct_bake_slots(compact.b, None, 504) == _lib.CT_E_INVAL
    assert L.ct_bake_download_stored(compact.b, None, 315 * 24) == _lib.CT_E_INVAL
    assert L.ct_bake_storage_info(compact.b, None) == _lib.CT_E_INVAL
    unchanged()


@pytest.mark.gpu
def test_an_empty_volume_stores_one_zero_slot():
    grid = (6, 5, 4)
    with ds.CloudTracer(np.zeros((20, 33, 45), np.uint8), width=W, height=H) as tr, small_net(tr) as net, \
            tr.network_bake(net, grid, 4, 2, compact=True) as bake, tr.network_bake(net, grid, 4, 2) as dense:
        info, st = bake.info, bake.storage_info
        assert st == {"compact": True, "slots": 1, "stored_entries": 8, "table_bytes": 32, "index_bytes": 4 * 120}
        assert info["gather_ms"] == 0 and info["network_ms"] == 0 and info["current"] and info["entries"] == 120 * 8
        assert not bake.slots().any() and not bake.mask().any() and bake.sparse_info["active_nodes"] == 0
        assert bake.stored_table().shape == (1, 4, 2) and not bits(bake.stored_table()).any() and not bits(bake.table()).any()
        want = tr.baked_render_subframe(dense, SID).cpu().numpy()
        frame = tr.baked_render_subframe(bake, SID).cpu().numpy()
        assert np.array_equal(bits(frame), bits(want)) and np.all(frame == np.array([0, 0, 0, 1], np.float32))


@pytest.mark.gpu
def test_cli_writes_the_same_image_with_a_compact_bake(tmp_path):
    from deepestscatter_amd import build
    cli = build.build_cli()
    N.save_weights(tmp_path / "w.bin", weights(SMALL), SMALL)
    common = [str(cli), "procedural:64", "--network", str(tmp_path / "w.bin"), "--size", f"{W}x{H}", "--spp", "4", "--net-scale", "0.5,2,3"]
    images = {}
    for name, extra in (("sparse", ["--net-bake-sparse"]), ("compact", ["--net-bake-compact"])):
        (tmp_path / name).mkdir()
        r = subprocess.run(common + ["--net-baked", "9,8,7,8,3"] + extra + ["--out", str(tmp_path / name)], capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        images[name] = {p.name: p.read_bytes() for p in sorted((tmp_path / name).glob("*.exr"))}
    assert len(images["sparse"]) >= 2 and images["sparse"].keys() == images["compact"].keys()
    for name, data in images["sparse"].items():
        assert data == images["compact"][name] and len(data) > 0, name
    # the flag alone is refused, and so are the two ways to bake together
    r = subprocess.run(common + ["--net-bake-compact", "--out", str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--net-bake-compact" in r.stdout + r.stderr and "--net-baked" in r.stdout + r.stderr
    r = subprocess.run(common + ["--net-baked", "9,8,7,8,3", "--net-bake-sparse", "--net-bake-compact", "--out", str(tmp_path)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--net-bake-sparse" in r.stdout + r.stderr and "--net-bake-compact" in r.stdout + r.stderr
