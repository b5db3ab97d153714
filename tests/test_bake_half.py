"""Half tables: ct_bake_half, a bake whose stored table is IEEE binary16 (include/cloudtrace.h, "half tables").

Every comparison is on the bits.  The stored bits are network.half_round_reference of the float32 table (numpy's float32 ->
float16 conversion), the rounding table of the issue is held in hand-computed bit patterns, and every lookup and frame is the
float32 definition (network.bake_lookup_reference, tests/test_network_baked.py's composition) applied to the widened table.

Scene and grids: those of tests/test_bake_file.py -- 5 x 4 x 3 x 4 with 3 polar nodes (odd: pairs at odd half offsets) and 2."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import deepestscatter_amd as ds
from deepestscatter_amd import _lib
from deepestscatter_amd import cloudtrace as ct
from deepestscatter_amd import network as N
from test_bake_file import (DELTA, GRID2, GRID3, H, LIGHT2, SAMPLES, SCALE, SID, STEP, W, _code, accessors, bits, frames, header_of, lookups, make,
                            records, reference_bytes, same, small_net, tracer, volume, write)

f32 = np.float32

# float32 input -> binary16 bits (None: ct_bake_half refuses the table)
ROUNDING = [
    (f32(65519.996), 0x7BFF),                                  # the largest float32 below the tie to infinity
    (f32(2.0 ** -25), 0x0000),                                 # the tie between 0 and the smallest subnormal: to even
    (np.nextafter(f32(2.0 ** -25), f32(1)), 0x0001),           # just above it
    (f32(1 + 2.0 ** -11), 0x3C00),                             # a tie: to the even mantissa below
    (f32(1 + 3 * 2.0 ** -11), 0x3C02),                         # a tie: to the even mantissa above
    (f32(-0.0), 0x8000),                                       # the sign of zero
    (f32(65520.0), None),
    (f32(np.nan), None),
]
MORE = [(f32(65504.0), 0x7BFF), (f32(-65519.996), 0xFBFF), (f32(2.0 ** -24), 0x0001), (f32(2.0 ** -14), 0x0400), (f32(2.0 ** -14 - 2.0 ** -25), 0x0400),
        (f32(1.5 * 2.0 ** -24), 0x0002), (f32(2.5 * 2.0 ** -24), 0x0002), (f32(-2.0 ** -26), 0x8000), (f32(1.0), 0x3C00), (f32(-2.0), 0xC000),
        (f32(0.1), 0x2E66), (f32(1e-10), 0x0000)]


# ---------------------------------------------------------------------------------------------------- CPU
def test_symbols_resolve_and_answer_null_arguments(product_lib):
    L = product_lib
    for name in ("ct_bake_half", "ct_bake_format", "ct_bake_download_half", "ct_debug_half_round"):
        assert hasattr(L, name) and name in _lib.EXPORTS
    out, word = C.c_void_p(1), C.c_uint32(7)
    assert L.ct_bake_half(None, None, C.byref(out)) == _lib.CT_E_INVAL
    assert L.ct_bake_format(None, C.byref(word)) == _lib.CT_E_INVAL and L.ct_bake_format(None, None) == _lib.CT_E_INVAL
    assert L.ct_bake_download_half(None, None, 0) == _lib.CT_E_INVAL
    assert (_lib.CT_BAKE_F32, _lib.CT_BAKE_F16) == (0, 1) == (N.BAKE_F32, N.BAKE_F16)


def test_the_rounding_table_in_hand_computed_bits(product_lib):
    values = np.array([v for v, _ in ROUNDING + MORE], f32)
    want = [b for _, b in ROUNDING + MORE]
    got, refused = N.half_round_reference(values)
    assert got.dtype == np.uint16 and refused.dtype == bool
    for v, b, g, r in zip(values, want, got, refused):
        assert r == (b is None), v
        if b is not None:
            assert int(g) == b, (v, hex(int(g)), hex(b))
            assert product_lib.ct_debug_half_round(float(v)) == b               # the conversion kernel's own rounding, on the host
    assert product_lib.ct_debug_half_round(65520.0) == 0x7C00 and product_lib.ct_debug_half_round(float("-inf")) == 0xFC00
    # the library's rounding against numpy's on a sweep of bit patterns: every exponent, ties and their neighbours
    rng = np.random.default_rng(4)
    sweep = np.concatenate([rng.integers(0, 2 ** 32, 20000, dtype=np.uint64).astype(np.uint32),
                            (np.arange(0, 2 ** 16, dtype=np.uint32) << 13 | 0x1000) + 0x33000000 - 0x1000,
                            np.arange(0x477FE000 - 64, 0x477FE000 + 12000, 97, dtype=np.uint32)])
    values = sweep.view(f32)
    ref, refused = N.half_round_reference(values)
    keep = ~np.isnan(values)
    mine = np.array([product_lib.ct_debug_half_round(float(v)) for v in values[keep]], np.uint16)
    assert np.array_equal(mine, ref[keep]) and refused[keep].any() and not refused[keep].all()
    assert np.array_equal(refused, ~(np.abs(values) < f32(65520.0)))


# ---------------------------------------------------------------------------------------------------- GPU
def hand_written(tr, values, kind=0, grid=(2, 2, 2), nphi=4, nc=3, nodes=None):
    """A float32 bake file of this tracer's scene whose stored table holds `values` first and small numbers behind them."""
    n = grid[0] * grid[1] * grid[2]
    active = n if nodes is None else int(nodes.sum())
    stored = (active + 1) * nphi * nc if kind == 2 else n * nphi * nc
    table = (np.arange(stored, dtype=f32) * f32(0.001)).astype(f32)
    table[:len(values)] = values
    p = tr.params
    word = lambda v: int(np.array(v, f32).view(np.uint32))
    with tr.traced_bake((2, 2, 2), 4, 2, 0) as frame:                       # the frame of this light, as the library makes it
        i = frame.info
    h = header_of(kind, 0, 0, 0, grid, nphi, nc, active=active, light=i["light"], axis_a=i["axis_a"], axis_b=i["axis_b"], dims=tr.dims,
                  estimator=p.estimator, tex_fixed8=0, sample_step_bits=word(p.sample_step), volume_hash=tr.volume_hash())
    return N.write_bake_file_reference(h, table, nodes=nodes), table


@pytest.mark.gpu
def test_the_rounding_table_through_a_hand_written_file(tmp_path):
    """Stored counts 96 (2 x 2 x 2 x 4 x 3) and 336 (28 slots of 4 x 3): multiples of neither 64 nor 256, so the conversion kernel's
    last wave and last block are partial.  (An odd stored count does not exist: Nphi is a multiple of 4, and ct_bake_file_info
    refuses a stored_entries that is not the grid's.)"""
    good = np.array([v for v, b in ROUNDING + MORE if b is not None], f32)
    want = np.array([b for _, b in ROUNDING + MORE if b is not None], np.uint16)
    with tracer() as tr:
        data, table = hand_written(tr, good)
        assert len(table) == 96
        with tr.load_bake(write(tmp_path, data)) as src, src.half() as half:
            assert src.format == 0 and half.format == 1 and half.info["current"]
            got = half.half_table().reshape(-1)
            assert np.array_equal(got[:len(want)], want)
            assert np.array_equal(got, N.half_round_reference(table)[0])
            assert np.array_equal(bits(half.table().reshape(-1)), bits(got.view(np.float16).astype(f32)))      # widened: exact
            assert half.storage_info["table_bytes"] == 2 * 96 and src.storage_info["table_bytes"] == 4 * 96
        full = N.bake_mask_reference(volume(), (3, 3, 3), STEP)[1].reshape(-1)
        assert full.all()                                                   # (this handle's mask of the grid: every node)
        data, table = hand_written(tr, good, kind=2, grid=(3, 3, 3), nodes=full)
        with tr.load_bake(write(tmp_path, data, "c.bake")) as src, src.half() as half:
            assert half.storage_info["stored_entries"] == 336 == len(table) and half.storage_info["compact"]
            assert np.array_equal(half.half_table().reshape(-1), N.half_round_reference(table)[0])
            assert np.array_equal(half.half_table().reshape(-1)[:len(want)], want)
        base = (np.arange(96, dtype=f32) * f32(0.001)).astype(f32)
        base[:len(good)] = good
        for value, where in ((f32(65520.0), 0), (f32(np.nan), 95), (f32(-np.inf), 41), (f32(1e6), 64)):
            bad = base.copy()
            bad[where] = value
            with tr.load_bake(write(tmp_path, hand_written(tr, bad)[0], "bad.bake")) as src:
                held = ct.debug_allocations()
                out = C.c_void_p(1)
                assert tr.L.ct_bake_half(tr.h, src.b, C.byref(out)) == _lib.CT_E_INVAL and not out.value
                message = tr.L.ct_last_error(tr.h).decode()
                assert "1 stored values" in message and f"stored index {where}" in message, message
                assert ct.debug_allocations() == held
                assert np.array_equal(bits(src.table().reshape(-1)), bits(bad))
        two = base.copy()
        two[[17, 80]] = f32(70000.0), f32(np.inf)
        with tr.load_bake(write(tmp_path, hand_written(tr, two)[0], "two.bake")) as src:
            assert _code(src.half) == _lib.CT_E_INVAL
            assert "2 stored values" in tr.L.ct_last_error(tr.h).decode() and "stored index 17" in tr.L.ct_last_error(tr.h).decode()


@pytest.fixture(scope="module")
def scene():
    """A tracer of SMALL with the traced dense, sparse and compact bakes of GRID3 and their half copies.  No test changes its light."""
    with tracer(small=True) as tr:
        made = []
        try:
            s = {"tr": tr}
            for kind in ("dense", "sparse", "compact"):
                s[kind] = make(tr, "traced", kind)
                s[kind + "_half"] = s[kind].half()
                made += [s[kind], s[kind + "_half"]]
            yield s
        finally:
            for obj in reversed(made):
                obj.close()


@pytest.mark.gpu
def test_the_bits_are_the_rounded_table(scene):
    on = np.repeat(scene["sparse"].mask().reshape(-1) != 0, 12)
    assert 0 < on.sum() < on.size
    for kind in ("dense", "sparse", "compact"):
        src, half = scene[kind], scene[kind + "_half"]
        stored = src.stored_table() if kind == "compact" else src.table()
        want, refused = N.half_round_reference(stored)
        assert not refused.any() and stored.any()
        assert half.format == 1 and src.format == 0
        assert np.array_equal(half.half_table(), want)
        wide = want.view(np.float16).astype(f32)
        assert np.array_equal(bits(half.stored_table() if kind == "compact" else half.table()), bits(wide))
        assert not np.array_equal(bits(wide), bits(stored))                 # the rounding is visible
        a, _ = accessors(src)
        b, _ = accessors(half)
        for key in a:                                                       # everything but the table and the format is carried over
            if key in ("table", "stored", "format", "storage.table_bytes") or key.startswith("adaptive."):
                continue
            assert np.array_equal(np.atleast_1d(a[key]), np.atleast_1d(b[key])), key
        assert b["storage.table_bytes"] * 2 == a["storage.table_bytes"] and b["trace.traced"] and b["trace.samples"] == SAMPLES
        assert not b["adaptive.adaptive"]
    dense, sparse, compact = (scene[k + "_half"] for k in ("dense", "sparse", "compact"))
    assert np.array_equal(dense.half_table().reshape(-1)[on], sparse.half_table().reshape(-1)[on])
    assert np.array_equal(compact.half_table()[1:].reshape(-1), sparse.half_table().reshape(-1)[on]) and not compact.half_table()[0].any()
    assert np.array_equal(bits(compact.table()), bits(sparse.table()))      # ct_bake_download expands the widened blocks


@pytest.mark.gpu
@pytest.mark.parametrize("grid", [GRID3, GRID2], ids=["nc3", "nc2"])
def test_lookups_are_the_float32_definition_on_the_widened_table(scene, grid):
    import torch
    tr = scene["tr"]
    box = np.array(tr.dims, f32) / f32(max(tr.dims))
    for kind in ("dense", "compact"):
        if grid is GRID3:
            check(tr, scene[kind + "_half"], box, torch)
        else:
            with make(tr, "traced", kind, grid) as src, src.half() as half:
                check(tr, half, box, torch)


def check(tr, half, box, torch):
    table, info = half.table(), half.info
    for n in (1, 63, 65, 257):
        pos, d = records(tr, n, nan=False)
        want = N.bake_lookup_reference(table, info, box, pos, d)
        got = tr.bake_lookup(half, torch.from_numpy(pos).cuda(), torch.from_numpy(d).cuda()).cpu().numpy()
        assert np.array_equal(bits(got), bits(want)), n
    assert np.isfinite(want).all() and np.ptp(want) > 0


@pytest.mark.gpu
def test_frames_fused_and_loop_are_the_definition_on_the_widened_table(scene):
    from test_network_baked import baked_definition
    tr = scene["tr"]
    for kind in ("dense", "compact"):
        half = scene[kind + "_half"]
        want = baked_definition(tr, half, SID, "linear", SCALE)[0]           # (bake.table(): the widened table)
        got = tr.baked_render_subframe(half, SID, rgb_scale=SCALE).cpu().numpy()
        assert np.array_equal(bits(got), bits(want)) and want[..., :3].any()
        assert not np.array_equal(bits(got), bits(tr.baked_render_subframe(scene[kind], SID, rgb_scale=SCALE).cpu().numpy()))
    assert np.array_equal(bits(tr.baked_render_subframe(scene["sparse_half"], SID, rgb_scale=SCALE).cpu().numpy()), bits(got))
    for direct in (False, True):                                            # fused = the loop of subframe + accumulate
        tr.reset()
        tr.baked_render_accumulate(scene["compact_half"], 1, 3, rgb_scale=SCALE, direct=direct)
        mean, m2 = tr.mean(), tr.m2()
        tr.reset()
        for sid in (1, 2, 3):
            tr.baked_render_subframe(scene["compact_half"], sid, rgb_scale=SCALE, direct=direct)
            tr.accumulate(sid)
        assert tr.subframes == 3 and np.array_equal(bits(tr.mean()), bits(mean)) and np.array_equal(bits(tr.m2()), bits(m2)) and m2.any()
        tr.reset()


@pytest.mark.gpu
def test_shard_frames_are_the_unsharded_frame_cut_by_tiles():
    w, h, count = 27, 13, 3
    with tracer(small=True, w=w, h=h) as tr, make(tr, "traced", "compact") as src, src.half() as half:
        whole = tr.baked_render_subframe(half, SID, rgb_scale=SCALE, direct=True).cpu().numpy()
        tr.baked_render_accumulate(half, 1, 3, rgb_scale=SCALE)
        whole_mean, whole_m2 = tr.mean(), tr.m2()
    ys, xs = np.mgrid[0:h, 0:w]
    total, sums = np.zeros((h, w, 4), f32), [np.zeros((h, w, 4), f32), np.zeros((h, w, 4), f32)]
    for index in range(count):
        own = np.vectorize(lambda x, y: ds.tile_owner(int(x) // 8, int(y) // 8, count) == index)(xs, ys)
        with tracer(small=True, w=w, h=h, shard_index=index, shard_count=count) as tr, make(tr, "traced", "compact") as src, src.half() as half:
            got = tr.baked_render_shard_subframe(half, SID, rgb_scale=SCALE, direct=True, band_pixels=64).cpu().numpy()
            assert np.array_equal(bits(got[own]), bits(whole[own])) and not got[~own].any()
            total += got
            tr.baked_render_shard_accumulate(half, 1, 3, rgb_scale=SCALE)
            sums[0] += tr.mean()
            sums[1] += tr.m2()
    assert np.array_equal(bits(total), bits(whole)) and whole[..., :3].any()
    assert np.array_equal(bits(sums[0]), bits(whole_mean)) and np.array_equal(bits(sums[1]), bits(whole_m2)) and whole_m2.any()


@pytest.mark.gpu
def test_a_half_bake_is_final(scene, tmp_path):
    tr = scene["tr"]
    L, h = tr.L, tr.h
    half = scene["compact_half"]
    before = half.half_table()

    def final(fn, *a):
        assert _code(fn, *a) == _lib.CT_E_INVAL
        assert "from float32" in L.ct_last_error(h).decode(), L.ct_last_error(h).decode()

    with small_net(tr) as net:
        final(half.update, net)
        with tr.network_bake(net, *GRID3, compact=True) as nb, nb.half() as nh:
            final(nh.update, net)                                           # a network's half bake, too
            assert not nh.trace_info()["traced"] and np.array_equal(nh.half_table(), N.half_round_reference(nb.stored_table())[0])
    for fn, a in ((half.trace_more, (1,)), (half.retrace, (4,)), (half.trace_adaptive_more, (16,)), (half.retrace_adaptive, ()), (half.half, ())):
        final(fn, *a)
    assert _code(half.counts) == _lib.CT_E_INVAL and _code(half.m2) == _lib.CT_E_INVAL
    assert _code(scene["compact"].half_table) == _lib.CT_E_INVAL            # a float32 bake holds no binary16 table
    words = np.empty(half.storage_info["stored_entries"] + 1, np.uint16)
    for count in (0, words.size - 2, words.size):
        assert L.ct_bake_download_half(half.b, words.ctypes.data_as(C.c_void_p), count) == _lib.CT_E_INVAL
    assert L.ct_bake_download_half(half.b, None, words.size - 1) == _lib.CT_E_INVAL
    with tracer(small=True) as other:
        out = C.c_void_p(1)
        assert L.ct_bake_half(other.h, scene["compact"].b, C.byref(out)) == _lib.CT_E_INVAL and not out.value
        assert "another handle" in L.ct_last_error(other.h).decode()
    assert L.ct_bake_half(h, scene["compact"].b, None) == _lib.CT_E_INVAL
    assert np.array_equal(half.half_table(), before)
    # an adaptive source: the half copy is not adaptive; the source goes on
    with tr.traced_bake_adaptive(*GRID3, round_samples=4, max_samples=8, rel_tol=0.7, zero_samples=7, compact=True) as ad, ad.half() as adh:
        assert not adh.adaptive_info()["adaptive"] and adh.trace_info()["samples"] == ad.trace_info()["samples"] == 8
        assert np.array_equal(adh.half_table(), N.half_round_reference(ad.stored_table())[0])
        ad.trace_adaptive_more(16)
    # the source can be destroyed; after ct_set_light the half bake is simply not current
    with tracer(small=True) as t2:
        src = make(t2, "traced", "sparse")
        keep = src.half()
        want = N.half_round_reference(src.table())[0]
        src.close()
        assert np.array_equal(keep.half_table(), want) and t2.baked_render_subframe(keep, SID, rgb_scale=SCALE).cpu().numpy()[..., :3].any()
        t2.set_light(LIGHT2)
        assert not keep.info["current"] and _code(t2.baked_render_subframe, keep, SID) == _lib.CT_E_STATE
        assert _code(keep.retrace, 4) == _lib.CT_E_INVAL
        keep.close()


@pytest.mark.gpu
def test_save_and_load_of_a_half_bake(scene, tmp_path):
    tr = scene["tr"]
    for kind in ("dense", "sparse", "compact"):
        half = scene[kind + "_half"]
        path = tmp_path / f"{kind}.bake"
        half.save(path)
        data = path.read_bytes()
        assert data == reference_bytes(tr, half, volume(True))
        info = N.bake_file_info(path)
        assert info["format"] == 1 and info["adaptive"] == 0 and info["m2_offset"] == 0 and info["samples"] == SAMPLES
        assert info["checksum_offset"] - info["table_offset"] in range(2 * info["stored_entries"], 2 * info["stored_entries"] + 8)
        with tracer(small=True) as other, other.load_bake(path) as loaded:
            a, _ = accessors(half)
            b, ms = accessors(loaded)
            same(a, b)
            assert all(v == 0 for v in ms.values())
            for x, y in zip(lookups(other, loaded), lookups(tr, half)):
                assert np.array_equal(bits(x), bits(y))
            for x, y in zip(frames(other, loaded), frames(tr, half)):
                assert np.array_equal(bits(x), bits(y)) and y.any()
            loaded.save(tmp_path / "again.bake")
            assert (tmp_path / "again.bake").read_bytes() == data
            assert _code(loaded.trace_more, 1) == _lib.CT_E_INVAL and _code(loaded.half) == _lib.CT_E_INVAL


@pytest.mark.gpu
def test_the_armed_invariants_and_the_allocations(monkeypatch):
    start = ct.debug_allocations()
    monkeypatch.setenv("CT_DEBUG_INVARIANTS", "1")
    with tracer(small=True) as tr:
        monkeypatch.delenv("CT_DEBUG_INVARIANTS")
        with make(tr, "traced", "compact") as src:
            held = ct.debug_allocations()
            with src.half() as half:
                # the half table, and copies of the node bytes, the list, the slots and the probe and direction tables
                assert ct.debug_allocations()["device_buffers"] == held["device_buffers"] + 6
                tr.baked_render_accumulate(half, 1, 2, rgb_scale=SCALE, direct=True)
                tr.render_accumulate(3, 2)
                iv = tr.debug_invariants()
                inside = ct.debug_allocations()
            assert ct.debug_allocations()["device_buffers"] == inside["device_buffers"] - 6
        assert iv["checks"] > 0 and iv["violations"] == 0
    assert ct.debug_allocations() == start


@pytest.mark.gpu
def test_cli_renders_from_the_half_copy_and_saves_it(tmp_path):
    from deepestscatter_amd import exr
    from test_bake_file import cli_common
    common, file, image = cli_common(tmp_path), tmp_path / "half.bake", tmp_path / "procedural_32.Back.PT.exr"
    r = subprocess.run(common + ["--traced-bake", "5,4,3,4,3", "--bake-samples", "4", "--net-bake-sparse", "--bake-half", "--bake-out", str(file)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = exr.read_exr(image)
    with ds.CloudTracer(ds.make_procedural_cloud(32), width=W, height=H, light_direction=ds.LIGHT_DIRECTIONS["Back"]) as tr, \
            tr.traced_bake((5, 4, 3), 4, 3, 4, sparse=True) as src, src.half() as half:
        tr.baked_render_accumulate(half, 1, 4, rgb_scale=SCALE, direct=True)
        want = tr.mean()[..., :3]
        tr.reset()
        tr.baked_render_accumulate(src, 1, 4, rgb_scale=SCALE, direct=True)
        assert np.array_equal(bits(got), bits(want)) and want.any() and not np.array_equal(bits(want), bits(tr.mean()[..., :3]))
        half.save(tmp_path / "python.bake")
    assert file.read_bytes() == (tmp_path / "python.bake").read_bytes() and N.bake_file_info(file)["format"] == 1
    first = image.read_bytes()
    image.unlink()
    r = subprocess.run(common + ["--bake-in", str(file)], capture_output=True, text=True, timeout=300)      # a half file renders as it is
    assert r.returncode == 0 and image.read_bytes() == first, r.stdout[-2000:] + r.stderr[-2000:]
