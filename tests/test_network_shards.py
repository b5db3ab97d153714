"""ct_network_render_shard_subframe / ct_network_render_shard_accumulate, ct_shard_tiles and ct_group_network_*: the scattering
network as a renderer on sharded handles and on a CtGroup (include/cloudtrace.h).

Everything is compared BIT FOR BIT (np.array_equal on the uint32 view of the float32 arrays): the reference of a shard's pixels
is the unsharded renderer that already exists -- ct_network_render_subframe / ct_network_render_accumulate on a shard_count == 1
handle of the same scene -- and the reference of the fused accumulation is the loop shard_subframe + accumulate.  No tolerance
of this file's own.

Scene: that of tests/test_network_direct.py -- make_procedural_cloud(64), the default pose, SCALE = (0.5, 2.0, 3.0), the seeded
(32, 1, 1) weights (helpers copied, not imported) -- on two frames: 24 x 16 (3 x 2 whole tiles, records in every tile) and
27 x 13 (4 x 2 tiles, the last column 3 pixels wide and the upper row 5 pixels high, so clipped tiles exist; the records lie
in the two middle tile columns).  On 27 x 13 with four shards, shard 3 owns tiles (3, 0) and (0, 1), where no primary ray
scatters: a shard that owns tiles and has no record at all.  The GPU tests assert these premises on the device's own record
list (descriptor_frame) before they rely on them."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import deepestscatter_amd as ds
from deepestscatter_amd import _lib
from deepestscatter_amd import network as N

FRAMES = [(24, 16), (27, 13)]
SID, SPP = 3, 3
SCALE = (0.5, 2.0, 3.0)
LIGHT2 = (0.586, -0.766, -0.271)
SMALL = N.NetworkShape(32, 1, 1)


# ------------------------------------------------------------------------------ helpers of tests/test_network_render.py
def seeded_weights(shape: N.NetworkShape, seed: int) -> np.ndarray:
    """Every matrix and bias uniform in +-1/sqrt(fan_in), in the flat array's order."""
    rng = np.random.default_rng(seed)
    dims = []
    for k in range(N.BLOCKS):
        dims += [(shape.width, shape.fan_in(k)), (shape.width, shape.width)]
    dims += [(shape.width, shape.width)] * (shape.head_layers - 1) + [(1, shape.width)]
    parts = []
    for rows, cols in dims:
        bound = 1.0 / np.sqrt(cols)
        parts.append(rng.uniform(-bound, bound, rows * cols).astype(np.float32))
        parts.append(rng.uniform(-bound, bound, rows).astype(np.float32))
    flat = np.concatenate(parts)
    assert flat.size == shape.weight_count()
    return flat


def weights():
    """The (32, 1, 1) case of tests/test_network_render.py: seed 13, outputs of both signs on this scene's records."""
    return seeded_weights(SMALL, 13)


def cloud():
    return ds.make_procedural_cloud(64)


def small_net(tr):
    return N.Network(tr, weights(), 32, 1, 1)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def _code(fn, *a, **kw):
    with pytest.raises(_lib.CloudTraceError) as e:
        fn(*a, **kw)
    return e.value.code


# ---------------------------------------------------------------------------------------------------- CPU
def test_symbols_resolve_and_answer_null_arguments(product_lib):
    names = ["ct_network_render_shard_subframe", "ct_network_render_shard_accumulate", "ct_debug_network_scratch", "ct_shard_tiles",
             "ct_group_network_create", "ct_group_network_destroy", "ct_group_network_render_accumulate"]
    for name in names:
        assert hasattr(product_lib, name) and name in _lib.EXPORTS
    p = _lib.CtNetworkRender(_lib.CT_ABI_VERSION, _lib.CT_NET_OUT_LINEAR, (C.c_float * 3)(1, 1, 1), 0)
    assert product_lib.ct_network_render_shard_subframe(None, None, C.byref(p), 1, None) == _lib.CT_E_INVAL
    assert product_lib.ct_network_render_shard_subframe(None, None, None, 1, None) == _lib.CT_E_INVAL
    assert product_lib.ct_network_render_shard_accumulate(None, None, C.byref(p), 1, 1) == _lib.CT_E_INVAL
    assert product_lib.ct_debug_network_scratch(None, None) == _lib.CT_E_INVAL
    out = C.c_void_p()
    assert product_lib.ct_group_network_create(None, None, C.byref(out)) == _lib.CT_E_INVAL
    assert product_lib.ct_group_network_render_accumulate(None, None, C.byref(p), 1, 1) == _lib.CT_E_INVAL
    assert product_lib.ct_group_network_destroy(None) == _lib.CT_OK


@pytest.mark.parametrize("size", [(24, 16), (27, 13), (1, 1)])
@pytest.mark.parametrize("count", [1, 2, 3, 7])
def test_shard_tiles_against_shard_mask(product_lib, size, count):
    w, h = size
    tiles_x, tiles_y = (w + 7) // 8, (h + 7) // 8
    seen = []
    for index in range(count):
        tiles = ds.shard_tiles(w, h, index, count)
        assert tiles.dtype == np.uint32
        assert (np.diff(tiles.astype(np.int64)) > 0).all()                        # ascending, none twice
        assert (tiles < tiles_x * tiles_y).all()
        for t in tiles:
            assert ds.tile_owner(int(t) % tiles_x, int(t) // tiles_x, count) == index
        mask = np.zeros((h, w), bool)
        for t in tiles:
            tx, ty = int(t) % tiles_x, int(t) // tiles_x
            mask[8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8] = True                     # (numpy clips the slices like the frame clips the tile)
        assert np.array_equal(mask, ds.shard_mask(w, h, index, count))
        seen += tiles.tolist()
        # the count query, an exact capacity, and one that is too small
        n = C.c_uint32(99)
        assert product_lib.ct_shard_tiles(w, h, index, count, None, 0, C.byref(n)) == _lib.CT_OK and n.value == len(tiles)
        if len(tiles):
            buf = np.full(len(tiles), 0xFFFFFFFF, np.uint32)
            n = C.c_uint32(99)
            rc = product_lib.ct_shard_tiles(w, h, index, count, buf.ctypes.data_as(C.c_void_p), len(tiles) - 1, C.byref(n))
            assert rc == _lib.CT_E_INVAL and n.value == len(tiles)
            assert np.array_equal(buf[:-1], tiles[:-1]) and buf[-1] == 0xFFFFFFFF      # nothing written past the capacity
    assert sorted(seen) == list(range(tiles_x * tiles_y))                         # every tile once over the shards


def test_shard_tiles_refuses_what_is_no_shard(product_lib):
    n = C.c_uint32(0)
    for w, h, index, count in ((0, 8, 0, 1), (8, 0, 0, 1), (8, 8, 0, 0), (8, 8, 1, 1), (8, 8, 3, 2)):
        assert product_lib.ct_shard_tiles(w, h, index, count, None, 0, C.byref(n)) == _lib.CT_E_INVAL
    assert product_lib.ct_shard_tiles(8, 8, 0, 1, None, 0, None) == _lib.CT_E_INVAL
    with pytest.raises(_lib.CloudTraceError):
        ds.shard_tiles(8, 8, 2, 2)


# ---------------------------------------------------------------------------------------------------- GPU
# The unsharded renderer on every configuration the tests below compare against, computed once and never changed:
# key -> dict(frame=..., mean=..., m2=..., pixels={sid: record pixel indices}).
_REFERENCE = {}


def reference(w, h, direct=False, transform="linear", **kw):
    key = (w, h, direct, transform, tuple(sorted(kw.items())))
    if key not in _REFERENCE:
        with ds.CloudTracer(cloud(), width=w, height=h, **kw) as tr, small_net(tr) as net:
            frame = tr.network_render_subframe(net, SID, transform=transform, rgb_scale=SCALE, direct=direct).cpu().numpy()
            tr.network_render_accumulate(net, 1, SPP, transform=transform, rgb_scale=SCALE, direct=direct)
            pixels = {sid: tr.descriptor_frame(sid)[3].cpu().numpy().astype(np.int64) for sid in range(1, SPP + 1)}
            _REFERENCE[key] = dict(frame=frame, mean=tr.mean(), m2=tr.m2(), pixels=pixels)
        for a in ("frame", "mean", "m2"):
            _REFERENCE[key][a].setflags(write=False)
        # a frame test is blind on a black picture
        assert _REFERENCE[key]["frame"][..., :3].any() and _REFERENCE[key]["mean"][..., :3].any() and _REFERENCE[key]["m2"][..., :3].any()
    return _REFERENCE[key]


CASES = {
    "linear": dict(),
    "expm1": dict(transform="expm1"),
    "direct": dict(direct=True),
    "direct-expm1": dict(direct=True, transform="expm1"),
    "fixed8-direct": dict(direct=True, flags=_lib.CT_FLAG_TEX_FIXED8),
    "delta": dict(estimator=_lib.CT_EST_DELTA),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_on_an_unsharded_handle_the_shard_entry_points_equal_the_existing_ones(case):
    kw = dict(CASES[case])
    call = dict(transform=kw.pop("transform", "linear"), direct=kw.pop("direct", False))
    for w, h in FRAMES:
        want = reference(w, h, **call, **kw)
        with ds.CloudTracer(cloud(), width=w, height=h, **kw) as tr, small_net(tr) as net:
            got = tr.network_render_shard_subframe(net, SID, rgb_scale=SCALE, **call).cpu().numpy()
            assert same(got, want["frame"]) and same(tr.frame(), want["frame"]), (case, w, h)
            assert tr.subframes == 0 and not tr.mean().any()
            tr.network_render_shard_accumulate(net, 1, SPP, rgb_scale=SCALE, **call)
            assert tr.subframes == SPP
            assert same(tr.mean(), want["mean"]) and same(tr.m2(), want["m2"]), (case, w, h)


def tiles_with_records(w, pixels):
    """-> the set of tiles (ty * tiles_x + tx) that hold one of the record pixels (y * w + x)."""
    tiles_x = (w + 7) // 8
    return set(((pixels // w) // 8 * tiles_x + (pixels % w) // 8).tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("size", FRAMES, ids=["24x16", "27x13"])
@pytest.mark.parametrize("count", [2, 3, 4])
def test_every_shard_renders_its_own_tiles_and_nothing_else(count, size):
    w, h = size
    plain, lit = reference(w, h), reference(w, h, direct=True)
    # the premises: some shard has records in two tiles or more; on 27 x 13 with four shards, shard 3 owns tiles and has no
    # record in any of the subframes
    record_tiles = [tiles_with_records(w, plain["pixels"][sid]) for sid in range(1, SPP + 1)]
    own = [set(ds.shard_tiles(w, h, i, count).tolist()) for i in range(count)]
    assert all(own), "a shard without a tile is not what this test is about"
    assert any(len(own[i] & record_tiles[SID - 1]) >= 2 for i in range(count))
    if (w, h, count) == (27, 13, 4):
        assert len(own[3]) == 2 and not any(own[3] & t for t in record_tiles)
    sums = {False: [np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)],
            True: [np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)]}
    for index in range(count):
        mask = ds.shard_mask(w, h, index, count)
        with ds.CloudTracer(cloud(), width=w, height=h, shard_index=index, shard_count=count) as tr, small_net(tr) as net:
            for direct, want in ((False, plain), (True, lit)):
                got = tr.network_render_shard_subframe(net, SID, rgb_scale=SCALE, direct=direct).cpu().numpy()
                assert same(got[mask], want["frame"][mask]), (index, direct)
                assert not bits(got[~mask]).any(), (index, direct)              # foreign pixels: (0, 0, 0, 0)
                assert same(tr.frame(), got)
                tr.network_render_shard_accumulate(net, 1, SPP, rgb_scale=SCALE, direct=direct)
                mean, m2 = tr.mean(), tr.m2()
                assert same(mean[mask], want["mean"][mask]) and same(m2[mask], want["m2"][mask]), (index, direct)
                assert not bits(mean[~mask]).any() and not bits(m2[~mask]).any(), (index, direct)
                sums[direct][0] += mean
                sums[direct][1] += m2
                tr.reset()
    for direct, want in ((False, plain), (True, lit)):
        assert same(sums[direct][0], want["mean"]) and same(sums[direct][1], want["m2"]), direct


@pytest.mark.gpu
def test_fused_equals_the_loop_on_a_shard():
    w, h = 27, 13
    for index, count in ((1, 3), (3, 4)):                      # (3 of 4: the shard without a record)
        states = []
        for fused in (True, False):
            with ds.CloudTracer(cloud(), width=w, height=h, shard_index=index, shard_count=count) as tr, small_net(tr) as net:
                if fused:
                    tr.network_render_shard_accumulate(net, 1, SPP, rgb_scale=SCALE, direct=True, band_pixels=128)
                else:
                    for sid in range(1, SPP + 1):
                        tr.network_render_shard_subframe(net, sid, rgb_scale=SCALE, direct=True, band_pixels=128, out=False)
                        tr.accumulate(sid)
                states.append((tr.mean(), tr.m2(), tr.subframes))
        (a, b) = states
        assert same(a[0], b[0]) and same(a[1], b[1]) and a[2] == b[2] == SPP
        assert a[0][..., 3].any()


@pytest.mark.gpu
@pytest.mark.parametrize("shards", [(0, 1), (0, 2)], ids=["unsharded", "shard-0-of-2"])
def test_the_image_does_not_depend_on_the_band(shards):
    """A band is max(1, band_pixels / 64) tiles: 1, 64 and 100 give one tile per band, 128 two, 192 three (the 8 tiles of the
    unsharded 27 x 13 frame make bands of 3, 3, 2), 2^20 and 0 the whole list at once."""
    w, h = 27, 13
    index, count = shards
    want = reference(w, h, direct=True)
    mask = ds.shard_mask(w, h, index, count)
    with ds.CloudTracer(cloud(), width=w, height=h, shard_index=index, shard_count=count) as tr, small_net(tr) as net:
        first = None
        for band in (1, 64, 100, 1 << 20, 0, 128, 192):
            frame = tr.network_render_shard_subframe(net, SID, rgb_scale=SCALE, direct=True, band_pixels=band).cpu().numpy()
            tr.network_render_shard_accumulate(net, 1, SPP, rgb_scale=SCALE, direct=True, band_pixels=band)
            got = (frame, tr.mean(), tr.m2())
            tr.reset()
            if first is None:
                first = got
                assert same(frame[mask], want["frame"][mask]) and same(got[1][mask], want["mean"][mask]) and same(got[2][mask], want["m2"][mask])
                assert not bits(frame[~mask]).any() and not bits(got[1][~mask]).any()
            assert all(same(x, y) for x, y in zip(got, first)), band


def _state(tr):
    return tr.mean(), tr.m2(), tr.subframes, tr.counters(), tr.fetch_counters()


@pytest.mark.gpu
def test_shard_subframe_has_no_side_effects_and_a_warm_call_allocates_nothing():
    w, h = 27, 13
    states = []
    for with_call in (True, False):
        with ds.CloudTracer(cloud(), width=w, height=h, shard_index=0, shard_count=2) as tr:
            tr.render_accumulate(1, 2)
            if with_call:
                before = _state(tr)
                with small_net(tr) as net:
                    assert not any(tr.network_scratch().values())
                    frame = tr.network_render_shard_subframe(net, SID, rgb_scale=SCALE, direct=True, band_pixels=128)
                    assert bool((frame[..., :3] != 0).any())
                    cold = tr.network_scratch()
                    assert all(cold[k] for k in ("found", "waves", "pos", "dir", "aux", "out", "desc", "direct", "tiles"))
                    assert cold["band_cap"] >= 128 and cold["direct_cap"] >= 128 and cold["desc_cap"] >= 1
                    # warm calls: the same band, a smaller one, the other entry point's first (it needs no more than was reserved)
                    tr.network_render_shard_subframe(net, SID, rgb_scale=SCALE, direct=True, band_pixels=128, out=False)
                    assert tr.network_scratch() == cold
                    tr.network_render_shard_subframe(net, SID, rgb_scale=SCALE, direct=True, band_pixels=64, out=False)
                    assert tr.network_scratch() == cold
                    times = tr.network_render_time()
                    assert len(times) == 4 and all(np.isfinite(t) and t >= 0 for t in times) and times[0] > 0 and times[2] > 0
                after = _state(tr)
                assert same(before[0], after[0]) and same(before[1], after[1]) and before[2:] == after[2:] and after[2] == 2
            tr.render_accumulate(3, 2)                      # the path tracer goes on as on a handle that never saw the network
            states.append(_state(tr))
    x, y = states
    assert same(x[0], y[0]) and same(x[1], y[1]) and x[0].any()
    assert x[2:] == y[2:] and x[2] == 4


@pytest.mark.gpu
def test_errors_leave_the_shard_usable():
    w, h = 27, 13
    want = reference(w, h)
    mask = ds.shard_mask(w, h, 1, 2)
    with ds.CloudTracer(cloud(), width=w, height=h, shard_index=1, shard_count=2) as tr, small_net(tr) as net:
        L, hnd = tr.L, tr.h

        def still_renders():
            got = tr.network_render_shard_subframe(net, SID, rgb_scale=SCALE).cpu().numpy()
            assert same(got[mask], want["frame"][mask]) and not bits(got[~mask]).any()
            assert tr.subframes == 0 and not tr.mean().any()

        still_renders()
        p = _lib.CtNetworkRender(_lib.CT_ABI_VERSION, 0, (C.c_float * 3)(1, 1, 1), 0)
        assert L.ct_network_render_shard_subframe(hnd, None, C.byref(p), SID, None) == _lib.CT_E_INVAL
        assert L.ct_network_render_shard_subframe(hnd, net.n, None, SID, None) == _lib.CT_E_INVAL
        assert L.ct_network_render_shard_accumulate(hnd, None, C.byref(p), 1, 1) == _lib.CT_E_INVAL
        assert L.ct_network_render_shard_accumulate(hnd, net.n, None, 1, 1) == _lib.CT_E_INVAL
        assert L.ct_network_render_shard_subframe(None, net.n, C.byref(p), SID, None) == _lib.CT_E_INVAL
        assert L.ct_network_render_shard_accumulate(None, net.n, C.byref(p), 1, 1) == _lib.CT_E_INVAL
        still_renders()
        for shape in (N.NetworkShape(32, 0, 1), N.NetworkShape(16, 2, 1)):                       # aux 0, aux 2
            with N.Network(tr, seeded_weights(shape, 2), shape.width, shape.aux, shape.head_layers) as other:
                assert _code(tr.network_render_shard_subframe, other, SID) == _lib.CT_E_INVAL
                assert b"aux" in L.ct_last_error(hnd)
                assert _code(tr.network_render_shard_accumulate, other, 1, 1) == _lib.CT_E_INVAL
            still_renders()
        for bad in (dict(transform=2), dict(rgb_scale=(1, np.nan, 1))):
            assert _code(tr.network_render_shard_subframe, net, SID, **bad) == _lib.CT_E_INVAL, bad
            assert _code(tr.network_render_shard_accumulate, net, 1, 1, **bad) == _lib.CT_E_INVAL, bad
        assert _code(tr.network_render_shard_subframe, net, 0) == _lib.CT_E_INVAL                # ids are 1-based
        assert _code(tr.network_render_shard_accumulate, net, 0, 1) == _lib.CT_E_INVAL
        assert _code(tr.network_render_shard_accumulate, net, 1, 0) == _lib.CT_E_INVAL           # count == 0
        assert _code(tr.network_render_shard_accumulate, net, 2, 1) == _lib.CT_E_STATE           # first != subframes + 1
        assert b"subframes are accumulated" in L.ct_last_error(hnd)
        still_renders()
        # the unsharded entry points keep refusing a shard, and say where to go
        assert _code(tr.network_render_subframe, net, SID) == _lib.CT_E_INVAL
        assert b"shard" in L.ct_last_error(hnd)
        assert _code(tr.network_render_accumulate, net, 1, 1) == _lib.CT_E_INVAL
        still_renders()
        tr.network_render_shard_accumulate(net, 1, 2, rgb_scale=SCALE)
        assert tr.subframes == 2
        assert _code(tr.network_render_shard_accumulate, net, 2, 1) == _lib.CT_E_STATE
        assert _code(tr.network_render_shard_accumulate, net, 4, 1) == _lib.CT_E_STATE
        tr.network_render_shard_accumulate(net, 3, 1, rgb_scale=SCALE)
        assert tr.subframes == 3 and same(tr.mean()[mask], want["mean"][mask]) and same(tr.m2()[mask], want["m2"][mask])


@pytest.mark.gpu
@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]], ids=["0,0", "0,0,0"])
def test_group_renders_what_one_handle_renders(devices):
    w, h = 27, 13
    call = dict(rgb_scale=SCALE, direct=True)
    with ds.CloudTracer(cloud(), width=w, height=h) as tr, small_net(tr) as net:
        tr.network_render_accumulate(net, 1, SPP, **call)
        first = (tr.mean(), tr.m2(), tr.tonemap(0.4), tr.is_converged())
        tr.network_render_accumulate(net, SPP + 1, 2, **call)
        second = (tr.mean(), tr.m2(), tr.subframes)
        tr.set_light(LIGHT2)
        tr.reset()
        tr.network_render_accumulate(net, 1, 2, **call)
        relit = (tr.mean(), tr.m2())
    assert same(first[0], reference(w, h, direct=True)["mean"]) and not same(relit[0], first[0])
    with ds.TracerGroup(cloud(), devices, width=w, height=h) as g:
        gn = g.network(weights(), 32, 1, 1)
        g.network_render_accumulate(gn, 1, SPP, **call)
        assert same(g.mean(), first[0]) and same(g.m2(), first[1])
        screen, avg = g.tonemap(0.4)
        assert np.array_equal(screen, first[2][0]) and avg == first[2][1] and screen[..., :3].any()
        assert g.is_converged() == first[3]
        g.network_render_accumulate(gn, SPP + 1, 2, **call)                   # a second call continues at subframe 4
        assert same(g.mean(), second[0]) and same(g.m2(), second[1]) and second[2] == SPP + 2
        with pytest.raises(_lib.CloudTraceError) as e:                       # every shard refuses a gap; the first one's message
            g.network_render_accumulate(gn, SPP + 4, 1, **call)
        assert e.value.code == _lib.CT_E_STATE and "shard 0" in e.value.message
        g.set_light(LIGHT2)
        g.reset()
        g.network_render_accumulate(gn, 1, 2, **call)
        assert same(g.mean(), relit[0]) and same(g.m2(), relit[1])
        # a network of another group, and none
        with ds.TracerGroup(cloud(), [0], width=w, height=h) as other:
            foreign = other.network(weights(), 32, 1, 1)
            with pytest.raises(_lib.CloudTraceError) as e:
                g.network_render_accumulate(foreign, 3, 1, **call)
            assert e.value.code == _lib.CT_E_INVAL
            foreign.close()
        with pytest.raises(_lib.CloudTraceError) as e:
            g.network_render_accumulate(None, 3, 1, **call)
        assert e.value.code == _lib.CT_E_INVAL
        with g.network(seeded_weights(N.NetworkShape(32, 0, 1), 2), 32, 0, 1) as no_aux:
            with pytest.raises(_lib.CloudTraceError) as e:                   # a network with no aux input: the first shard says so
                g.network_render_accumulate(no_aux, 3, 1, **call)
            assert e.value.code == _lib.CT_E_INVAL and "aux" in e.value.message and "shard 0" in e.value.message
        g.network_render_accumulate(gn, 3, 1, **call)                         # the group is usable after each
        gn.close()


@pytest.mark.gpu
def test_cli_renders_the_network_on_a_group(tmp_path):
    """cloudtrace --network F --gpus 0,0 writes the files cloudtrace --network F writes, byte for byte, for both of the job's
    suns (the second through ct_group_set_light)."""
    from deepestscatter_amd import build
    cli = build.build_cli()
    N.save_weights(tmp_path / "w.bin", weights(), SMALL)
    written = []
    for extra in ([], ["--gpus", "0,0"]):
        out = tmp_path / ("g" if extra else "s")
        out.mkdir()
        r = subprocess.run([str(cli), "procedural:64", "--network", str(tmp_path / "w.bin"), "--size", "27x13", "--spp", "3", "--net-scale", "0.5,2,3",
                            "--net-transform", "expm1", "--net-direct", "--out", str(out), *extra], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "rendering subframe 3" in r.stdout
        written.append({light: (out / f"procedural_64.{light}.PT.exr").read_bytes() for light in ("Side", "Back")})
    assert written[0] == written[1]
    assert written[0]["Side"] != written[0]["Back"] and len(written[0]["Side"]) > 27 * 13 * 3
