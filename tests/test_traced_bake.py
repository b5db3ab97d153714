"""ct_bake_traced: the probe table filled with path-traced radiance (include/cloudtrace.h, "the traced bake").

An entry of a traced bake is the float32 mean of S experiments of ct_point_radiance_launch's estimator, so everything here is held
to that entry point, to the oracle, or to another bake, bit for bit: every comparison is np.array_equal on the bits.

Scene: that of tests/test_network_render.py -- make_procedural_cloud(64), 24 x 16, the default pose.  GRID is the grid of
tests/test_network_bake_compact.py: 504 nodes, 314 of them active on cloud() (network.bake_mask_reference), 12 096 entries.
Four experiments per entry unless a test says otherwise."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import _oracle as O
import deepestscatter_amd as ds
from deepestscatter_amd import _lib
from deepestscatter_amd import network as N
from test_network_render import H, LIGHT2, SCALE, SID, SMALL, W, cloud, weights

GRID = ((9, 8, 7), 8, 3)
ENTRIES = 9 * 8 * 7 * 8 * 3
SAMPLES = 4
STEP = ds.SceneParams().sample_step
MARCH, DELTA = 0, 1
f32 = np.float32

_MASKS = {}


def reference_nodes(grid):
    """The reference mask's node bytes of cloud() at the default step, computed once per grid and left unchanged."""
    if grid not in _MASKS:
        _MASKS[grid] = N.bake_mask_reference(cloud(), grid, STEP)[1]
        _MASKS[grid].setflags(write=False)
    return _MASKS[grid]


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _code(fn, *a, **kw):
    with pytest.raises(_lib.CloudTraceError) as e:
        fn(*a, **kw)
    return e.value.code


# ---------------------------------------------------------------------------------------------------- CPU
def test_symbols_resolve_and_answer_null_arguments(product_lib):
    L = product_lib
    for name in ("ct_bake_traced", "ct_bake_trace_more", "ct_bake_retrace", "ct_bake_trace_info", "ct_bake_directions"):
        assert hasattr(L, name) and name in _lib.EXPORTS
    d = _lib.CtBakeDesc(_lib.CT_ABI_VERSION, (C.c_uint32 * 3)(2, 2, 2), 4, 2)
    out = C.c_void_p()
    assert L.ct_bake_traced(None, C.byref(d), _lib.CT_BAKE_DENSE, 1, C.byref(out)) == _lib.CT_E_INVAL
    assert L.ct_bake_traced(None, None, 0, 0, None) == _lib.CT_E_INVAL
    assert L.ct_bake_trace_more(None, None, 1) == _lib.CT_E_INVAL
    assert L.ct_bake_retrace(None, None, 1) == _lib.CT_E_INVAL
    assert L.ct_bake_trace_info(None, None) == _lib.CT_E_INVAL
    assert L.ct_bake_directions(None, None, 0) == _lib.CT_E_INVAL
    assert (_lib.CT_BAKE_DENSE, _lib.CT_BAKE_SPARSE, _lib.CT_BAKE_COMPACT) == (0, 1, 2)
    T = _lib.CtBakeTraceInfo
    assert [C.sizeof(T), T.samples.offset, T.paths.offset, T.trace_ms.offset] == [32, 4, 8, 16]


def test_struct_layout_matches_the_header():
    import tempfile
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "cloudtrace.h"\nint main(){printf("%zu %zu %zu %zu %d %d %d", '
           'sizeof(CtBakeTraceInfo), offsetof(CtBakeTraceInfo, samples), offsetof(CtBakeTraceInfo, paths), '
           'offsetof(CtBakeTraceInfo, trace_ms), CT_BAKE_DENSE, CT_BAKE_SPARSE, CT_BAKE_COMPACT);return 0;}')
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "p.c").write_text(src)
        subprocess.run(["gcc", "-I", str(root / "include"), "-o", f"{d}/p", f"{d}/p.c"], check=True)
        out = subprocess.run([f"{d}/p"], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [32, 4, 8, 16, 0, 1, 2]


def hand_made_frame(nphi, nc):
    """A frame that is not axis-aligned, as bake_frame makes it in double, and the u_j of the header's formula -> (info, u)."""
    l = np.array([-0.03, -0.25, 0.8])
    l /= np.linalg.norm(l)
    a = np.cross(l, [1.0, 0.0, 0.0])
    a /= np.linalg.norm(a)
    b = np.cross(l, a)
    info = {"light": l.astype(f32), "axis_a": a.astype(f32), "axis_b": b.astype(f32), "azimuths": nphi, "cosines": nc,
            "cosine": np.array([-1.0 + 2.0 * k / (nc - 1) for k in range(nc)], f32)}
    u = np.empty((nphi, 3))
    for j in range(nphi):
        t = j / (nphi // 4)
        p = 1.0 - t if t <= 2.0 else t - 3.0
        q = 1.0 - abs(p) if t <= 2.0 else -(1.0 - abs(p))
        v = p * info["axis_a"].astype(np.float64) + q * info["axis_b"].astype(np.float64)
        u[j] = v / np.linalg.norm(v)
    return info, u.astype(f32)


@pytest.mark.parametrize("nphi", [4, 8, 64])
@pytest.mark.parametrize("nc", [2, 3, 64])
def test_reference_directions_are_unit_vectors_on_the_lookups_nodes(nphi, nc):
    info, u = hand_made_frame(nphi, nc)
    d = N.bake_directions_reference(info, u)
    assert d.shape == (nphi, nc, 3) and d.dtype == f32
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=2) - 1.0).max() <= 1e-6
    for j in range(nphi):                                                 # c = -1 and c = 1: -l and l, whatever the azimuth
        assert np.array_equal(bits(d[j, 0]), bits(-info["light"])) and np.array_equal(bits(d[j, nc - 1]), bits(info["light"]))
    # the lookup's split (network.bake_lookup_reference: bake_azimuth and the fc formula) puts d(j, k) on node (j, k)
    flat, l = d.reshape(-1, 3), info["light"]
    c = ((flat[:, 0] * l[0] + flat[:, 1] * l[1]).astype(f32) + flat[:, 2] * l[2]).astype(f32)
    fc = ((c + f32(1.0)).astype(f32) * f32(f32(0.5) * f32(nc - 1))).astype(f32)
    ft = (N.bake_azimuth(flat, info["axis_a"], info["axis_b"]) * f32(f32(nphi) * f32(0.25))).astype(f32)
    jj, kk = np.divmod(np.arange(nphi * nc), nc)
    assert np.array_equal(np.rint(fc).astype(np.int64), kk)
    inner = (kk != 0) & (kk != nc - 1)                                    # (along the light there is no azimuth)
    assert np.array_equal(np.rint(ft).astype(np.int64)[inner] % nphi, jj[inner])


def test_point_fold_reference_is_a_literal_loop_of_add_experiment_result():
    rng = np.random.default_rng(5)
    values = (rng.random((9, 7), dtype=f32) * f32(40)).astype(f32)
    want = np.zeros(7, f32)
    for i in range(7):
        radiance, count = f32(0), 0
        for x in values[:, i]:
            count += 1
            new_weight = f32(1.0 / float(f32(count)))
            radiance = f32(radiance + f32(f32(x - radiance) * new_weight))
        want[i] = radiance
    got = N.point_fold_reference(values)
    assert got.dtype == f32 and np.array_equal(bits(got), bits(want))
    # continued from a state: 4 + 5 experiments are the 9
    again = N.point_fold_reference(values[4:], mean=N.point_fold_reference(values[:4]), count=4)
    assert np.array_equal(bits(again), bits(want))
    assert N.point_fold_reference(np.array([[1.0], [2.0], [6.0]], f32))[0] == f32(3.0)


def test_python_refuses_contradicting_arguments():
    with pytest.raises(ValueError):
        N.Bake(None, None, (2, 2, 2), 4, 2, sparse=True, compact=True, samples=4)
    with pytest.raises(ValueError):
        ds.CloudTracer.traced_bake(None, (2, 2, 2), 4, 2, 4, sparse=True, compact=True)
    with pytest.raises(ValueError):
        N.Bake(None, object(), (2, 2, 2), 4, 2, samples=4)                # a network and samples
    with pytest.raises(ValueError):
        N.Bake(None, None, (2, 2, 2), 4, 2)                               # neither


# ---------------------------------------------------------------------------------------------------- GPU
def tracer(**kw):
    return ds.CloudTracer(cloud(), width=W, height=H, **kw)


def entry_tasks(bake, entries=None):
    """The point tasks of the definition for virtual entries `entries` (default: all): the probe's position, d(j, k)."""
    info = bake.info
    nphi, nc = info["azimuths"], info["cosines"]
    e = np.arange(info["entries"], dtype=np.int64) if entries is None else np.asarray(entries, np.int64)
    pos = bake.probes()[0]
    d = bake.directions()
    return pos[e // nc], d[(e // nc) % nphi, e % nc]


@pytest.fixture(scope="module")
def scene():
    """A mode-0 MARCH tracer with the dense, sparse and compact traced bakes of GRID, and a mode-1 tracer for the public estimator.
    No test changes their light or accumulates on them."""
    with tracer() as tr, tracer(mode=1) as point:
        made = []
        try:
            s = {"tr": tr, "point": point}
            for key, kw in (("dense", {}), ("sparse", {"sparse": True}), ("compact", {"compact": True})):
                s[key] = tr.traced_bake(*GRID, SAMPLES, **kw)
                made.append(s[key])
            yield s
        finally:
            for obj in reversed(made):
                obj.close()


@pytest.mark.gpu
@pytest.mark.parametrize("estimator, flags", [(MARCH, 0), (DELTA, 0), (MARCH, _lib.CT_FLAG_TEX_FIXED8)], ids=["march", "delta", "march-fixed8"])
def test_every_entry_is_the_public_estimators_mean(scene, estimator, flags):
    """All 12 096 entries against ct_point_radiance_launch on a mode-1 handle: task e = (probe position, d(j, k)), frames 1 .. 4."""
    def check(tr, point, bake):
        pos, d = entry_tasks(bake)
        assert len(pos) == ENTRIES
        want = point.point_radiance_launch(ds.make_point_tasks(pos, d), 1, SAMPLES)["radiance"]
        got = bake.table().reshape(-1)
        assert np.array_equal(bits(got), bits(want)) and want.any() and np.isfinite(want).all()
        ti = bake.trace_info()
        assert ti["traced"] and ti["samples"] == SAMPLES and ti["paths"] == ENTRIES * SAMPLES and ti["trace_ms"] > 0 and ti["fold_ms"] > 0
        info = bake.info
        assert info["gather_ms"] == 0 and info["network_ms"] == 0 and info["current"]
        assert np.array_equal(bits(bake.directions()), bits(N.bake_directions_reference(info, bake.probes(0, info["azimuths"])[1])))
        return got

    if (estimator, flags) == (MARCH, 0):
        check(scene["tr"], scene["point"], scene["dense"])
        return
    with tracer(estimator=estimator, flags=flags) as tr, tracer(mode=1, estimator=estimator, flags=flags) as point, \
            tr.traced_bake(*GRID, SAMPLES) as bake:
        got = check(tr, point, bake)
        assert not np.array_equal(bits(got), bits(scene["dense"].table().reshape(-1)))


@pytest.mark.gpu
def test_entries_equal_the_oracles_paths_folded(scene):
    """48 entries of active nodes, spread over the list: the oracle's mode-1 path for (launch e, frame f), f = 1 .. 4, folded."""
    bake = scene["dense"]
    active = np.flatnonzero(reference_nodes(GRID[0]).reshape(-1))
    assert len(active) == 314
    block = GRID[1] * GRID[2]
    nodes = active[np.linspace(0, len(active) - 1, 48).astype(np.int64)]
    entries = nodes * block + (np.arange(48) * 5) % block                 # every (j, k) of the block occurs
    assert len(set((entries % block).tolist())) == block
    pos, d = entry_tasks(bake, entries)
    orc = O.Oracle(cloud(), W, H, mode=1, fast=True, inscatter="lazy", light_direction=ds.SceneParams().light_direction)
    paths = np.array([[orc.point_radiance(int(e), f, pos[i], d[i])[0] for i, e in enumerate(entries)] for f in range(1, SAMPLES + 1)], f32)
    want = N.point_fold_reference(paths)
    got = bake.table().reshape(-1)[entries]
    assert np.array_equal(bits(got), bits(want))
    assert 12 <= (want > 0).sum() < 48                                    # rays that find lit cloud, and rays that leave the box unlit


@pytest.mark.gpu
def test_the_handles_mode_does_not_matter_and_its_image_is_left_alone(scene):
    want = bits(scene["dense"].table())
    for mode in (1, 2):
        with tracer(mode=mode) as tr, tr.traced_bake(*GRID, SAMPLES) as bake:
            assert np.array_equal(bits(bake.table()), want), mode
    with tracer() as tr:
        tr.render_subframe(1)
        tr.accumulate(1)
        tr.render_accumulate(2, 1)
        before = (tr.mean(), tr.m2(), tr.frame(), tr.subframes, tr.rendered_subframes())
        with tr.traced_bake(*GRID, SAMPLES, compact=True) as bake:
            bake.trace_more(1)
            after = (tr.mean(), tr.m2(), tr.frame(), tr.subframes, tr.rendered_subframes())
        for x, y in zip(before[:3], after[:3]):
            assert np.array_equal(bits(x), bits(y)) and x.any()
        assert before[3:] == after[3:] == (2, 2)
        tr.render_accumulate(3, 1)                                        # ... and the render goes on
        assert tr.subframes == 3


@pytest.mark.gpu
def test_sparse_and_compact_agree_with_dense_on_the_active_nodes(scene):
    dense, sparse, compact = scene["dense"], scene["sparse"], scene["compact"]
    nodes = reference_nodes(GRID[0])
    on = nodes.reshape(-1) != 0
    block = GRID[1] * GRID[2]
    full = dense.table().reshape(-1, GRID[1], GRID[2])
    sp = sparse.table().reshape(-1, GRID[1], GRID[2])
    assert np.array_equal(bits(sp[on]), bits(full[on])) and full[on].any()
    assert not bits(sp[~on]).any() and full[~on].any()                    # 0.0f off the mask, where the dense bake traced
    stored = compact.stored_table()
    assert stored.shape == (315, GRID[1], GRID[2]) and not bits(stored[0]).any()
    assert np.array_equal(bits(stored[1:]), bits(full[on]))               # the active blocks in list order
    assert np.array_equal(bits(compact.table()), bits(sparse.table()))
    for bake in (sparse, compact):
        ti = bake.trace_info()
        assert ti["traced"] and ti["samples"] == SAMPLES and ti["paths"] == 314 * block * SAMPLES
        assert np.array_equal(bake.mask(), nodes) and bake.sparse_info["active_nodes"] == 314 and bake.sparse_info["sparse"]
        assert np.array_equal(bits(bake.directions()), bits(dense.directions()))
    assert np.array_equal(compact.slots(), N.bake_slots_reference(nodes))
    assert compact.storage_info == {"compact": True, "slots": 315, "stored_entries": 315 * block, "table_bytes": 4 * 315 * block,
                                    "index_bytes": 4 * 504}
    assert dense.storage_info["stored_entries"] == ENTRIES and not dense.sparse_info["sparse"] and dense.mask().all()


@pytest.mark.gpu
def test_increments_and_cuts_give_the_same_bits(monkeypatch):
    with tracer() as tr, tr.traced_bake(*GRID, 8) as whole, tr.traced_bake(*GRID, 3) as parts:
        want = bits(whole.table())
        assert not np.array_equal(bits(parts.table()), want)
        parts.trace_more(5)
        assert np.array_equal(bits(parts.table()), want)
        assert parts.trace_info()["samples"] == 8 and parts.trace_info()["paths"] == ENTRIES * 8
    # 64 results per pass: 189 chunks of 64 entries, one sample per pass
    monkeypatch.setenv("CT_BAKE_TRACE_RESULTS", "64")
    with tracer() as cut:
        monkeypatch.delenv("CT_BAKE_TRACE_RESULTS")
        with cut.traced_bake(*GRID, 8) as bake:
            assert np.array_equal(bits(bake.table()), want)
        with cut.traced_bake(*GRID, 8, compact=True) as bake:
            on = reference_nodes(GRID[0]).reshape(-1) != 0
            assert np.array_equal(bits(bake.stored_table()[1:]), want.reshape(-1, GRID[1], GRID[2])[on])


def wrapped_entries_equal_the_public_estimator(point, bake, entries, samples):
    """`entries` (virtual indices >= 2^20, distinct modulo 2^20) of `bake` against a 2^20-task call of the public estimator with
    entry e at array index e mod 2^20 -- the index with e's seed base (uint32)(e * 4096) -- and every other slot a task that
    misses the box."""
    slot = entries % 2 ** 20
    assert len(entries) == 2048 and entries.min() >= 2 ** 20 and len(np.unique(slot)) == 2048
    pos, d = entry_tasks(bake, entries)
    all_pos = np.tile(np.array([10, 10, 10], f32), (2 ** 20, 1))
    all_d = np.tile(np.array([1, 0, 0], f32), (2 ** 20, 1))
    all_pos[slot], all_d[slot] = pos, d
    tasks = point.point_radiance_launch(ds.make_point_tasks(all_pos, all_d), 1, samples)
    want = tasks["radiance"][slot]
    got = bake.table().reshape(-1)[entries]
    assert np.array_equal(bits(got), bits(want)) and want.any()
    others = np.ones(2 ** 20, bool)
    others[slot] = False
    assert not tasks["radiance"][others].any()


@pytest.mark.gpu
def test_entries_beyond_2_to_the_20_keep_their_own_index(scene):
    """(33, 33, 33) x 8 x 4 has 1 149 984 virtual entries, the smallest shape at which a 32-bit entry index or seed base goes
    wrong: an entry e >= 2^20 is the task at array index e of the public estimator, whose seed base (uint32)(e * 4096) is that of
    index e - 2^20.  On cloud() the nodes of that grid with e >= 2^20 are its three uppermost z layers, which the mask leaves
    inactive, so a compact bake of this grid never reaches such an entry.  The grid's wrap is therefore held on its DENSE traced
    bake, which traces every node, with the compact bake held to the dense one on every active block; and the compact bake's own
    route to e >= 2^20 -- the virtual index made from the list -- on (33, 33, 33) x 8 x 16, where node 8192 on is beyond 2^20."""
    grid, nphi, nc, samples = (33, 33, 33), 8, 4, 2
    block = nphi * nc
    nodes = reference_nodes(grid).reshape(-1)
    active = np.flatnonzero(nodes)
    assert 33 ** 3 * block == 1149984 > 2 ** 20 and (len(active) + 1) * block < 2 ** 22 < 2 ** 26
    assert active.max() * block < 2 ** 20
    tr, point = scene["tr"], scene["point"]
    with tr.traced_bake(grid, nphi, nc, samples, compact=True) as compact, tr.traced_bake(grid, nphi, nc, samples) as dense:
        assert compact.info["entries"] == dense.info["entries"] == 1149984 and compact.sparse_info["active_nodes"] == len(active)
        late = np.arange(2 ** 20 // block, 33 ** 3)
        pick = late[np.linspace(0, len(late) - 1, 64).astype(np.int64)]
        entries = (pick[:, None] * block + np.arange(block)[None, :]).reshape(-1)
        wrapped_entries_equal_the_public_estimator(point, dense, entries, samples)
        blocks = dense.table().reshape(-1, nphi, nc)[active]
        assert np.array_equal(bits(compact.stored_table()[1:]), bits(blocks)) and blocks.any()
    nc = 16
    block = nphi * nc
    assert (len(active) + 1) * block < 2 ** 26
    with tr.traced_bake(grid, nphi, nc, samples, compact=True) as compact:
        late = active[active * block >= 2 ** 20]
        assert len(late) >= 2048
        pick = late[np.linspace(0, len(late) - 1, 2048).astype(np.int64)]
        entries = pick * block + (np.arange(2048) * 7) % block            # (distinct modulo 2^20: the helper asserts it)
        wrapped_entries_equal_the_public_estimator(point, compact, entries, samples)


@pytest.mark.gpu
def test_rendering_from_a_traced_bake(scene):
    import torch
    tr, dense, compact = scene["tr"], scene["dense"], scene["compact"]
    want = tr.baked_render_subframe(dense, SID, rgb_scale=SCALE).cpu().numpy()
    got = tr.baked_render_subframe(compact, SID, rgb_scale=SCALE).cpu().numpy()
    assert np.array_equal(bits(got), bits(want)) and want[..., :3].any()
    with tracer() as t2, t2.traced_bake(*GRID, SAMPLES) as d2, t2.traced_bake(*GRID, SAMPLES, compact=True) as c2:
        for direct in (False, True):
            t2.reset()
            t2.baked_render_accumulate(d2, 1, 2, rgb_scale=SCALE, direct=direct)
            mean, m2 = t2.mean(), t2.m2()
            t2.reset()
            t2.baked_render_accumulate(c2, 1, 2, rgb_scale=SCALE, direct=direct)
            assert t2.subframes == 2 and np.array_equal(bits(t2.mean()), bits(mean)) and np.array_equal(bits(t2.m2()), bits(m2))
            assert mean[..., :3].any(), direct
    # the lookup, against its numpy definition on the downloaded table
    info = dense.info
    box = np.array(tr.dims, f32) / f32(max(tr.dims))
    rng = np.random.default_rng(21)
    pos = (rng.uniform(-0.5, 0.5, (256, 3)) * box).astype(f32)
    d = rng.normal(size=(256, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
    ref = N.bake_lookup_reference(dense.table(), info, box, pos, d)
    look = tr.bake_lookup(dense, torch.from_numpy(pos).cuda(), torch.from_numpy(d).cuda()).cpu().numpy()
    assert np.array_equal(look, ref) and np.ptp(ref) > 0
    # a shard: its own tiles of the unsharded frame, from a bake made on the shard's handle, whose table is the unsharded one
    with tracer(shard_index=1, shard_count=2) as sh, sh.traced_bake(*GRID, SAMPLES, compact=True) as sb:
        assert np.array_equal(bits(sb.stored_table()), bits(compact.stored_table()))
        frame = sh.baked_render_shard_subframe(sb, SID, rgb_scale=SCALE).cpu().numpy()
        own = frame[..., 3] == 1
        assert 0 < own.sum() < W * H and not frame[~own].any()
        assert np.array_equal(bits(frame[own]), bits(want[own])) and frame[own][:, :3].any()
        sh.baked_render_shard_accumulate(sb, 1, 2, rgb_scale=SCALE)
        tr_mean = None
        with tracer() as whole, whole.traced_bake(*GRID, SAMPLES, compact=True) as wb:
            whole.baked_render_accumulate(wb, 1, 2, rgb_scale=SCALE)
            tr_mean = whole.mean()
        assert np.array_equal(bits(sh.mean()[own]), bits(tr_mean[own])) and not sh.mean()[~own].any()


@pytest.mark.gpu
def test_a_new_light_needs_a_retrace(scene):
    with tracer() as tr, tr.traced_bake(*GRID, SAMPLES, compact=True) as bake, N.Network(tr, weights(SMALL), 32, 1, 1) as net, \
            tr.network_bake(net, (3, 3, 3), 4, 2) as netbake:
        old = bake.stored_table()
        # a traced bake takes no network, a network's bake no samples
        assert tr.L.ct_bake_update(tr.h, net.n, bake.b) == _lib.CT_E_INVAL and "ct_bake_retrace" in tr.L.ct_last_error(tr.h).decode()
        assert np.array_equal(bits(bake.stored_table()), bits(old))
        assert _code(netbake.trace_more, 1) == _lib.CT_E_INVAL and _code(netbake.retrace, 1) == _lib.CT_E_INVAL
        assert netbake.trace_info() == {"traced": False, "samples": 0, "paths": 0, "trace_ms": 0.0, "fold_ms": 0.0}
        assert netbake.directions().shape == (4, 2, 3)
        tr.set_light(LIGHT2)
        assert not bake.info["current"]
        assert _code(bake.trace_more, 1) == _lib.CT_E_STATE
        assert _code(tr.baked_render_subframe, bake, SID) == _lib.CT_E_STATE
        assert np.array_equal(bits(bake.stored_table()), bits(old)) and bake.trace_info()["samples"] == SAMPLES
        bake.retrace(SAMPLES)
        assert bake.info["current"] and np.array_equal(bake.info["light"], tr.light_direction())
        ti = bake.trace_info()
        assert ti["samples"] == SAMPLES and ti["paths"] == 314 * GRID[1] * GRID[2] * SAMPLES
        with tracer(light_direction=LIGHT2) as fresh, fresh.traced_bake(*GRID, SAMPLES, compact=True) as again:
            assert np.array_equal(bits(bake.stored_table()), bits(again.stored_table()))
            assert np.array_equal(bits(bake.directions()), bits(again.directions()))
            want = fresh.baked_render_subframe(again, SID, rgb_scale=SCALE).cpu().numpy()
        assert not np.array_equal(bits(bake.stored_table()), bits(old))
        assert np.array_equal(bits(tr.baked_render_subframe(bake, SID, rgb_scale=SCALE).cpu().numpy()), bits(want)) and want[..., :3].any()


@pytest.mark.gpu
def test_errors_leave_the_handle_usable(scene):
    tr, dense = scene["tr"], scene["dense"]
    L, h = tr.L, tr.h
    want = tr.baked_render_subframe(dense, SID, rgb_scale=SCALE).cpu().numpy()
    table = dense.table()

    def unchanged():
        assert np.array_equal(bits(tr.baked_render_subframe(dense, SID, rgb_scale=SCALE).cpu().numpy()), bits(want))
        assert np.array_equal(bits(dense.table()), bits(table)) and dense.trace_info()["samples"] == SAMPLES

    def desc(grid=(2, 2, 2), nphi=4, nc=2, abi=_lib.CT_ABI_VERSION):
        return _lib.CtBakeDesc(abi, (C.c_uint32 * 3)(*grid), nphi, nc)

    def message():
        return L.ct_last_error(h).decode()

    for kind, samples, kw, word in ((3, 1, {}, "kind"), (0xffffffff, 1, {}, "kind"), (0, 65536, {}, "65535"),
                                    (1, 1, dict(abi=_lib.CT_ABI_VERSION + 1), "abi_version"), (2, 1, dict(grid=(1, 2, 2)), "grid[0]"),
                                    (0, 1, dict(nphi=6), "azimuths"), (0, 1, dict(nc=65), "cosines"),
                                    (0, 1, dict(grid=(256, 256, 256), nphi=64, nc=64), "2^26")):
        d, out = desc(**kw), C.c_void_p(1)
        assert L.ct_bake_traced(h, C.byref(d), kind, samples, C.byref(out)) == _lib.CT_E_INVAL and not out.value, (kind, samples, kw)
        assert word in message() and "ct_bake_traced" in message(), (word, message())
    d, out = desc(), C.c_void_p(1)
    assert L.ct_bake_traced(h, None, 0, 1, C.byref(out)) == _lib.CT_E_INVAL
    assert L.ct_bake_traced(h, C.byref(d), 0, 1, None) == _lib.CT_E_INVAL
    unchanged()
    # the sample counts
    assert _code(dense.trace_more, 0) == _lib.CT_E_INVAL and _code(dense.retrace, 0) == _lib.CT_E_INVAL
    assert _code(dense.trace_more, 65536) == _lib.CT_E_INVAL and _code(dense.retrace, 65536) == _lib.CT_E_INVAL
    assert L.ct_bake_trace_more(h, None, 1) == _lib.CT_E_INVAL and L.ct_bake_retrace(h, None, 1) == _lib.CT_E_INVAL
    unchanged()
    # a bake of another handle, a simple-kernel handle
    with tracer() as other, tracer(flags=_lib.CT_FLAG_SIMPLE_KERNEL) as simple:
        assert L.ct_bake_trace_more(other.h, dense.b, 1) == _lib.CT_E_INVAL and "another handle" in L.ct_last_error(other.h).decode()
        assert L.ct_bake_retrace(other.h, dense.b, 1) == _lib.CT_E_INVAL
        assert _code(other.baked_render_subframe, dense, SID) == _lib.CT_E_INVAL
        out = C.c_void_p(1)
        assert L.ct_bake_traced(simple.h, C.byref(d), 0, 1, C.byref(out)) == _lib.CT_E_INVAL and not out.value
        assert "persistent kernel" in L.ct_last_error(simple.h).decode()
    unchanged()
    # ct_bake_directions takes exactly 3 Nphi Nc floats
    floats = np.empty(3 * 24 + 1, f32)
    for count in (0, 71, 73, 24):
        assert L.ct_bake_directions(dense.b, floats.ctypes.data_as(C.c_void_p), count) == _lib.CT_E_INVAL
    assert L.ct_bake_directions(dense.b, None, 72) == _lib.CT_E_INVAL
    assert L.ct_bake_trace_info(dense.b, None) == _lib.CT_E_INVAL
    unchanged()
    # no samples: CT_OK, an all-zero table, nothing launched
    counters = tr.counters()
    with tr.traced_bake(*GRID, 0) as empty, tr.traced_bake(*GRID, 0, compact=True) as empty_compact:
        ti = empty.trace_info()
        assert ti["traced"] and ti["samples"] == 0 and ti["paths"] == 0 and ti["trace_ms"] == 0 and ti["fold_ms"] == 0
        assert not bits(empty.table()).any() and not bits(empty_compact.stored_table()).any()
        assert tr.counters() == counters
        empty.trace_more(SAMPLES)                                         # ... and it can be traced from there
        assert np.array_equal(bits(empty.table()), bits(table))
    unchanged()


@pytest.mark.gpu
def test_a_table_holds_at_most_2_to_the_24_experiments():
    """Arithmetic, not tracing: a sparse bake of an empty volume has no active node, so its calls count samples and launch
    nothing.  256 calls of 65535 are 16 776 960; 256 more fit, then none."""
    with ds.CloudTracer(np.zeros((20, 33, 45), np.uint8), width=W, height=H) as tr, tr.traced_bake((6, 5, 4), 4, 2, 65535, sparse=True) as bake:
        assert bake.sparse_info["active_nodes"] == 0
        for _ in range(255):
            bake.trace_more(65535)
        assert bake.trace_info()["samples"] == 256 * 65535 == 2 ** 24 - 256
        for _ in range(3):
            assert _code(bake.trace_more, 65535) == _lib.CT_E_INVAL and _code(bake.trace_more, 257) == _lib.CT_E_INVAL
        assert "2^24" in tr.L.ct_last_error(tr.h).decode()
        bake.trace_more(256)
        assert bake.trace_info() == {"traced": True, "samples": 2 ** 24, "paths": 0, "trace_ms": 0.0, "fold_ms": 0.0}
        assert _code(bake.trace_more, 1) == _lib.CT_E_INVAL
        assert not bits(bake.table()).any()
        bake.retrace(7)                                                   # a retrace starts the count again
        assert bake.trace_info()["samples"] == 7


@pytest.mark.gpu
def test_cli_renders_from_a_traced_bake(tmp_path):
    from deepestscatter_amd import build
    cli = build.build_cli()
    common = [str(cli), "procedural:64", "--size", f"{W}x{H}", "--spp", "4", "--net-scale", "0.5,2,3"]
    images = {}
    for name, extra in (("dense", []), ("compact", ["--net-bake-compact"])):
        (tmp_path / name).mkdir()
        r = subprocess.run(common + ["--traced-bake", "9,8,7,8,3", "--bake-samples", "4", "--net-direct"] + extra + ["--out", str(tmp_path / name)],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        images[name] = {p.name: p.read_bytes() for p in sorted((tmp_path / name).glob("*.exr"))}
    assert len(images["dense"]) >= 2 and images["dense"].keys() == images["compact"].keys()
    for name, data in images["dense"].items():
        assert data == images["compact"][name] and len(data) > 0, name
    N.save_weights(tmp_path / "w.bin", weights(SMALL), SMALL)
    r = subprocess.run(common + ["--traced-bake", "9,8,7,8,3", "--bake-samples", "4", "--network", str(tmp_path / "w.bin"), "--out", str(tmp_path)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--traced-bake" in r.stdout + r.stderr and "--network" in r.stdout + r.stderr
    r = subprocess.run(common + ["--traced-bake", "9,8,7,8,3", "--out", str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--bake-samples" in r.stdout + r.stderr
