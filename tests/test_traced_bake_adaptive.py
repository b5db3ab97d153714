"""ct_bake_traced_adaptive: a traced bake in rounds, with per-entry m2 and count and the reference's stopping rule (include/
cloudtrace.h, "the adaptive traced bake").

Everything is held bit for bit -- np.array_equal on the bits, no tolerance -- to a host loop over the public estimator
(ct_point_radiance_launch on a mode-1 handle) with the numpy rule, to the oracle, or to another bake.

Scene and GRID are those of tests/test_traced_bake.py: make_procedural_cloud(64), 24 x 16, (9, 8, 7) x 8 x 3, 314 active nodes,
7 536 stored entries when sparse.  Parameters P: R = 4, cap 32, rel_tol 0.5, abs_tol 1e-4, zero_samples 7 -- every round
compacts, the survivor lists are sparse and unaligned, and both exits of the rule occur."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import _oracle as O
import deepestscatter_amd as ds
from deepestscatter_amd import _lib
from deepestscatter_amd import cloudtrace as ct
from deepestscatter_amd import network as N
from test_network_render import H, LIGHT2, SCALE, SID, W, cloud
from test_traced_bake import DELTA, ENTRIES, GRID, MARCH, _code, bits, entry_tasks, reference_nodes, tracer

P = dict(round_samples=4, max_samples=32, rel_tol=0.5, abs_tol=1e-4, zero_samples=7)
BLOCK = GRID[1] * GRID[2]
ACTIVE = 314 * BLOCK
f32 = np.float32
EPS = np.finfo(f32).eps


def params(**kw):
    return N.AdaptiveParams(**{**P, **kw})


def cparams(abi=_lib.CT_ABI_VERSION, **kw):
    p = {**P, **kw}
    return _lib.CtBakeAdaptive(abi, p["round_samples"], p["max_samples"], p["zero_samples"], p["rel_tol"], p["abs_tol"])


def active_entries():
    on = reference_nodes(GRID[0]).reshape(-1) != 0
    return np.repeat(on, BLOCK)


# ---------------------------------------------------------------------------------------------------- CPU
def test_symbols_resolve_and_answer_null_arguments(product_lib):
    L = product_lib
    for name in ("ct_bake_traced_adaptive", "ct_bake_trace_adaptive_more", "ct_bake_retrace_adaptive", "ct_bake_adaptive_info",
                 "ct_bake_download_counts", "ct_bake_download_m2"):
        assert hasattr(L, name) and name in _lib.EXPORTS + _lib.DIGIT_EXPORTS
    d = _lib.CtBakeDesc(_lib.CT_ABI_VERSION, (C.c_uint32 * 3)(2, 2, 2), 4, 2)
    p = cparams()
    out = C.c_void_p()
    assert L.ct_bake_traced_adaptive(None, C.byref(d), _lib.CT_BAKE_SPARSE, C.byref(p), C.byref(out)) == _lib.CT_E_INVAL
    assert L.ct_bake_traced_adaptive(None, None, 0, None, None) == _lib.CT_E_INVAL
    assert L.ct_bake_trace_adaptive_more(None, None, 8) == _lib.CT_E_INVAL
    assert L.ct_bake_retrace_adaptive(None, None) == _lib.CT_E_INVAL
    assert L.ct_bake_adaptive_info(None, None) == _lib.CT_E_INVAL
    assert L.ct_bake_download_counts(None, None, 0) == _lib.CT_E_INVAL
    assert L.ct_bake_download_m2(None, None, 0) == _lib.CT_E_INVAL
    A, T = _lib.CtBakeAdaptive, _lib.CtBakeAdaptiveInfo
    assert [C.sizeof(A), A.round_samples.offset, A.max_samples.offset, A.zero_samples.offset, A.rel_tol.offset, A.abs_tol.offset] == \
        [24, 4, 8, 12, 16, 20]
    assert [C.sizeof(T), T.rounds.offset, T.entries_active.offset, T.converged.offset, T.capped.offset, T.paths.offset, T.trace_ms.offset,
            T.test_ms.offset] == [88, 24, 32, 40, 48, 56, 64, 80]


def test_struct_layout_matches_the_header():
    import tempfile
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    fields = ["round_samples", "max_samples", "zero_samples", "rel_tol", "abs_tol", "rounds", "entries_active", "converged", "capped", "paths",
              "trace_ms", "fold_ms", "test_ms"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "cloudtrace.h"\nint main(){printf("%zu %zu %zu %zu", sizeof(CtBakeAdaptive), '
           'offsetof(CtBakeAdaptive, zero_samples), offsetof(CtBakeAdaptive, abs_tol), sizeof(CtBakeAdaptiveInfo));'
           + "".join(f'printf(" %zu", offsetof(CtBakeAdaptiveInfo, {f}));' for f in fields) + "return 0;}")
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "p.c").write_text(src)
        subprocess.run(["gcc", "-I", str(root / "include"), "-o", f"{d}/p", f"{d}/p.c"], check=True)
        out = [int(v) for v in subprocess.run([f"{d}/p"], capture_output=True, text=True, check=True).stdout.split()]
    assert out[:4] == [24, 12, 20, 88]
    assert out[4:] == [getattr(_lib.CtBakeAdaptiveInfo, f).offset for f in fields] == [4, 8, 12, 16, 20, 24, 32, 40, 48, 56, 64, 72, 80]


def test_point_fold_var_reference_is_a_literal_loop_of_add_experiment_result():
    rng = np.random.default_rng(6)
    values = (rng.random((9, 7), dtype=f32) * f32(40)).astype(f32)
    values[:, 3] = 0
    mean, m2 = np.zeros(7, f32), np.zeros(7, f32)
    for i in range(7):
        radiance, variance, count = f32(0), f32(0), 0
        for x in values[:, i]:                                            # PointRadianceTask.h:40-51
            count += 1
            new_weight = f32(1.0 / float(f32(count)))
            previous = radiance
            new_mean = f32(radiance + f32(f32(x - previous) * new_weight))
            radiance = new_mean
            variance = f32(variance + f32(f32(x - previous) * f32(x - new_mean)))
        mean[i], m2[i] = radiance, variance
    got = N.point_fold_var_reference(values)
    assert got[0].dtype == f32 and got[1].dtype == f32
    assert np.array_equal(bits(got[0]), bits(mean)) and np.array_equal(bits(got[1]), bits(m2)) and (got[2] == 9).all() and m2.any()
    assert np.array_equal(bits(got[0]), bits(N.point_fold_reference(values)))
    # continued from a state, with counts that differ between the entries' states
    first = N.point_fold_var_reference(values[:4])
    again = N.point_fold_var_reference(values[4:], *first)
    assert all(np.array_equal(a.view(np.uint32) if a.dtype == f32 else a, b.view(np.uint32) if b.dtype == f32 else b) for a, b in zip(again, got))
    # ... and the oracle's own fold of its own paths: radiance and runningVariance of orc_point_radiance_launch
    orc = O.Oracle(cloud(), W, H, mode=1, fast=True, inscatter="lazy", light_direction=ds.SceneParams().light_direction)
    pos = np.array([[0.0, 0.0, 0.0], [0.1, -0.1, 0.05], [-0.2, 0.1, 0.0], [0.05, 0.2, -0.1]], f32)
    d = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0], [0.6, 0, 0.8]], f32)
    tasks = orc.point_radiance_launch(ds.make_point_tasks(pos, d), 1, 6)
    paths = np.array([[orc.point_radiance(i, f, pos[i], d[i])[0] for i in range(4)] for f in range(1, 7)], f32)
    mean, m2, count = N.point_fold_var_reference(paths)
    assert np.array_equal(bits(mean), bits(tasks["radiance"])) and np.array_equal(bits(m2), bits(tasks["runningVariance"]))
    assert np.array_equal(count, tasks["experimentCount"]) and m2.any()


def test_point_converged_reference_is_the_collectors_test():
    rng = np.random.default_rng(7)
    n = 4096
    rad = (rng.random(n, dtype=f32) * f32(3)).astype(f32)
    var = (rng.random(n, dtype=f32) * f32(50)).astype(f32)
    cnt = rng.integers(1, 300000, n)
    rad[:64] = 0                                                          # mean < FLT_EPSILON, on both sides of zero_samples
    rad[64:96] = EPS / f32(2)
    rad[96:128] = EPS
    cnt[:96:3] = np.arange(32) % 9
    var[128:256] = 0                                                      # m2 = 0
    var[:32] = 0
    cnt[256:320] = 0                                                      # count = 0: 0 / 0
    rad[320:352] = np.nan
    var[352:384] = np.nan
    var[384:400] = np.inf
    cnt[400:432] = rng.integers(99990, 100010, 32)
    rad[400:432] = 0
    var[432:1024] = (var[432:1024] * f32(1e-3)).astype(f32)               # states near the thresholds
    for rel, ab, zero in ((2e-2, 1e-4, 100000), (0.5, 1e-4, 7), (0.0, 0.0, 0)):
        with np.errstate(divide="ignore", invalid="ignore"):              # collector.RadianceCollector.update's expressions
            Nf = cnt.astype(f32)
            absolute = (f32(1.96) * np.sqrt(var / Nf)) / np.sqrt(Nf)
            relative = absolute / (rad + EPS)
        converged = (relative < f32(rel)) | (absolute < f32(ab))
        converged = np.where(rad < EPS, cnt > zero, converged)
        got = N.point_converged_reference(rad, var, cnt, rel, ab, zero)
        assert got.dtype == bool and np.array_equal(got, converged)
        # a NaN compares false: a NaN m2 never converges, a NaN mean only by the absolute interval
        assert not got[352:384].any() and np.array_equal(got[320:352], (absolute < f32(ab))[320:352])
        if rel:
            assert 0 < got.sum() < n and got[:96].any() and not got[:96].all()


def test_python_refuses_contradicting_arguments():
    with pytest.raises(ValueError):
        N.Bake(None, None, (2, 2, 2), 4, 2, sparse=True, compact=True, adaptive=params())
    with pytest.raises(ValueError):
        ds.CloudTracer.traced_bake_adaptive(None, (2, 2, 2), 4, 2, 4, 32, sparse=True, compact=True)
    with pytest.raises(ValueError):
        N.Bake(None, object(), (2, 2, 2), 4, 2, adaptive=params())        # a network and rounds
    with pytest.raises(ValueError):
        N.Bake(None, None, (2, 2, 2), 4, 2, samples=4, adaptive=dict(P))  # uniform and adaptive
    with pytest.raises(TypeError):
        N.Bake(None, None, (2, 2, 2), 4, 2, adaptive=dict(P, rounds=3))   # no such parameter


# ---------------------------------------------------------------------------------------------------- GPU
def adaptive_reference(point, pos, d, live, p=P, index=None):
    """The definition as a host loop over the public estimator: the tasks stay at their array index (the seeds), every round is
    one call with frames c + 1 .. c + R, the state is carried in the task structs, and only the entries still live take the
    call's result.  live: bool per task, the first round's set -> (tasks, the round every entry stopped in or 0, rounds)."""
    tasks = ds.make_point_tasks(pos, d)
    live = live.copy()
    stopped = np.zeros(len(tasks), np.int64)
    c = rounds = 0
    while live.any() and c < p["max_samples"]:
        new = point.point_radiance_launch(tasks.copy(), c + 1, p["round_samples"])
        tasks[live] = new[live]
        c += p["round_samples"]
        rounds += 1
        conv = N.point_converged_reference(tasks["radiance"], tasks["runningVariance"], tasks["experimentCount"], p["rel_tol"], p["abs_tol"],
                                           p["zero_samples"])
        stopped[live & conv] = rounds
        live &= ~conv
    return tasks, stopped, rounds


def check_against(bake, tasks, stopped, rounds, live0, cap=P["max_samples"]):
    """A dense or sparse bake against the reference's task structs, and its info against the reference's rounds."""
    mean, m2, count = bake.table().reshape(-1), bake.m2().reshape(-1), bake.counts().reshape(-1)
    assert count.dtype == np.uint32 and m2.dtype == f32
    assert np.array_equal(bits(mean[live0]), bits(tasks["radiance"][live0]))
    assert np.array_equal(bits(m2[live0]), bits(tasks["runningVariance"][live0]))
    assert np.array_equal(count[live0], tasks["experimentCount"][live0])
    assert not bits(mean[~live0]).any() and not bits(m2[~live0]).any() and not count[~live0].any()
    info = bake.adaptive_info()
    capped = int((live0 & (stopped == 0)).sum())
    assert info["adaptive"] and info["rounds"] == rounds and info["entries_active"] == live0.sum()
    assert info["capped"] == capped and info["converged"] == live0.sum() - capped
    assert info["paths"] == int(tasks["experimentCount"][live0].sum())
    assert (info["round_samples"], info["max_samples"], info["zero_samples"]) == (P["round_samples"], cap, P["zero_samples"])
    assert info["rel_tol"] == f32(P["rel_tol"]) and info["abs_tol"] == f32(P["abs_tol"])
    assert info["trace_ms"] > 0 and info["fold_ms"] > 0 and info["test_ms"] > 0
    ti = bake.trace_info()
    assert ti["traced"] and ti["samples"] == rounds * P["round_samples"] and ti["paths"] == info["paths"]
    return info


_REFS = {}


@pytest.fixture(scope="module")
def scene():
    """A mode-0 MARCH tracer with the dense, sparse and compact adaptive bakes of GRID and P, a mode-1 tracer for the public
    estimator, and the reference of the sparse bake.  No test changes their light or accumulates on them."""
    with tracer() as tr, tracer(mode=1) as point:
        made = []
        try:
            s = {"tr": tr, "point": point}
            before = tr.counters()["paths"]
            for key, kw in (("sparse", {"sparse": True}), ("dense", {}), ("compact", {"compact": True})):
                s[key] = tr.traced_bake_adaptive(*GRID, **P, **kw)
                made.append(s[key])
                if key == "sparse":
                    s["sparse_paths"] = tr.counters()["paths"] - before
            pos, d = entry_tasks(s["sparse"])
            s["ref"] = adaptive_reference(point, pos, d, active_entries())
            yield s
        finally:
            for obj in reversed(made):
                obj.close()


@pytest.mark.gpu
@pytest.mark.parametrize("estimator, flags", [(MARCH, 0), (DELTA, 0), (MARCH, _lib.CT_FLAG_TEX_FIXED8)], ids=["march", "delta", "march-fixed8"])
def test_every_entry_is_the_host_loop_over_the_public_estimator(scene, estimator, flags):
    """mean, m2 and count of all 7 536 entries of a sparse bake, rounds, converged, capped and paths."""
    live0 = active_entries()
    assert live0.sum() == ACTIVE == 7536 and len(live0) == ENTRIES

    def check(bake, ref, paths):
        tasks, stopped, rounds = ref
        # the reference itself: entries stop in at least 4 different rounds, 1 000 or more before the cap, 1 000 or more reach it
        at_cap = live0 & (stopped == 0)
        assert len(set(stopped[live0 & (stopped != 0)].tolist())) >= 4 and rounds == 8
        assert (live0 & (stopped != 0) & (tasks["experimentCount"] < P["max_samples"])).sum() >= 1000 and at_cap.sum() >= 1000
        assert (tasks["experimentCount"][at_cap] == P["max_samples"]).all()
        assert (tasks["radiance"][live0] < EPS).any() and (tasks["radiance"][live0 & (stopped != 0)] >= EPS).any()   # both exits of the rule
        info = check_against(bake, tasks, stopped, rounds, live0)
        assert paths == info["paths"]
        return bake.table()

    if (estimator, flags) == (MARCH, 0):
        check(scene["sparse"], scene["ref"], scene["sparse_paths"])
        return
    with tracer(estimator=estimator, flags=flags) as tr, tracer(mode=1, estimator=estimator, flags=flags) as point:
        before = tr.counters()["paths"]
        with tr.traced_bake_adaptive(*GRID, **P, sparse=True) as bake:
            paths = tr.counters()["paths"] - before
            pos, d = entry_tasks(bake)
            got = check(bake, adaptive_reference(point, pos, d, live0), paths)
            assert not np.array_equal(bits(got), bits(scene["sparse"].table()))


@pytest.mark.gpu
def test_dense_sparse_and_compact_agree_on_the_active_nodes(scene):
    dense, sparse, compact = scene["dense"], scene["sparse"], scene["compact"]
    on = reference_nodes(GRID[0]).reshape(-1) != 0
    shape = (-1, GRID[1], GRID[2])
    for get in (lambda b: bits(b.stored_table() if b is compact else b.table()), lambda b: bits(b.m2()), lambda b: b.counts()):
        full, sp, st = get(dense).reshape(shape), get(sparse).reshape(shape), get(compact)
        assert np.array_equal(sp[on], full[on]) and full[on].any()
        assert not sp[~on].any()                                          # 0 / 0 / 0 off the mask
        assert st.shape == (315, GRID[1], GRID[2]) and not st[0].any()    # ... and in the zero block
        assert np.array_equal(st[1:], full[on])
    assert np.array_equal(bits(compact.table()), bits(sparse.table()))
    # the dense bake's inactive nodes against the reference with every entry live: count 8 by the zero rule, or their own value
    pos, d = entry_tasks(dense)
    everything = np.ones(ENTRIES, bool)
    tasks, stopped, rounds = adaptive_reference(scene["point"], pos, d, everything)
    check_against(dense, tasks, stopped, rounds, everything)
    off = np.repeat(~on, BLOCK)
    count, mean = dense.counts().reshape(-1)[off], dense.table().reshape(-1)[off]
    assert (count[mean < EPS] == 8).all() and (mean < EPS).sum() > 1000 and (mean >= EPS).any()
    for bake in (sparse, compact):
        assert bake.adaptive_info()["entries_active"] == ACTIVE and bake.sparse_info["active_nodes"] == 314
        for key in ("rounds", "converged", "capped", "paths"):
            assert bake.adaptive_info()[key] == sparse.adaptive_info()[key]
    assert compact.storage_info["stored_entries"] == 315 * BLOCK and dense.storage_info["stored_entries"] == ENTRIES


@pytest.mark.gpu
def test_chunks_and_passes_give_the_same_bits(scene, monkeypatch):
    """512 results per pass: chunks of 512 live entries, one-sample passes."""
    monkeypatch.setenv("CT_BAKE_TRACE_RESULTS", "512")
    with tracer() as cut:
        monkeypatch.delenv("CT_BAKE_TRACE_RESULTS")
        for kind in ("sparse", "compact"):
            with cut.traced_bake_adaptive(*GRID, **P, **{kind: True}) as bake:
                want = scene[kind]
                get = (lambda b: b.stored_table()) if kind == "compact" else (lambda b: b.table())
                assert np.array_equal(bits(get(bake)), bits(get(want))) and np.array_equal(bits(bake.m2()), bits(want.m2()))
                assert np.array_equal(bake.counts(), want.counts())
                for key in ("rounds", "converged", "capped", "paths"):
                    assert bake.adaptive_info()[key] == want.adaptive_info()[key]


@pytest.mark.gpu
def test_raising_the_cap_continues_to_the_same_bits(scene):
    tr, want = scene["tr"], scene["compact"]
    with tr.traced_bake_adaptive(*GRID, **{**P, "max_samples": 16}, compact=True) as bake:
        first = bake.adaptive_info()
        assert bake.counts().max() == 16 and first["max_samples"] == 16 and first["rounds"] == 4 and first["capped"] > 1000
        assert not np.array_equal(bits(bake.stored_table()), bits(want.stored_table()))
        assert (bake.counts() == 16).sum() >= first["capped"]
        bake.trace_adaptive_more(32)
        assert np.array_equal(bits(bake.stored_table()), bits(want.stored_table())) and np.array_equal(bits(bake.m2()), bits(want.m2()))
        assert np.array_equal(bake.counts(), want.counts())
        info = bake.adaptive_info()
        for key in ("rounds", "converged", "capped", "paths", "max_samples", "entries_active"):
            assert info[key] == want.adaptive_info()[key], key
        assert bake.trace_info()["samples"] == 32 and bake.trace_info()["paths"] == info["paths"]
        # the cap only rises, in whole rounds
        for cap in (32, 16, 0, 34, 2 ** 24 + 4):
            assert _code(bake.trace_adaptive_more, cap) == _lib.CT_E_INVAL, cap
        assert np.array_equal(bake.counts(), want.counts()) and bake.adaptive_info()["max_samples"] == 32


@pytest.mark.gpu
def test_entries_and_live_positions_beyond_2_to_the_20(scene):
    """(33, 33, 33) x 8 x 4 dense, R = 4, cap 8: 1 149 984 entries, of which the zero rule keeps more than 2^20 live into the second
    round, so that round's list has positions beyond 2^20 and goes through in two chunks.  Entries e >= 2^20 are held to a
    2^20-task call of the public estimator per round, entry e at array index e mod 2^20 (the index with e's seed base), every
    other slot a task that misses the box."""
    grid, nphi, nc = (33, 33, 33), 8, 4
    p = {**P, "max_samples": 8}
    block = nphi * nc
    tr, point = scene["tr"], scene["point"]
    with tr.traced_bake_adaptive(grid, nphi, nc, **p) as bake:
        info = bake.adaptive_info()
        assert info["entries_active"] == 1149984 and info["rounds"] == 2
        count = bake.counts().reshape(-1)
        assert (count == 8).sum() > 2 ** 20 and (count == 4).sum() > 0 and ((count == 4) | (count == 8)).all()
        assert info["paths"] == int(count.astype(np.int64).sum())
        late = np.arange(2 ** 20 // block, 33 ** 3)
        pick = late[np.linspace(0, len(late) - 1, 64).astype(np.int64)]
        entries = (pick[:, None] * block + np.arange(block)[None, :]).reshape(-1)
        slot = entries % 2 ** 20
        assert len(entries) == 2048 and entries.min() >= 2 ** 20 and len(np.unique(slot)) == 2048
        pos, d = entry_tasks(bake, entries)
        all_pos = np.tile(np.array([10, 10, 10], f32), (2 ** 20, 1))
        all_d = np.tile(np.array([1, 0, 0], f32), (2 ** 20, 1))
        all_pos[slot], all_d[slot] = pos, d
        live = np.zeros(2 ** 20, bool)
        live[slot] = True
        tasks, stopped, rounds = adaptive_reference(point, all_pos, all_d, live, p)
        assert rounds == 2
        want = tasks[slot]
        assert np.array_equal(bits(bake.table().reshape(-1)[entries]), bits(want["radiance"])) and want["radiance"].any()
        assert np.array_equal(bits(bake.m2().reshape(-1)[entries]), bits(want["runningVariance"])) and want["runningVariance"].any()
        assert np.array_equal(count[entries], want["experimentCount"])
        assert set(np.unique(count[entries]).tolist()) == {4, 8}            # both exits among the entries that were checked


@pytest.mark.gpu
def test_rendering_from_an_adaptive_bake(scene):
    import torch
    tr, dense, compact = scene["tr"], scene["dense"], scene["compact"]
    want = tr.baked_render_subframe(dense, SID, rgb_scale=SCALE).cpu().numpy()
    got = tr.baked_render_subframe(compact, SID, rgb_scale=SCALE).cpu().numpy()
    assert np.array_equal(bits(got), bits(want)) and want[..., :3].any()
    with tracer() as t2, t2.traced_bake_adaptive(*GRID, **P) as d2, t2.traced_bake_adaptive(*GRID, **P, compact=True) as c2:
        for direct in (False, True):
            t2.reset()
            t2.baked_render_accumulate(d2, 1, 2, rgb_scale=SCALE, direct=direct)
            mean, m2 = t2.mean(), t2.m2()
            t2.reset()
            t2.baked_render_accumulate(c2, 1, 2, rgb_scale=SCALE, direct=direct)
            assert t2.subframes == 2 and np.array_equal(bits(t2.mean()), bits(mean)) and np.array_equal(bits(t2.m2()), bits(m2))
            assert mean[..., :3].any(), direct
    info = dense.info
    box = np.array(tr.dims, f32) / f32(max(tr.dims))
    rng = np.random.default_rng(22)
    pos = (rng.uniform(-0.5, 0.5, (256, 3)) * box).astype(f32)
    d = rng.normal(size=(256, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
    for bake in (dense, compact):                                         # (the compact bake: zeros off the mask)
        ref = N.bake_lookup_reference(bake.table(), info, box, pos, d)
        look = tr.bake_lookup(bake, torch.from_numpy(pos).cuda(), torch.from_numpy(d).cuda()).cpu().numpy()
        assert np.array_equal(look, ref) and np.ptp(ref) > 0
    assert np.array_equal(bits(dense.directions()), bits(compact.directions()))
    assert np.array_equal(bits(compact.table().reshape(-1)[active_entries()]), bits(compact.stored_table()[1:].reshape(-1)))


@pytest.mark.gpu
def test_a_new_light_needs_an_adaptive_retrace(scene):
    with tracer() as tr, tr.traced_bake_adaptive(*GRID, **P, compact=True) as bake:
        old = (bake.stored_table(), bake.m2(), bake.counts(), bake.adaptive_info())
        assert np.array_equal(bits(old[0]), bits(scene["compact"].stored_table()))
        tr.set_light(LIGHT2)
        assert not bake.info["current"]
        assert _code(bake.trace_adaptive_more, 64) == _lib.CT_E_STATE
        assert "ct_bake_retrace_adaptive" in tr.L.ct_last_error(tr.h).decode()
        assert _code(tr.baked_render_subframe, bake, SID) == _lib.CT_E_STATE
        assert np.array_equal(bits(bake.stored_table()), bits(old[0])) and np.array_equal(bake.counts(), old[2])
        assert bake.adaptive_info()["max_samples"] == 32
        bake.retrace_adaptive()
        assert bake.info["current"] and np.array_equal(bake.info["light"], tr.light_direction())
        with tracer(light_direction=LIGHT2) as fresh, fresh.traced_bake_adaptive(*GRID, **P, compact=True) as again:
            assert np.array_equal(bits(bake.stored_table()), bits(again.stored_table())) and np.array_equal(bits(bake.m2()), bits(again.m2()))
            assert np.array_equal(bake.counts(), again.counts())
            for key in ("rounds", "converged", "capped", "paths", "max_samples"):
                assert bake.adaptive_info()[key] == again.adaptive_info()[key], key
            want = fresh.baked_render_subframe(again, SID, rgb_scale=SCALE).cpu().numpy()
        assert not np.array_equal(bits(bake.stored_table()), bits(old[0]))
        assert np.array_equal(bits(tr.baked_render_subframe(bake, SID, rgb_scale=SCALE).cpu().numpy()), bits(want)) and want[..., :3].any()
        bake.trace_adaptive_more(36)                                      # ... and the retraced bake continues
        assert bake.adaptive_info()["rounds"] == 9 and bake.counts().max() == 36


@pytest.mark.gpu
def test_the_handles_image_is_left_alone():
    with tracer() as tr:
        tr.render_subframe(1)
        tr.accumulate(1)
        tr.render_accumulate(2, 1)
        before = (tr.mean(), tr.m2(), tr.frame(), tr.subframes, tr.rendered_subframes())
        with tr.traced_bake_adaptive(*GRID, **{**P, "max_samples": 8}, compact=True) as bake:
            bake.trace_adaptive_more(12)
            after = (tr.mean(), tr.m2(), tr.frame(), tr.subframes, tr.rendered_subframes())
        for x, y in zip(before[:3], after[:3]):
            assert np.array_equal(bits(x), bits(y)) and x.any()
        assert before[3:] == after[3:] == (2, 2)
        tr.render_accumulate(3, 1)                                        # ... and the render goes on
        assert tr.subframes == 3


@pytest.mark.gpu
def test_every_allocation_is_given_back(scene):
    start = ct.debug_allocations()
    with tracer() as tr:
        held = ct.debug_allocations()
        with tr.traced_bake_adaptive(*GRID, **{**P, "max_samples": 8}, compact=True) as bake:
            inside = ct.debug_allocations()
            assert inside["device_buffers"] >= held["device_buffers"] + 7   # table, m2, counts, two live lists, wave counts, ...
            tr.set_light(LIGHT2)
            bake.retrace_adaptive()
            bake.trace_adaptive_more(12)
            assert ct.debug_allocations()["device_buffers"] == inside["device_buffers"]
    assert ct.debug_allocations() == start


@pytest.mark.gpu
def test_errors_leave_the_handle_usable(scene):
    tr, sparse = scene["tr"], scene["sparse"]
    L, h = tr.L, tr.h
    want = tr.baked_render_subframe(sparse, SID, rgb_scale=SCALE).cpu().numpy()
    state = (sparse.table(), sparse.m2(), sparse.counts(), sparse.adaptive_info()["paths"])

    def unchanged():
        assert np.array_equal(bits(tr.baked_render_subframe(sparse, SID, rgb_scale=SCALE).cpu().numpy()), bits(want))
        assert np.array_equal(bits(sparse.table()), bits(state[0])) and np.array_equal(bits(sparse.m2()), bits(state[1]))
        assert np.array_equal(sparse.counts(), state[2]) and sparse.adaptive_info()["paths"] == state[3]

    def desc(grid=(2, 2, 2), nphi=4, nc=2, abi=_lib.CT_ABI_VERSION):
        return _lib.CtBakeDesc(abi, (C.c_uint32 * 3)(*grid), nphi, nc)

    def message(handle=h):
        return L.ct_last_error(handle).decode()

    def create(handle, d, kind, p):
        out = C.c_void_p(1)
        rc = L.ct_bake_traced_adaptive(handle, C.byref(d) if d is not None else None, kind, C.byref(p) if p is not None else None, C.byref(out))
        assert not out.value or rc == _lib.CT_OK
        return rc

    # ct_bake_traced's errors, then the parameters
    for kind, dkw, pkw, word in ((3, {}, {}, "kind"), (1, dict(abi=_lib.CT_ABI_VERSION + 1), {}, "abi_version"), (2, dict(grid=(1, 2, 2)), {}, "grid[0]"),
                                 (0, dict(nphi=6), {}, "azimuths"), (0, dict(nc=65), {}, "cosines"),
                                 (0, dict(grid=(256, 256, 256), nphi=64, nc=64), {}, "2^26"),
                                 (1, {}, dict(abi=_lib.CT_ABI_VERSION + 1), "abi_version"), (1, {}, dict(round_samples=0, max_samples=0), "round_samples"),
                                 (1, {}, dict(round_samples=65536, max_samples=65536), "round_samples"), (1, {}, dict(max_samples=34), "max_samples"),
                                 (1, {}, dict(max_samples=0), "max_samples"), (1, {}, dict(max_samples=2 ** 24 + 4), "2^24"),
                                 (1, {}, dict(rel_tol=-1.0), "rel_tol"), (1, {}, dict(abs_tol=float("nan")), "abs_tol"),
                                 (1, {}, dict(rel_tol=float("inf")), "rel_tol"), (1, {}, dict(abs_tol=-0.5), "abs_tol")):
        assert create(h, desc(**dkw), kind, cparams(**pkw)) == _lib.CT_E_INVAL, (kind, dkw, pkw)
        assert word in message() and "ct_bake_traced_adaptive" in message(), (word, message())
    d, p, out = desc(), cparams(), C.c_void_p()
    assert L.ct_bake_traced_adaptive(h, None, 0, C.byref(p), C.byref(out)) == _lib.CT_E_INVAL
    assert L.ct_bake_traced_adaptive(h, C.byref(d), 0, None, C.byref(out)) == _lib.CT_E_INVAL and "parameters" in message()
    assert L.ct_bake_traced_adaptive(h, C.byref(d), 0, C.byref(p), None) == _lib.CT_E_INVAL
    unchanged()
    # a grid error comes before a parameter error, as the order of ct_bake_traced's checks has it
    assert create(h, desc(nphi=6), 0, cparams(max_samples=34)) == _lib.CT_E_INVAL and "azimuths" in message()
    # downloads take exactly the stored entries
    words = np.empty(ENTRIES + 1, np.uint32)
    for entry in (L.ct_bake_download_counts, L.ct_bake_download_m2):
        for count in (0, ENTRIES - 1, ENTRIES + 1, ACTIVE):
            assert entry(sparse.b, words.ctypes.data_as(C.c_void_p), count) == _lib.CT_E_INVAL
        assert entry(sparse.b, None, ENTRIES) == _lib.CT_E_INVAL
        assert entry(scene["compact"].b, words.ctypes.data_as(C.c_void_p), ENTRIES) == _lib.CT_E_INVAL   # a compact bake stores 315 blocks
    assert L.ct_bake_adaptive_info(sparse.b, None) == _lib.CT_E_INVAL
    assert L.ct_bake_trace_adaptive_more(h, None, 64) == _lib.CT_E_INVAL and L.ct_bake_retrace_adaptive(h, None) == _lib.CT_E_INVAL
    unchanged()
    # the uniform calls refuse an adaptive bake and name the adaptive ones; the adaptive calls refuse every other bake
    assert _code(sparse.trace_more, 4) == _lib.CT_E_INVAL and "ct_bake_trace_adaptive_more" in message()
    assert _code(sparse.retrace, 4) == _lib.CT_E_INVAL and "ct_bake_retrace_adaptive" in message()
    from test_network_render import SMALL, weights
    with N.Network(tr, weights(SMALL), 32, 1, 1) as net, tr.network_bake(net, (3, 3, 3), 4, 2) as netbake, tr.traced_bake((3, 3, 3), 4, 2, 2) as uniform:
        assert L.ct_bake_update(h, net.n, sparse.b) == _lib.CT_E_INVAL and "ct_bake_retrace_adaptive" in message()
        for other in (netbake, uniform):
            assert _code(other.trace_adaptive_more, 64) == _lib.CT_E_INVAL and "ct_bake_traced_adaptive" in message()
            assert _code(other.retrace_adaptive) == _lib.CT_E_INVAL
            assert _code(other.counts) == _lib.CT_E_INVAL and _code(other.m2) == _lib.CT_E_INVAL
            assert other.adaptive_info() == {k: 0 for k in other.adaptive_info()} and not other.adaptive_info()["adaptive"]
        uniform.trace_more(1)                                             # ... and are what they were
        assert uniform.trace_info()["samples"] == 3
    unchanged()
    # a bake of another handle, a simple-kernel handle
    with tracer() as other, tracer(flags=_lib.CT_FLAG_SIMPLE_KERNEL) as simple:
        assert L.ct_bake_trace_adaptive_more(other.h, sparse.b, 64) == _lib.CT_E_INVAL and "another handle" in message(other.h)
        assert L.ct_bake_retrace_adaptive(other.h, sparse.b) == _lib.CT_E_INVAL and "another handle" in message(other.h)
        assert create(simple.h, desc(), 0, cparams()) == _lib.CT_E_INVAL and "persistent kernel" in message(simple.h)
        assert create(simple.h, desc(), 0, cparams(max_samples=34)) == _lib.CT_E_INVAL and "max_samples" in message(simple.h)
    unchanged()
    # an empty volume: no active node, no round, nothing launched
    counters = tr.counters()
    with ds.CloudTracer(np.zeros((20, 33, 45), np.uint8), width=W, height=H) as empty, empty.traced_bake_adaptive((6, 5, 4), 4, 2, **P, sparse=True) as bake:
        info = bake.adaptive_info()
        assert info["adaptive"] and (info["rounds"], info["entries_active"], info["converged"], info["capped"], info["paths"]) == (0, 0, 0, 0, 0)
        assert not bits(bake.table()).any() and not bake.counts().any()
        bake.trace_adaptive_more(64)
        assert bake.adaptive_info()["max_samples"] == 64 and bake.adaptive_info()["rounds"] == 0
    assert tr.counters() == counters
    unchanged()


@pytest.mark.gpu
def test_cli_renders_from_an_adaptive_bake(tmp_path):
    from deepestscatter_amd import build, exr
    cli = build.build_cli()
    with ds.CloudTracer(cloud(), width=W, height=H, light_direction=ds.LIGHT_DIRECTIONS["Back"]) as tr, \
            tr.traced_bake_adaptive(*GRID, **P, compact=True) as bake:
        tr.baked_render_accumulate(bake, 1, 4, rgb_scale=SCALE, direct=True)
        want = tr.mean()[..., :3]
        info = bake.adaptive_info()
    common = [str(cli), "procedural:64", "--size", f"{W}x{H}", "--spp", "4", "--net-scale", "0.5,2,3", "--light", "Back", "--traced-bake", "9,8,7,8,3",
              "--net-direct", "--net-bake-compact"]
    r = subprocess.run(common + ["--bake-adaptive", "4,32,0.5,1e-4,7", "--out", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert np.array_equal(bits(exr.read_exr(tmp_path / "procedural_64.Back.PT.exr")), bits(want)) and want.any()
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("adaptive bake:")]
    assert len(line) == 1 and f"{info['rounds']} rounds of 4, cap 32" in line[0]
    assert f"{info['entries_active']} entries, {info['converged']} converged, {info['capped']} capped, {info['paths']} paths" in line[0]
    r = subprocess.run(common + ["--bake-adaptive", "4,32", "--bake-samples", "4", "--out", str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--bake-adaptive" in r.stdout + r.stderr and "--bake-samples" in r.stdout + r.stderr
    r = subprocess.run(common[:-4] + ["--bake-adaptive", "4,32", "--out", str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--traced-bake" in r.stdout + r.stderr
