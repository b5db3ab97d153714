"""ct_collector_*: RadianceCollector's loop on the device (include/cloudtrace.h, "the radiance collector on the device"; DESIGN.md
8(f) f-15).

Everything is held bit for bit (tobytes()) to collector.collect_reference -- the host loop with its constants as parameters --
over the CPU oracle (the CPU tests) or over ct_point_radiance_launch on a second handle of the same scene (the GPU tests).

Scene: conftest.sphere_volume(32, seed=12), an 8 x 8 frame, mode 1 unless said otherwise.  Parameter sets (histories as the
reference loop gives them on the oracle with fast=True):
  A  40 tasks, T = 4096, L = 3, rel 0.1, zero 1000, 16 updates: completes in update 15, r from 102 to 4096 (n r = 4080 is no
     multiple of 64, r >= 65 takes the merge kernel's second chunk, n == 1 occurs), the miss ray leaves by the zero rule in update 3
  B  150 tasks, T = 320, L = 4, rel 0.6, zero 20, 12 updates: 23 tasks live at the end, r from 2 to 11, tasks leave in every update
  C  as B with other tasks and rel 0.8: completes in update 9, r up to 160
  D  150 tasks, T = 200, L = 4, rel 0.5, zero 40, 8 updates: r == 1 throughout (the lane-per-task kernel), 121 live at the end"""
import ctypes as C
import subprocess

import numpy as np
import pytest

import _oracle as O
import deepestscatter_amd as ds
from deepestscatter_amd import _lib
from deepestscatter_amd import cloudtrace as ct
from deepestscatter_amd import collector as col
from conftest import sphere_volume

SETS = {
    "A": dict(count=40, seed=5, max_thread_count=4096, launches_per_update=3, rel_tol=0.1, abs_tol=1e-4, zero_samples=1000, updates=16),
    "B": dict(count=150, seed=5, max_thread_count=320, launches_per_update=4, rel_tol=0.6, abs_tol=1e-4, zero_samples=20, updates=12),
    "C": dict(count=150, seed=17, max_thread_count=320, launches_per_update=4, rel_tol=0.8, abs_tol=1e-4, zero_samples=20, updates=12),
    "D": dict(count=150, seed=5, max_thread_count=200, launches_per_update=4, rel_tol=0.5, abs_tol=1e-4, zero_samples=40, updates=8),
}
R_OF = {
    "A": [102, 102, 132, 186, 227, 292, 372, 409, 455, 512, 585, 1365, 2048, 4096, 4096],
    "B": [2, 2, 2, 3, 3, 4, 5, 6, 7, 8, 8, 11],
}


def sample_tasks(n, seed=0):
    rng = np.random.default_rng(seed)
    pos = (rng.random((n, 3), dtype=np.float32) - 0.5) * 0.5          # inside the cloud's box
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pos[0] = (3.0, 0.0, 0.0)
    d[0] = (1.0, 0.0, 0.0)                                              # a ray that misses the box
    pos[1] = (2.0, 0.1, 0.0)
    d[1] = (-2.0, 0.0, 0.0)                                             # enters from outside, unnormalised direction
    return pos, d


def volume():
    return sphere_volume(32, seed=12)


def tasks_of(name):
    return sample_tasks(SETS[name]["count"], seed=SETS[name]["seed"])


def params_of(name, **kw):
    p = {k: v for k, v in SETS[name].items() if k not in ("count", "seed")}
    p.update(kw)
    return p


def reference(launch, name, **kw):
    pos, d = tasks_of(name)
    return col.collect_reference(launch, pos, d, **params_of(name, **kw))


def check_history(name, history, converged_update):
    """The conditions the parameter sets were chosen for, on the REFERENCE's history: a device run is compared with it afterwards."""
    n, r, left = (list(v) for v in zip(*history))
    live_at_end = int((converged_update == 0).sum())
    assert n[0] == SETS[name]["count"] and all(a - b == c for a, b, c in zip(n, n[1:] + [live_at_end], left))
    if name == "A":
        assert r == R_OF["A"] and len(set(r)) >= 8 and max(r) >= 65 and 1 in n and live_at_end == 0 and len(history) == 15
        assert converged_update[0] == 3 and (n[0] * r[0]) % 64 != 0        # the miss ray: mean 0, 102 * 3 * 3 + 132 * 3 > 1000
    elif name == "B":
        assert r == R_OF["B"] and live_at_end == 23 and live_at_end >= 10 and sum(1 for c in left if c) >= 8 and all(left)
    elif name == "C":
        assert live_at_end == 0 and len(history) == 9 and max(r) == 160
    elif name == "D":
        assert all(v == 1 for v in r) and len(history) == 8 and live_at_end == 121


# ---------------------------------------------------------------------------------------------------- CPU
_ORACLE_RUNS = {}


def oracle_run(name):
    if name not in _ORACLE_RUNS:
        _ORACLE_RUNS[name] = reference(O.Oracle(volume(), 8, 8, mode=1, fast=True).point_radiance_launch, name)
    return _ORACLE_RUNS[name]


def test_symbols_resolve_and_answer_null_arguments(product_lib):
    L = product_lib
    for name in ("ct_collector_create", "ct_collector_update", "ct_collector_info", "ct_collector_download", "ct_collector_destroy"):
        assert hasattr(L, name) and name in _lib.EXPORTS
    d = _lib.CtCollectorDesc(_lib.CT_ABI_VERSION, 64, 1, 10, 0.1, 0.1)
    pos = np.zeros(3, np.float32)
    out = C.c_void_p()
    assert L.ct_collector_create(None, C.byref(d), pos.ctypes.data_as(C.c_void_p), pos.ctypes.data_as(C.c_void_p), 1, C.byref(out)) == _lib.CT_E_INVAL
    assert L.ct_collector_update(None, None, 1) == _lib.CT_E_INVAL
    assert L.ct_collector_info(None, None) == _lib.CT_E_INVAL
    assert L.ct_collector_download(None, None, None, 0) == _lib.CT_E_INVAL
    assert L.ct_collector_destroy(None) == _lib.CT_OK


def test_struct_layout_matches_the_header():
    import tempfile
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    desc = ["abi_version", "max_thread_count", "launches_per_update", "zero_samples", "rel_tol", "abs_tol"]
    info = ["batch", "remaining", "converged", "updates", "frame_id", "repeat_count", "threads", "completed", "paths", "trace_ms", "fold_ms", "test_ms"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "cloudtrace.h"\nint main(){printf("%zu %zu", sizeof(CtCollectorDesc), sizeof(CtCollectorInfo));'
           + "".join(f'printf(" %zu", offsetof(CtCollectorDesc, {f}));' for f in desc)
           + "".join(f'printf(" %zu", offsetof(CtCollectorInfo, {f}));' for f in info) + "return 0;}")
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "p.c").write_text(src)
        subprocess.run(["gcc", "-I", str(root / "include"), "-o", f"{d}/p", f"{d}/p.c"], check=True)
        out = [int(v) for v in subprocess.run([f"{d}/p"], capture_output=True, text=True, check=True).stdout.split()]
    assert out[:2] == [24, 64] == [C.sizeof(_lib.CtCollectorDesc), C.sizeof(_lib.CtCollectorInfo)]
    assert out[2:8] == [getattr(_lib.CtCollectorDesc, f).offset for f in desc] == [0, 4, 8, 12, 16, 20]
    assert out[8:] == [getattr(_lib.CtCollectorInfo, f).offset for f in info] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 56]


def test_collect_reference_is_the_collectors_loop():
    """collect_reference with the reference's constants against RadianceCollector driven update by update: set B's tasks,
    T = 320, L = 4, 6 updates."""
    pos, d = tasks_of("B")
    tex = volume()
    tasks, converged_update, history = col.collect_reference(O.Oracle(tex, 8, 8, mode=1, fast=True).point_radiance_launch, pos, d,
                                                             max_thread_count=320, launches_per_update=4, rel_tol=2e-2, abs_tol=1e-4,
                                                             zero_samples=100000, updates=6)
    c = col.RadianceCollector(O.Oracle(tex, 8, 8, mode=1, fast=True).point_radiance_launch, pos, d, max_thread_count=320, launches_per_update=4)
    want_history, want_update = [], np.zeros(150, np.uint32)
    for u in range(1, 7):
        n, r, before = c.get_remaining_count(), c.task_repeat_count, c.get_converged_count()
        c.update()
        want_history.append((n, r, c.get_converged_count() - before))
        for t in c.converged_tasks[before:]:
            want_update[t["id"]] = u
    assert history == want_history and c.frame_id == 24 and converged_update.tobytes() == want_update.tobytes()
    assert len(history) == 6 and c.get_converged_count() > 0 and not c.is_completed()
    done = {int(t["id"]): t for t in c.converged_tasks}
    live = {int(t["id"]): t for t in c.tasks_buffer[0::c.task_repeat_count]}
    assert sorted(list(done) + list(live)) == list(range(150))
    for i in range(150):
        assert tasks[i].tobytes() == (done[i] if i in done else live[i]).tobytes(), i
        assert (converged_update[i] != 0) == (i in done)
    assert tasks["position"].tobytes() == pos.tobytes() and tasks["direction"].tobytes() == d.tobytes()
    assert all(int(tasks[i]["experimentCount"]) == 4 * sum(r for _, r, _ in history) for i in live)


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_the_parameter_sets_have_the_histories_they_were_chosen_for(name):
    tasks, converged_update, history = oracle_run(name)
    check_history(name, history, converged_update)
    p = SETS[name]
    counts = tasks["experimentCount"].astype(np.int64)
    for i in range(p["count"]):                                           # a task's count: L * the r of the updates it was live in
        upto = int(converged_update[i]) or len(history)
        assert counts[i] == p["launches_per_update"] * sum(r for _, r, _ in history[:upto])


# ---------------------------------------------------------------------------------------------------- GPU
MARCH, DELTA = _lib.CT_EST_MARCH, _lib.CT_EST_DELTA
_GPU_RUNS = {}


def tracer(**kw):
    return ds.CloudTracer(volume(), **{**dict(width=8, height=8, mode=1), **kw})


def gpu_reference(name, **kw):
    """collect_reference over ct_point_radiance_launch on a handle of its own, once per (set, handle variant):
    -> (tasks, converged_update, history, that handle's counters)."""
    key = (name, tuple(sorted(kw.items())))
    if key not in _GPU_RUNS:
        with tracer(**kw) as tr:
            _GPU_RUNS[key] = reference(tr.point_radiance_launch, name) + (tr.counters(),)
    return _GPU_RUNS[key]


def assert_equals_reference(tr, c, name, ref, sets=SETS):
    tasks, converged_update, history, counters = ref
    p = sets[name]
    got_tasks, got_update = c.tasks()
    assert got_tasks.tobytes() == tasks.tobytes()
    assert got_update.tobytes() == converged_update.tobytes()
    live = int((converged_update == 0).sum())
    info = c.info()
    L, T = p["launches_per_update"], p["max_thread_count"]
    assert (info["batch"], info["remaining"], info["converged"], info["updates"]) == (p["count"], live, p["count"] - live, len(history))
    assert info["frame_id"] == L * len(history) and info["repeat_count"] == (T // live if live else 0)
    assert info["threads"] == live * info["repeat_count"] and info["completed"] == (live == 0)
    assert info["paths"] == sum(n * r * L for n, r, _ in history)
    assert tr.counters() == counters
    assert c.is_completed() == (live == 0) and c.get_remaining_count() == live and c.get_converged_count() == p["count"] - live


def device_run(tr, name, split=None, **kw):
    pos, d = tasks_of(name)
    p = params_of(name, **kw)
    updates = p.pop("updates")
    c = tr.radiance_collector(pos, d, **p)
    for k in split or [updates]:
        c.update(k)
    return c


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_device_collector_equals_the_host_loop(name):
    ref = gpu_reference(name)
    check_history(name, ref[2], ref[1])
    with tracer() as tr, device_run(tr, name) as c:
        assert_equals_reference(tr, c, name, ref)
        if name == "B":                                                   # the surface of RadianceCollector
            start = 4096
            want = [(start + i, col.encode_result(float(t["radiance"]), True)) for i, t in enumerate(ref[0]) if ref[1][i]]
            c.batch_start_id = start
            assert c.results() == want and len(want) == 127


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(estimator=DELTA), dict(flags=_lib.CT_FLAG_TEX_FIXED8), dict(mode=0)], ids=["delta", "fixed8", "mode0"])
def test_set_b_with_the_handles_estimator_flags_and_mode(kw):
    ref = gpu_reference("B", **kw)
    assert ref[2] and any(c for _, _, c in ref[2])                        # (other paths, other history: only that tasks leave)
    plain = gpu_reference("B")
    assert ref[0].tobytes() != plain[0].tobytes()
    with tracer(**kw) as tr, device_run(tr, "B") as c:
        assert_equals_reference(tr, c, "B", ref)


@pytest.mark.gpu
def test_the_split_over_calls_does_not_matter_and_a_completed_collector_stays():
    ref = gpu_reference("B")
    check_history("B", ref[2], ref[1])
    with tracer() as tr, device_run(tr, "B", split=[5, 7]) as c:
        assert_equals_reference(tr, c, "B", ref)
    ref = gpu_reference("A")
    check_history("A", ref[2], ref[1])
    with tracer() as tr, device_run(tr, "A", split=[100]) as c:           # stops at completion, in update 15
        assert_equals_reference(tr, c, "A", ref)
        assert c.is_completed() and c.info()["repeat_count"] == 0
        counters, launches = tr.counters(), tr.kernel_time()
        c.update()                                                        # CT_OK, nothing launched
        c.update(3)
        assert_equals_reference(tr, c, "A", ref)
        assert tr.counters() == counters and tr.kernel_time() == launches


@pytest.mark.gpu
def test_the_handles_image_is_left_alone():
    with tracer() as tr:
        eye = (2.5, -0.4, 0.0)
        tr.set_camera(eye, *ds.calculate_camera_variables(eye, (0, 0, 0), (0, 1, 0), 30.0, 1.0))
        tr.render_accumulate(1, 2)
        before = (tr.mean(), tr.m2(), tr.frame(), tr.subframes, tr.rendered_subframes())
        with device_run(tr, "D") as c:
            assert c.info()["updates"] == 8
            after = (tr.mean(), tr.m2(), tr.frame(), tr.subframes, tr.rendered_subframes())
        for x, y in zip(before[:3], after[:3]):
            assert x.tobytes() == y.tobytes()
        assert before[0].any() and before[3:] == after[3:] == (2, 2)
        tr.render_accumulate(3, 1)                                        # ... and the render goes on
        assert tr.subframes == 3


@pytest.mark.gpu
def test_after_set_light_update_is_a_state_error_and_download_still_works():
    with tracer() as tr, device_run(tr, "D", split=[2]) as c:
        tasks, converged_update = c.tasks()
        info = c.info()
        tr.set_light((0.3, -0.8, 0.2))
        with pytest.raises(_lib.CloudTraceError) as e:
            c.update()
        assert e.value.code == _lib.CT_E_STATE and "light" in e.value.message
        again, again_update = c.tasks()
        assert again.tobytes() == tasks.tobytes() and again_update.tobytes() == converged_update.tobytes()
        assert {k: v for k, v in c.info().items() if not k.endswith("_ms")} == {k: v for k, v in info.items() if not k.endswith("_ms")}


@pytest.mark.gpu
def test_every_allocation_is_given_back():
    start = ct.debug_allocations()
    with tracer() as tr:
        held = ct.debug_allocations()
        with device_run(tr, "D", split=[1]) as c:
            inside = ct.debug_allocations()
            assert inside["device_buffers"] >= held["device_buffers"] + 9   # positions, directions, three state arrays, converged_update, two lists, wave counts
            c.update(3)
            assert ct.debug_allocations()["device_buffers"] == inside["device_buffers"]   # (the point buffers hold 200 threads already)
    assert ct.debug_allocations() == start


@pytest.mark.gpu
def test_errors_leave_the_handle_and_the_collector_as_they_were():
    pos, d = tasks_of("D")
    with tracer() as tr, device_run(tr, "D", split=[2]) as c:
        L, h = tr.L, tr.h
        state = (c.tasks(), {k: v for k, v in c.info().items() if not k.endswith("_ms")}, tr.counters())

        def unchanged():
            now = c.tasks()
            assert now[0].tobytes() == state[0][0].tobytes() and now[1].tobytes() == state[0][1].tobytes()
            assert {k: v for k, v in c.info().items() if not k.endswith("_ms")} == state[1] and tr.counters() == state[2]

        def message(handle=h):
            return L.ct_last_error(handle).decode()

        def create(handle=h, abi=_lib.CT_ABI_VERSION, T=200, launches=4, zero=40, rel=0.5, abs_tol=1e-4, positions=pos, directions=d, count=150,
                   with_desc=True, with_out=True):
            desc = _lib.CtCollectorDesc(abi, T, launches, zero, rel, abs_tol)
            out = C.c_void_p(1)
            rc = L.ct_collector_create(handle, C.byref(desc) if with_desc else None,
                                       positions.ctypes.data_as(C.c_void_p) if positions is not None else None,
                                       directions.ctypes.data_as(C.c_void_p) if directions is not None else None, count,
                                       C.byref(out) if with_out else None)
            assert rc != _lib.CT_OK and (not with_out or not out.value or handle is None)
            return rc

        allocations = ct.debug_allocations()
        assert create(handle=None) == _lib.CT_E_INVAL
        for kw in (dict(with_desc=False), dict(positions=None), dict(directions=None), dict(with_out=False)):
            assert create(**kw) == _lib.CT_E_INVAL and "ct_collector_create" in message(), kw
        for kw, word in ((dict(abi=_lib.CT_ABI_VERSION + 1), "abi_version"), (dict(T=0), "max_thread_count"), (dict(T=2 ** 24 + 1), "max_thread_count"),
                         (dict(launches=0), "launches_per_update"), (dict(launches=65536), "launches_per_update"),
                         (dict(rel=-1.0), "rel_tol"), (dict(rel=float("inf")), "rel_tol"), (dict(abs_tol=float("nan")), "abs_tol"), (dict(abs_tol=-0.5), "abs_tol"),
                         (dict(count=0), "tasks"), (dict(T=149), "tasks"), (dict(T=2 ** 24, launches=257), "task-launches")):
            assert create(**kw) == _lib.CT_E_INVAL, kw
            assert word in message() and "ct_collector_create" in message(), (word, message())
        for index, column, value, word in ((7, "d", (0, 0, 0), "direction"), (149, "d", (1, float("nan"), 0), "direction"), (3, "d", (float("inf"), 0, 0), "direction"),
                                           (0, "p", (0, float("nan"), 0), "position"), (64, "p", (0, 0, float("-inf")), "position")):
            bad_pos, bad_d = pos.copy(), d.copy()
            (bad_d if column == "d" else bad_pos)[index] = value
            assert create(positions=bad_pos, directions=bad_d) == _lib.CT_E_INVAL
            assert f"task {index} " in message() and word in message(), message()
        with tracer(flags=_lib.CT_FLAG_SIMPLE_KERNEL) as simple, tracer() as other:
            assert create(handle=simple.h) == _lib.CT_E_INVAL and "persistent kernel" in message(simple.h)
            assert L.ct_collector_update(other.h, c.c, 1) == _lib.CT_E_INVAL and "another handle" in message(other.h)
        assert L.ct_collector_update(h, c.c, 0) == _lib.CT_E_INVAL and "at least one" in message()
        assert L.ct_collector_update(h, None, 1) == _lib.CT_E_INVAL and L.ct_collector_update(None, c.c, 1) == _lib.CT_E_INVAL
        assert L.ct_collector_info(c.c, None) == _lib.CT_E_INVAL
        tasks = np.zeros(151, ds.POINT_TASK_DTYPE)
        for count in (0, 149, 151):
            assert L.ct_collector_download(c.c, tasks.ctypes.data_as(C.c_void_p), None, count) == _lib.CT_E_INVAL and "150" in message()
        assert L.ct_collector_download(c.c, None, None, 150) == _lib.CT_E_INVAL
        assert L.ct_collector_download(c.c, tasks.ctypes.data_as(C.c_void_p), None, 150) == _lib.CT_OK   # converged_update may be NULL
        assert tasks[:150].tobytes() == state[0][0].tobytes()
        assert ct.debug_allocations() == allocations
        unchanged()
        c.update(6)                                                       # ... and the collector goes on to what set D gives
        assert_equals_reference(tr, c, "D", gpu_reference("D"))


def _cli_collect(tmp_path, tag, *extra):
    from deepestscatter_amd import build
    cli = build.build_cli()
    out = tmp_path / tag
    r = subprocess.run([str(cli), "collect", "procedural:48", "--batch", "96", "--scene-id", "3", "--light", "Back", "--out", str(out), *extra],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout, {t: col.read_flat_dataset(out / f"{t}.flat") for t in ("SceneSetup", "ScatterSample", "Result", "DisneyDescriptor")}


@pytest.mark.gpu
def test_cli_device_collector_writes_the_host_collectors_tables(tmp_path):
    """`cloudtrace collect` with the arguments of test_cpp_cli_collect_equals_the_python_pipeline, with and without
    --device-collector: identical tables; the same with two setups and --jobs 2."""
    host_out, host = _cli_collect(tmp_path, "host")
    dev_out, dev = _cli_collect(tmp_path, "device", "--device-collector")
    assert "Finished writing emissions." in dev_out and "converged: 96 of 96" in dev_out and "converged: 96 of 96" in host_out
    assert dev == host and len(dev["Result"][1]) == 96
    _, host2 = _cli_collect(tmp_path, "host2", "--scenes", "2", "--jobs", "2")
    dev2_out, dev2 = _cli_collect(tmp_path, "device2", "--scenes", "2", "--jobs", "2", "--device-collector")
    assert dev2 == host2 and len(dev2["Result"][1]) == 192 and '"jobs": 2' in dev2_out
