"""The adaptive frame (ct_adaptive_frame_*, its shard and group forms) and the device collector (ct_collector_*) at the sizes they
run at: the paths of their fold, scan and list kernels that the 24 x 16 frames and 150 tasks of tests/test_adaptive_frame.py,
tests/test_adaptive_frame_shards.py and tests/test_device_collector.py never enter.

  1  adaptive_fold_kernel's eight-wide unrolled loop and its subframe ids: round_samples 8, 11 and 19 on 24 x 16, whole and cut
     into passes of 9 and 8.  The uniform images are ct_render_subframe's frames folded on the host, not ct_render_accumulate's.
  2  adaptive_scan_kernel with several counts per thread (more than 1024 waves): 320 x 208 (1040 waves, two counts per thread,
     threads 520 .. 1023 own nothing) and 520 x 253 (2056 waves, three per thread, thread 685 owns one, the last wave has 40
     lanes); the same frame in chunks and passes; the cut of a round into passes by 2^24 results per launch.
  3  adaptive_own_count_kernel / adaptive_own_list_kernel behind that scan, and the group merge, on those frames.
  4  collect_scan_kernel with several counts per thread: 1300 and 2500 tasks with r > 1 (one count per task), 90000 tasks with
     r == 1 (one count per wave).

Every comparison is on the bits (tobytes()).  The references never come from the code under test: adaptive_frame_reference over
a second, unsharded handle of the same scene, collect_reference over ct_point_radiance_launch on a second handle; the CPU tests
run the same references over the CPU oracle.  The conditions a case was chosen for are asserted on the reference's history
before a device run is compared with it, so a case cannot pass by missing the path it was written for.

Scene: conftest.sphere_volume(32, seed=12), default camera and light.  Histories on the oracle with fast=True:
  fold, MARCH   R  8, cap 48: live 384, 135, 116, 100, 88, 76, 68 capped      DELTA   R 19: live 384, 124, 92, 76, 67 capped
                R 11, cap 66: live 384, 133, 111, 90, 74, 67, 60 capped
                R 19, cap 76: live 384, 132, 97, 78, 65 capped
  320 x 208, R 8, min 16, cap 40: (66560, 0), (66560, 42332), (24228, 3275), (20953, 2552), (18401, 18401), 16508 capped
  collector sets P, Q and S: HISTORY below"""
import numpy as np
import pytest

import _oracle as O
import test_adaptive_frame as TA
import test_adaptive_frame_shards as TS
import test_device_collector as TC
from deepestscatter_amd import _lib
from deepestscatter_amd.adaptive import adaptive_frame_reference, merge_reference, shard_pixels_reference
from deepestscatter_amd.collector import collect_reference
from test_adaptive_frame import Stepper, volume
from test_device_collector import sample_tasks

MARCH, DELTA = _lib.CT_EST_MARCH, _lib.CT_EST_DELTA
bits = TS.bits


def scan_shape(n):
    """adaptive_scan_kernel and collect_scan_kernel over n counts: (counts per thread, threads that own any, counts of the last of
    those)."""
    per = -(-n // 1024)
    owners = -(-n // per)
    return per, owners, n - (owners - 1) * per


def test_scan_shapes_of_the_cases():
    assert scan_shape(6) == (1, 6, 1) and scan_shape(1024) == (1, 1024, 1)    # what the small suites reach
    assert scan_shape(320 * 208 // 64) == (2, 520, 2)                         # threads 520 .. 1023 own nothing
    assert 520 * 253 % 64 == 40 and scan_shape(-(-520 * 253 // 64)) == (3, 686, 1)   # thread 685 owns one count
    assert scan_shape(1300) == (2, 650, 2) and scan_shape(2500) == (3, 834, 1) and scan_shape(-(-90000 // 64)) == (2, 704, 1)


# ==================================================================================================== 1: the unrolled fold
W, H = TA.W, TA.H
FOLD_CAP = {8: 48, 11: 66, 19: 76}
FOLD_PASSES = {(8, 0): [8], (11, 0): [11], (19, 0): [19], (19, 9): [9, 9, 1], (19, 8): [8, 8, 3]}   # (R, pass_subframes): a round's passes
FOLD_LOOPS = {(8, 0): [(1, 0)], (11, 0): [(1, 3)], (19, 0): [(2, 3)], (19, 9): [(1, 1), (1, 1), (0, 1)], (19, 8): [(1, 0), (1, 0), (0, 3)]}
FOLD_LIVE = {(MARCH, 8): ([384, 135, 116, 100, 88, 76], 68), (MARCH, 11): ([384, 133, 111, 90, 74, 67], 60),
             (MARCH, 19): ([384, 132, 97, 78], 65), (DELTA, 19): ([384, 124, 92, 76], 67)}


def fold_params(R, **kw):
    return dict(round_samples=R, min_samples=R, max_samples=FOLD_CAP[R], rel_tol=0.7, abs_tol=1e-2, **kw)


def host_fold(render):
    """(mean, M2) behind every subframe 1 .. 76 of the 24 x 16 frame: render(s) -> that subframe's frame, folded with the literal
    float32 Welford update of the oracle."""
    mean, m2 = np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32)
    states = {}
    for s in range(1, max(FOLD_CAP.values()) + 1):
        O.accumulate(render(s), mean, m2, s)
        states[s] = (mean.copy(), m2.copy())
    return states


def fold_reference(states, R):
    return adaptive_frame_reference(Stepper(lambda first, n: states[first + n - 1]), W, H, **fold_params(R))


def check_fold_history(R, ref):
    """Every round of the cap's worth runs, pixels leave in each, and behind the first no list is whole waves: the fold's last
    wave is partial and the unrolled loop runs on a list, not on the frame's own order."""
    mean, m2, counts, history, capped = ref
    live = [n for n, _ in history]
    assert live[0] == W * H and all(a - left == b for (a, left), b in zip(history, live[1:]))
    assert len(history) == FOLD_CAP[R] // R and all(left for _, left in history)
    assert all(n % 64 for n in live[1:]) and 0 < len(capped) < live[-1]
    assert counts.max() == FOLD_CAP[R] and counts.min() == R and counts.sum() == R * sum(live)


_ORACLE_FOLD = {}


def oracle_fold_states(estimator):
    if estimator not in _ORACLE_FOLD:
        _ORACLE_FOLD[estimator] = host_fold(O.Oracle(volume(), W, H, mode=0, fast=True, estimator=estimator).render_subframe)
    return _ORACLE_FOLD[estimator]


@pytest.mark.parametrize("estimator, R", list(FOLD_LIVE), ids=[f"{'md'[e == DELTA]}-{R}" for e, R in FOLD_LIVE])
def test_the_fold_cases_have_the_histories_they_were_chosen_for(estimator, R):
    ref = fold_reference(oracle_fold_states(estimator), R)
    check_fold_history(R, ref)
    assert ([n for n, _ in ref[3]], len(ref[4])) == FOLD_LIVE[(estimator, R)]


def test_the_fold_cases_run_the_unrolled_loop_and_its_tail():
    """Per pass (unrolled blocks of eight subframes, subframes of the tail loop), and the subframes done before it."""
    for (R, pass_subframes), passes in FOLD_PASSES.items():
        per_pass = pass_subframes or R
        assert passes == [min(per_pass, R - at) for at in range(0, R, per_pass)]
        assert [(p // 8, p % 8) for p in passes] == FOLD_LOOPS[(R, pass_subframes)]
    assert [sum(FOLD_PASSES[(19, 9)][:k]) for k in range(3)] == [0, 9, 18]


# ==================================================================================================== 2: more than 1024 waves
BIG = dict(round_samples=8, min_samples=16, max_samples=40, rel_tol=0.7, abs_tol=1e-2)
FRAMES = [(320, 208), (520, 253)]
FRAME_IDS = [f"{w}x{h}" for w, h in FRAMES]
HISTORY_320 = [(66560, 0), (66560, 42332), (24228, 3275), (20953, 2552), (18401, 18401)]
FIT = dict(round_samples=300, min_samples=300, max_samples=600, rel_tol=0.7, abs_tol=1e-2)
SILHOUETTE, SKY = (80, 40, 88, 48), (0, 0, 8, 8)


def check_big_history(w, h, ref):
    """Round 1 compacts the whole unlisted frame with every pixel surviving -- full counts through the scan with several counts
    per thread -- and round 2 a listed input of as many entries into a sparse, unaligned list: mixed counts."""
    mean, m2, counts, history, capped = ref
    live = [n for n, _ in history]
    assert all(a - left == b for (a, left), b in zip(history, live[1:]))
    assert live[0] == live[1] == w * h > 65536 and history[0][1] == 0 and scan_shape(-(-w * h // 64))[0] > 1
    assert 0.1 * w * h <= history[1][1] <= 0.9 * w * h
    assert len(live) == 5 and all(n % 64 for n in live[2:]) and 0 < len(capped) < live[-1]
    assert counts.sum() == 8 * sum(live)


def launches_of(history, R, chunk_pixels=0, pass_subframes=0):
    """The estimator launches ct_adaptive_frame_update makes for a history: per round its chunks times the passes of each, a pass
    holding at most 2^24 results (include/cloudtrace.h, "the adaptive frame")."""
    total = []
    for live, _ in history:
        chunk = min(live, chunk_pixels or 1 << 20)
        chunk = chunk & ~63 if chunk >= 64 else chunk
        count = 0
        for first in range(0, live, chunk):
            n_pad = (min(chunk, live - first) + 63) & ~63
            per_pass = min(pass_subframes or R, max(1, (1 << 24) // n_pad), 0xffff)
            count += -(-R // per_pass)
        total.append(count)
    return total


def test_launch_counts_of_the_cases():
    assert launches_of([(384, 0)] * 2, 4, 128, 3) == [6, 6]                                   # test_adaptive_frame's own case
    # (a list that is no multiple of 64 ends in a chunk of its own: the chunks before it are whole waves)
    assert launches_of(HISTORY_320, 8) == [1, 1, 2, 2, 2] and launches_of(HISTORY_320, 8, 16384, 5) == [10, 10, 4, 4, 4]
    assert launches_of([(384, 0), (135, 0)], 19, 0, 9) == [3, 6]
    assert (1 << 24) // 66560 == 252 and launches_of([(66560, 1), (55936, 1), (55872, 1)], 300) == [2, 2, 1]


# ==================================================================================================== 4: the collector's sets
SETS = {
    "P": dict(count=1300, seed=5, max_thread_count=2600, launches_per_update=3, rel_tol=0.6, abs_tol=1e-4, zero_samples=20, updates=6),
    "Q": dict(count=2500, seed=5, max_thread_count=20480, launches_per_update=3, rel_tol=0.35, abs_tol=1e-4, zero_samples=60, updates=8),
    "S": dict(count=90000, seed=5, max_thread_count=90000, launches_per_update=2, rel_tol=0.9, abs_tol=1e-4, zero_samples=3, updates=3),
}
HISTORY = {
    "P": [(1300, 2, 90), (1210, 2, 97), (1113, 2, 113), (1000, 2, 106), (894, 2, 86), (808, 3, 84)],
    "Q": [(2500, 8, 87), (2413, 8, 292), (2121, 9, 342), (1779, 11, 276), (1503, 13, 204), (1299, 15, 187), (1112, 18, 162), (950, 21, 125)],
    "S": [(90000, 1, 17080), (72920, 1, 15795), (57125, 1, 5161)],
}


def collect_params(name, **kw):
    p = {k: v for k, v in SETS[name].items() if k not in ("count", "seed")}
    p.update(kw)
    return p


def collect(launch, name, **kw):
    pos, d = sample_tasks(SETS[name]["count"], seed=SETS[name]["seed"])
    return collect_reference(launch, pos, d, **collect_params(name, **kw))


def scan_counts(history):
    """What collect_scan_kernel scans per update: one count per task (r > 1), or per wave of the lane-per-task kernel (r == 1)."""
    return [n if r > 1 else -(-n // 64) for n, r, _ in history]


def check_collect_history(name, history, converged_update, updates=None):
    n, r, left = (list(v) for v in zip(*history))
    live_at_end = int((converged_update == 0).sum())
    assert n[0] == SETS[name]["count"] and all(a - b == c for a, b, c in zip(n, n[1:] + [live_at_end], left))
    assert len(history) == (updates or SETS[name]["updates"]) and all(left) and live_at_end > 0
    big = [scan_shape(c)[0] for c in scan_counts(history)]
    if name == "P":
        assert sum(p > 1 for p in big) >= 2 and 1 in big and len(set(r)) > 1 and min(r) > 1
    elif name == "Q":
        assert sum(p > 1 for p in big) >= 5 and {2, 3} <= set(big) and len(set(r)) > 2 and min(r) > 1
    elif name == "S":
        assert sum(p > 1 for p in big) >= 2 and set(r) == {1} and 1 in big


@pytest.mark.parametrize("name, updates", [("P", 6), ("Q", 5)], ids=["P", "Q"])
def test_the_collector_sets_have_the_histories_they_were_chosen_for(name, updates):
    """(set Q in its first five updates: the other three are the GPU test's; set S takes too long on the CPU)"""
    tasks, converged_update, history = collect(O.Oracle(volume(), 8, 8, mode=1, fast=True).point_radiance_launch, name, updates=updates)
    check_collect_history(name, history, converged_update, updates)
    assert history == HISTORY[name][:updates]


def test_the_recorded_history_of_set_s_has_the_scan_counts_it_was_chosen_for():
    check_collect_history("S", HISTORY["S"], np.zeros(57125 - 5161, np.uint32))
    assert scan_counts(HISTORY["S"]) == [1407, 1140, 893] and [scan_shape(c)[0] for c in scan_counts(HISTORY["S"])] == [2, 2, 1]


# ==================================================================================================== GPU
tracer = TS.tracer


# ---------------------------------------------------------------------------------------------------- 1
_GPU_FOLD = {}


def gpu_fold_states(estimator):
    """host_fold over a handle of its own that is stepped with ct_render_subframe and downloaded after every subframe."""
    if estimator not in _GPU_FOLD:
        with tracer(W, H, estimator=estimator) as tr:
            def render(s):
                tr.render_subframe(s)
                return tr.frame()
            _GPU_FOLD[estimator] = host_fold(render)
    return _GPU_FOLD[estimator]


@pytest.mark.gpu
@pytest.mark.parametrize("estimator, R", list(FOLD_LIVE), ids=[f"{'md'[e == DELTA]}-{R}" for e, R in FOLD_LIVE])
def test_the_host_fold_of_subframes_is_render_accumulate(estimator, R):
    """... whose list kernel is unrolled like the adaptive fold: if this fails and the adaptive frame's test passes, it is
    accumulate_list_kernel that is wrong; the other way round, adaptive_fold_kernel."""
    mean, m2 = gpu_fold_states(estimator)[R]
    with tracer(W, H, estimator=estimator) as tr:
        tr.render_accumulate(1, R)
        assert bits(tr.mean()) == bits(mean) and bits(tr.m2()) == bits(m2) and mean[..., 0].any() and m2[..., 0].any()


@pytest.mark.gpu
@pytest.mark.parametrize("estimator, R, pass_subframes", [(MARCH, R, p) for R, p in FOLD_PASSES] + [(DELTA, R, p) for R, p in FOLD_PASSES if R == 19],
                         ids=[f"march-{R}-{p}" for R, p in FOLD_PASSES] + [f"delta-{R}-{p}" for R, p in FOLD_PASSES if R == 19])
def test_the_unrolled_fold_equals_the_host_fold_of_the_subframes(estimator, R, pass_subframes):
    ref = fold_reference(gpu_fold_states(estimator), R)
    check_fold_history(R, ref)
    with tracer(W, H, estimator=estimator) as tr:
        before, launches = tr.counters()["paths"], tr.kernel_time()[2]
        with tr.adaptive_frame(**fold_params(R, pass_subframes=pass_subframes)) as f:
            f.update()
            TA.assert_equals_reference(f, ref, cap=FOLD_CAP[R])
            assert tr.counters()["paths"] - before == int(ref[2].sum())
            assert tr.kernel_time()[2] - launches == sum(launches_of(ref[3], R, 0, pass_subframes))


# ---------------------------------------------------------------------------------------------------- 2
_UNIFORM = {}


def uniform_snapshots(w, h, R=8, cap=40):
    """A handle of its own stepped with ct_render_accumulate(first, R) and downloaded after every round, once per frame size:
    -> {count: (mean, m2)}."""
    key = (w, h, R, cap)
    if key not in _UNIFORM:
        with tracer(w, h) as tr:
            kept = {}
            for c in range(R, cap + 1, R):
                tr.render_accumulate(c - R + 1, R)
                kept[c] = (tr.mean(), tr.m2())
            assert tr.counters()["paths"] == cap * w * h
        _UNIFORM[key] = kept
    return _UNIFORM[key]


_REFERENCES = {}


def big_reference(w, h, pixels=None, key=None, params=BIG):
    """adaptive_frame_reference over uniform_snapshots, for the whole frame or a shard's own pixels (key: its (index, count))."""
    k = (w, h, key, params["round_samples"])
    if k not in _REFERENCES:
        kept = uniform_snapshots(w, h, params["round_samples"], params["max_samples"])
        _REFERENCES[k] = adaptive_frame_reference(Stepper(lambda first, n: kept[first + n - 1]), w, h, pixels=pixels, **params)
    return _REFERENCES[k]


@pytest.mark.gpu
@pytest.mark.parametrize("w, h", FRAMES, ids=FRAME_IDS)
def test_a_frame_of_more_than_1024_waves_equals_the_loop_over_uniform_images(w, h):
    ref = big_reference(w, h)
    check_big_history(w, h, ref)
    with tracer(w, h) as tr:
        before, launches = tr.counters()["paths"], tr.kernel_time()[2]
        with tr.adaptive_frame(**BIG) as f:
            f.update()
            TA.assert_equals_reference(f, ref, cap=40, W=w, H=h)
            assert tr.counters()["paths"] - before == int(ref[2].sum())
            assert tr.kernel_time()[2] - launches == sum(launches_of(ref[3], 8))
    with tracer(w, h) as tr, tr.adaptive_frame(**BIG) as f:                   # ... and stopped behind the sparse list's round
        f.update(2)
        f.update(1)
        TA.assert_equals_reference(f, big_reference(w, h, key="3 rounds", params=dict(BIG, rounds=3)), cap=40, W=w, H=h)


@pytest.mark.gpu
def test_the_uniform_handle_of_320_x_208_is_the_oracles_in_two_windows():
    """What holds the reference handle itself: 16 subframes of two 8 x 8 windows on the CPU oracle, one on the cloud's silhouette
    and one in the sky."""
    w, h = FRAMES[0]
    mean, m2 = uniform_snapshots(w, h)[16]
    orc = O.Oracle(volume(), w, h, mode=0, fast=True)
    lit = {}
    for window in (SILHOUETTE, SKY):
        x0, y0, x1, y1 = window
        want_mean, want_m2 = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
        for s in range(1, 17):
            O.accumulate(orc.render_subframe(s, window=window), want_mean, want_m2, s)
        assert bits(mean[y0:y1, x0:x1]) == bits(want_mean[y0:y1, x0:x1]) and bits(m2[y0:y1, x0:x1]) == bits(want_m2[y0:y1, x0:x1])
        lit[window] = int((want_mean[y0:y1, x0:x1, 0] != 0).sum())
    assert 0 < lit[SILHOUETTE] < 64 and lit[SKY] == 0


@pytest.mark.gpu
def test_chunks_and_passes_do_not_change_the_bits_of_320_x_208():
    """chunk_pixels 16384, pass_subframes 5: five chunks per early round, the last one partial, and passes of 5 and 3, so the wave
    counts are written by the second pass of every chunk."""
    w, h = FRAMES[0]
    ref = big_reference(w, h)
    check_big_history(w, h, ref)
    want = launches_of(ref[3], 8, 16384, 5)
    assert want[:2] == [10, 10] and w * h % 16384 != 0
    with tracer(w, h) as tr, tr.adaptive_frame(chunk_pixels=16384, pass_subframes=5, **BIG) as f:
        launches = tr.kernel_time()[2]
        f.update(1)
        assert tr.kernel_time()[2] - launches == 10
        f.update()
        TA.assert_equals_reference(f, ref, cap=40, W=w, H=h)
        assert tr.kernel_time()[2] - launches == sum(want)


@pytest.mark.gpu
def test_a_round_of_more_than_2_to_the_24_results_is_cut_into_passes():
    """320 x 208 with R = 300: 66560 * 300 results are more than a launch holds, 2^24 / 66560 = 252, so round 1 runs as passes of
    252 and 48 and its second pass folds from done = 252."""
    w, h = FRAMES[0]
    ref = big_reference(w, h, params=FIT)
    mean, m2, counts, history, capped = ref
    assert len(history) == 2 and history[0][0] == w * h and 0 < history[0][1] < w * h and history[1][0] % 64 and len(capped) > 0
    want = launches_of(history, 300)
    assert w * h * 300 > 1 << 24 and want[0] == 2
    with tracer(w, h) as tr, tr.adaptive_frame(**FIT) as f:
        before, launches = tr.counters()["paths"], tr.kernel_time()[2]
        f.update(1)
        assert tr.kernel_time()[2] - launches == 2
        f.update()
        TA.assert_equals_reference(f, ref, cap=600, W=w, H=h)
        assert tr.counters()["paths"] - before == int(counts.sum())
        assert tr.kernel_time()[2] - launches == sum(want)


# ---------------------------------------------------------------------------------------------------- 3
SHARDS = {(320, 208, 3): [23296, 21632, 21632], (520, 253, 5): [26312] * 5}
SHARD_IDS = [f"{w}x{h}-{n}" for w, h, n in SHARDS]
_SHARD_RUNS = {}


def shard_runs(w, h, n):
    """Every shard's frame from ct_adaptive_frame_create_shard on a sharded handle of its own, once per case: -> per shard the
    state behind update(1), the state behind update() and the handle's paths."""
    if (w, h, n) not in _SHARD_RUNS:
        out = []
        for i in range(n):
            with tracer(w, h, shard_index=i, shard_count=n) as tr:
                before = tr.counters()["paths"]
                with tr.adaptive_frame(shard=True, **BIG) as f:
                    f.update(1)
                    first = TS.state(f)
                    f.update()
                    last = TS.state(f)
                out.append((first, last, tr.counters()["paths"] - before))
        _SHARD_RUNS[(w, h, n)] = out
    return _SHARD_RUNS[(w, h, n)]


@pytest.mark.gpu
@pytest.mark.parametrize("w, h, n", list(SHARDS), ids=SHARD_IDS)
def test_the_first_live_list_of_a_large_shard_is_its_own_pixels(w, h, n):
    """Through update(1)'s counts, as tests/test_adaptive_frame_shards.py does: exactly the own pixels hold R."""
    assert [len(shard_pixels_reference(w, h, i, n)) for i in range(n)] == SHARDS[(w, h, n)] and sum(SHARDS[(w, h, n)]) == w * h
    for i, (s, _, _) in enumerate(shard_runs(w, h, n)):
        own = shard_pixels_reference(w, h, i, n)
        want = np.zeros(w * h, np.uint32)
        want[own] = 8
        assert bits(s[2]) == bits(want)
        assert not s[0].reshape(w * h, 4)[want == 0].view(np.uint32).any() and not s[1].reshape(w * h, 4)[want == 0].view(np.uint32).any()
        assert (s[3]["pixels"], s[3]["live"], s[3]["rounds"], s[3]["paths"]) == (len(own), len(own), 1, 8 * len(own))


@pytest.mark.gpu
@pytest.mark.parametrize("w, h, n", list(SHARDS), ids=SHARD_IDS)
def test_large_shard_frames_are_the_whole_frame_on_their_own_pixels(w, h, n):
    whole = big_reference(w, h)
    check_big_history(w, h, whole)
    runs = shard_runs(w, h, n)
    for i, (_, s, paths) in enumerate(runs):
        own = shard_pixels_reference(w, h, i, n)
        TS.assert_shard_of(s, whole, w, h, own)
        mean, m2, counts, history, capped = big_reference(w, h, own, (i, n))
        assert [bits(a) for a in s[:3]] == [bits(mean), bits(m2), bits(counts)]
        info = s[3]
        assert (info["width"], info["height"], info["pixels"], info["max_samples"], info["rounds"]) == (w, h, len(own), 40, len(history))
        assert (info["live"], info["capped"], info["converged"]) == (0, len(capped), len(own) - len(capped))
        assert paths == info["paths"] == int(counts.sum())
    total = {k: sum(s[3][k] for _, s, _ in runs) for k in ("pixels", "live", "converged", "capped", "paths")}
    assert total == dict(pixels=w * h, live=0, converged=w * h - len(whole[4]), capped=len(whole[4]), paths=int(whole[2].sum()))
    merged = merge_reference([s[:3] for _, s, _ in runs])
    assert [bits(a) for a in merged] == [bits(a) for a in whole[:3]]


@pytest.mark.gpu
@pytest.mark.parametrize("w, h, n", list(SHARDS), ids=SHARD_IDS)
def test_a_large_group_frame_merges_to_the_whole_frame(w, h, n):
    whole = big_reference(w, h)
    check_big_history(w, h, whole)
    with TS.group(w, h, n) as g, g.adaptive_frame(**BIG) as gf:
        gf.update(2)
        gf.update()
        got = TS.state(gf)
        assert [bits(a) for a in got[:3]] == [bits(a) for a in whole[:3]]
        info = got[3]
        assert (info["width"], info["height"], info["pixels"], info["rounds"], info["max_samples"]) == (w, h, w * h, 5, 40)
        assert (info["live"], info["capped"], info["converged"]) == (0, len(whole[4]), w * h - len(whole[4]))
        assert info["paths"] == int(whole[2].sum()) == g.counters()["paths"]
        shards = []
        for i in range(n):
            s = gf.shard(i)
            shards.append((s.mean(), s.m2(), s.counts()))
            TS.assert_shard_of(shards[-1], whole, w, h, shard_pixels_reference(w, h, i, n))
            assert s.info()["pixels"] == SHARDS[(w, h, n)][i]
        assert [bits(a) for a in merge_reference(shards)] == [bits(a) for a in got[:3]]


# ---------------------------------------------------------------------------------------------------- 4
_GPU_COLLECT = {}


def gpu_collect_reference(name):
    """collect_reference over ct_point_radiance_launch on a handle of its own, once per set: -> (tasks, converged_update, history,
    that handle's counters)."""
    if name not in _GPU_COLLECT:
        with TC.tracer() as tr:
            _GPU_COLLECT[name] = collect(tr.point_radiance_launch, name) + (tr.counters(),)
    return _GPU_COLLECT[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name, split", [("P", [6]), ("Q", [8]), ("Q", [3, 5]), ("S", [3])], ids=["P", "Q", "Q-split", "S"])
def test_a_collector_of_more_than_1024_scan_counts_equals_the_host_loop(name, split):
    ref = gpu_collect_reference(name)
    check_collect_history(name, ref[2], ref[1])
    pos, d = sample_tasks(SETS[name]["count"], seed=SETS[name]["seed"])
    p = collect_params(name)
    assert sum(split) == p.pop("updates")
    with TC.tracer() as tr, tr.radiance_collector(pos, d, **p) as c:
        for k in split:
            c.update(k)
        TC.assert_equals_reference(tr, c, name, ref, sets=SETS)
