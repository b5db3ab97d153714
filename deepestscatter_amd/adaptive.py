"""The adaptive frame (include/cloudtrace.h, "the adaptive frame"; ct_adaptive_frame_*): the progressive image rendered in rounds
that go only to the pixels which have not yet passed Camera::isConverged's test (Camera.cpp:232-268), and the numpy references
of its rule and of its loop.

This is plumbing only -- every sample comes from libcloudtrace.so (HIP kernels).
"""
from __future__ import annotations

import ctypes as C
from typing import Callable

import numpy as np

from . import _lib
from ._lib import CT_ADAPTIVE_COUNTS, CT_ADAPTIVE_M2, CT_ADAPTIVE_MEAN

FLT_EPSILON = np.float32(1.1920929e-07)


def pixel_converged_reference(mean_x, m2_x, count: int, rel_tol: float, abs_tol: float) -> np.ndarray:
    """Camera::isConverged's test of one channel at `count` samples, per pixel, in float32 with IEEE division and square root:
    sigma = sqrt(m2 / N), abs = 1.96f * sigma / sqrt(N), rel = abs / (mean + FLT_EPSILON), converged = rel < rel_tol or
    abs < abs_tol (a NaN compares false).  -> bool array of mean_x's shape."""
    mean_x, m2_x = np.asarray(mean_x, np.float32), np.asarray(m2_x, np.float32)
    n = np.float32(count)
    with np.errstate(all="ignore"):
        sigma = np.sqrt(m2_x / n, dtype=np.float32)
        abs_ci = np.float32(1.96) * sigma / np.sqrt(n, dtype=np.float32)
        rel_ci = abs_ci / (mean_x + FLT_EPSILON)
        return (rel_ci < np.float32(rel_tol)) | (abs_ci < np.float32(abs_tol))


def check_params(round_samples: int, max_samples: int, min_samples: int, rel_tol: float, abs_tol: float,
                 chunk_pixels: int = 0, pass_subframes: int = 0) -> None:
    """The ranges of CtAdaptiveFrameDesc; ValueError names the first that is violated."""
    r = int(round_samples)
    if not 1 <= r <= 0xFFFF:
        raise ValueError(f"round_samples {round_samples}: 1 .. 65535")
    if not (r <= max_samples <= 1 << 24 and max_samples % r == 0):
        raise ValueError(f"max_samples {max_samples}: a multiple of round_samples ({r}), at most 2^24")
    if not (r <= min_samples <= max_samples and min_samples % r == 0):
        raise ValueError(f"min_samples {min_samples}: a multiple of round_samples ({r}), at most max_samples ({max_samples})")
    for name, v in (("rel_tol", rel_tol), ("abs_tol", abs_tol)):
        if not (np.isfinite(v) and v >= 0):
            raise ValueError(f"{name} {v}: finite and not negative")
    if chunk_pixels < 0 or chunk_pixels % 64:
        raise ValueError(f"chunk_pixels {chunk_pixels}: 0 or a multiple of 64")
    if not 0 <= pass_subframes <= r:
        raise ValueError(f"pass_subframes {pass_subframes}: 0 or 1 .. round_samples ({r})")


def shard_pixels_reference(width: int, height: int, shard_index: int, shard_count: int) -> np.ndarray:
    """The first live list of ct_adaptive_frame_create_shard, stated from the tile rule: the pixels p = y * width + x whose 8 x 8
    tile (x // 8, y // 8) belongs to the shard -- (tx + 3 * ty) % shard_count == shard_index, every tile with one shard -- in
    ascending p (int64)."""
    if not 0 <= shard_index < max(shard_count, 1):
        raise ValueError(f"shard_index {shard_index}: 0 .. shard_count - 1 ({shard_count})")
    p = np.arange(width * height, dtype=np.int64)
    tx, ty = (p % width) // 8, (p // width) // 8
    owner = (tx + 3 * ty) % shard_count if shard_count > 1 else np.zeros_like(p)
    return p[owner == shard_index]


def merge_reference(shards) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """ct_group_adaptive_frame_merge on the host: `shards` is a list of (mean, m2, counts), one per shard, zero bits outside the
    shard's own pixels; every 32-bit word of the result is the unsigned maximum of the shards' words, so each pixel keeps the
    bits of the one shard that holds it.  -> (mean, m2, counts) with the first shard's shapes and dtypes."""
    shards = [tuple(np.ascontiguousarray(a) for a in s) for s in shards]
    out = []
    for k, first in enumerate(shards[0]):
        words = first.view(np.uint32).copy()
        for s in shards[1:]:
            np.maximum(words, s[k].view(np.uint32), out=words)
        out.append(words.view(first.dtype).reshape(first.shape))
    return tuple(out)


def adaptive_frame_reference(snapshot: Callable[[int], tuple[np.ndarray, np.ndarray]], width: int, height: int, *, round_samples: int,
                             max_samples: int, min_samples: int, rel_tol: float, abs_tol: float, rounds: int = 0, pixels=None):
    """The adaptive frame's loop over uniform images: snapshot(c) -> (mean, m2), float32 [H, W, 4], of the whole frame after the
    subframes 1 .. c (called with ascending c, once per round).  A live pixel takes its (mean, m2) from the snapshot of its
    count; one that has left keeps what it had.  rounds: stop after that many (0: until nothing is live).  pixels: the ascending
    pixels that start live (a shard's, shard_pixels_reference; the others stay zero); None: the whole frame.
    -> (mean [H, W, 4], m2 [H, W, 4], counts uint32 [H, W], history [(live pixels of the round, pixels that left the list behind
    it: converged, or all of them at max_samples), ..], capped: the ascending pixels that failed the rule at max_samples)."""
    check_params(round_samples, max_samples, min_samples, rel_tol, abs_tol)
    n = width * height
    mean, m2 = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
    counts = np.zeros(n, np.uint32)
    live = np.arange(n) if pixels is None else np.asarray(pixels, np.int64).reshape(-1)
    capped = np.zeros(0, np.int64)
    history, c = [], 0
    while len(live) and c < max_samples and (rounds == 0 or len(history) < rounds):
        c += round_samples
        s_mean, s_m2 = (np.asarray(v, np.float32).reshape(n, 4) for v in snapshot(c))
        mean[live], m2[live], counts[live] = s_mean[live], s_m2[live], c
        goes_on = np.ones(len(live), bool)
        if c >= min_samples:
            goes_on = ~pixel_converged_reference(mean[live, 0], m2[live, 0], c, rel_tol, abs_tol)
        survivors = live[goes_on]
        if c >= max_samples:   # at the cap every pixel leaves the list; those that fail the rule are the capped ones
            capped, survivors = survivors, survivors[:0]
        history.append((len(live), len(live) - len(survivors)))
        live = survivors
    return mean.reshape(height, width, 4), m2.reshape(height, width, 4), counts.reshape(height, width), history, capped


class AdaptiveFrame:
    """A CtAdaptiveFrame on a CloudTracer, for the pose and light the tracer has now.  update() renders rounds of round_samples
    subframes for the live pixels; mean(), m2() and counts() download the state; raise_cap() lets the capped pixels go on.
    Close it (or leave its `with` block) before the tracer."""

    def __init__(self, tracer, round_samples: int = 10, max_samples: int = 1000, min_samples: int = 100, rel_tol: float = 2e-2,
                 abs_tol: float = 1e-2, chunk_pixels: int = 0, pass_subframes: int = 0, shard: bool = False):
        check_params(round_samples, max_samples, min_samples, rel_tol, abs_tol, chunk_pixels, pass_subframes)
        self.L, self.tracer = tracer.L, tracer
        self.width, self.height = tracer.width, tracer.height
        desc = _lib.CtAdaptiveFrameDesc(_lib.CT_ABI_VERSION, round_samples, min_samples, max_samples, rel_tol, abs_tol, chunk_pixels,
                                        pass_subframes)
        f = C.c_void_p()
        # shard: ct_adaptive_frame_create_shard -- the tracer's own pixels (its shard_index of shard_count), zero bits elsewhere
        create = self.L.ct_adaptive_frame_create_shard if shard else self.L.ct_adaptive_frame_create
        _lib.check(create(tracer.h, C.byref(desc), C.byref(f)), tracer.h)
        self.f = f

    def close(self):
        if getattr(self, "f", None):
            if getattr(self, "_owned", True):   # (a GroupAdaptiveFrame's shard belongs to the group frame)
                self.L.ct_adaptive_frame_destroy(self.f)
            self.f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def update(self, rounds: int = 0) -> dict:
        """ct_adaptive_frame_update: at most `rounds` rounds, 0 = until nothing is live.  -> info()."""
        _lib.check(self.L.ct_adaptive_frame_update(self.f, rounds), self.tracer.h)
        return self.info()

    def raise_cap(self, max_samples: int) -> None:
        """ct_adaptive_frame_raise_cap: a higher multiple of round_samples; the capped pixels go live again."""
        _lib.check(self.L.ct_adaptive_frame_raise_cap(self.f, max_samples), self.tracer.h)

    def info(self) -> dict:
        """ct_adaptive_frame_info: width, height, round_samples, min_samples, max_samples, rounds, rel_tol, abs_tol, pixels, live,
        converged, capped, paths and the GPU milliseconds of the last update call (trace_ms, fold_ms, test_ms)."""
        i = _lib.CtAdaptiveFrameInfo()
        _lib.check(self.L.ct_adaptive_frame_info(self.f, C.byref(i)), self.tracer.h)
        return i.as_dict()

    def _download(self, which: int, out: np.ndarray) -> np.ndarray:
        _lib.check(self.L.ct_adaptive_frame_download(self.f, which, out.ctypes.data_as(C.c_void_p), out.nbytes), self.tracer.h)
        return out

    def mean(self) -> np.ndarray:
        return self._download(CT_ADAPTIVE_MEAN, np.empty((self.height, self.width, 4), np.float32))

    def m2(self) -> np.ndarray:
        return self._download(CT_ADAPTIVE_M2, np.empty((self.height, self.width, 4), np.float32))

    def counts(self) -> np.ndarray:
        return self._download(CT_ADAPTIVE_COUNTS, np.empty((self.height, self.width), np.uint32))

    def device_ptr(self, which: int = CT_ADAPTIVE_MEAN) -> int:
        p = C.c_void_p()
        _lib.check(self.L.ct_adaptive_frame_device_ptr(self.f, which, C.byref(p)), self.tracer.h)
        return int(p.value)

    def tonemap(self, exposure: float = 0.4):
        """ct_tonemap_buffer on the adaptive mean -> (uint8 [H, W, 4] screen, average luminance)."""
        return self.tracer.tonemap_buffer(self.device_ptr(CT_ADAPTIVE_MEAN), exposure)


class GroupAdaptiveFrame:
    """A CtGroupAdaptiveFrame on a TracerGroup (ct_group_adaptive_frame_*): one shard frame per handle of the group, each running
    its own rounds over its own pixels; mean(), m2(), counts() and device_ptr() give the merged arrays on the group's first
    device, bit for bit what one AdaptiveFrame on an unsharded tracer holds after the same calls.  Close it before the group."""

    def __init__(self, group, round_samples: int = 10, max_samples: int = 1000, min_samples: int = 100, rel_tol: float = 2e-2,
                 abs_tol: float = 1e-2, chunk_pixels: int = 0, pass_subframes: int = 0):
        check_params(round_samples, max_samples, min_samples, rel_tol, abs_tol, chunk_pixels, pass_subframes)
        self.L, self.group = group.L, group
        self.width, self.height = group.width, group.height
        desc = _lib.CtAdaptiveFrameDesc(_lib.CT_ABI_VERSION, round_samples, min_samples, max_samples, rel_tol, abs_tol, chunk_pixels,
                                        pass_subframes)
        gf = C.c_void_p()
        group._check(self.L.ct_group_adaptive_frame_create(group.g, C.byref(desc), C.byref(gf)))
        self.gf = gf
        group.__dict__.setdefault("_adaptive_frames", []).append(self)

    def close(self):
        if getattr(self, "gf", None):
            self.L.ct_group_adaptive_frame_destroy(self.gf)
            self.gf = None
            if self in getattr(self.group, "_adaptive_frames", []):
                self.group._adaptive_frames.remove(self)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def update(self, rounds: int = 0) -> dict:
        """ct_group_adaptive_frame_update: at most `rounds` rounds on every shard, 0 = until nothing is live.  -> info()."""
        self.group._check(self.L.ct_group_adaptive_frame_update(self.gf, rounds))
        return self.info()

    def raise_cap(self, max_samples: int) -> None:
        self.group._check(self.L.ct_group_adaptive_frame_raise_cap(self.gf, max_samples))

    def info(self) -> dict:
        """ct_group_adaptive_frame_info: AdaptiveFrame.info's fields for the whole frame -- sums over the shards; rounds and the
        three times are the largest."""
        i = _lib.CtAdaptiveFrameInfo()
        self.group._check(self.L.ct_group_adaptive_frame_info(self.gf, C.byref(i)))
        return i.as_dict()

    def shard(self, index: int) -> "AdaptiveFrame":
        """Shard `index`'s frame as an AdaptiveFrame that does not own it: info, downloads and device_ptr of that shard alone."""
        f, h = C.c_void_p(), C.c_void_p()
        self.group._check(self.L.ct_group_adaptive_frame_shard(self.gf, index, C.byref(f)))
        self.group._check(self.L.ct_group_handle(self.group.g, index, C.byref(h)))
        view = AdaptiveFrame.__new__(AdaptiveFrame)
        view.L, view.width, view.height = self.L, self.width, self.height
        view.tracer = _ShardHandle(h)
        view.f, view._owned = f, False
        return view

    def merge(self) -> None:
        self.group._check(self.L.ct_group_adaptive_frame_merge(self.gf))

    def _download(self, which: int, out: np.ndarray) -> np.ndarray:
        self.group._check(self.L.ct_group_adaptive_frame_download(self.gf, which, out.ctypes.data_as(C.c_void_p), out.nbytes))
        return out

    def mean(self) -> np.ndarray:
        return self._download(CT_ADAPTIVE_MEAN, np.empty((self.height, self.width, 4), np.float32))

    def m2(self) -> np.ndarray:
        return self._download(CT_ADAPTIVE_M2, np.empty((self.height, self.width, 4), np.float32))

    def counts(self) -> np.ndarray:
        return self._download(CT_ADAPTIVE_COUNTS, np.empty((self.height, self.width), np.uint32))

    def device_ptr(self, which: int = CT_ADAPTIVE_MEAN) -> int:
        p = C.c_void_p()
        self.group._check(self.L.ct_group_adaptive_frame_device_ptr(self.gf, which, C.byref(p)))
        return int(p.value)

    def tonemap(self, exposure: float = 0.4):
        """ct_tonemap_buffer of the merged mean on the group's first handle -> (uint8 [H, W, 4] screen, average luminance)."""
        h = C.c_void_p()
        self.group._check(self.L.ct_group_handle(self.group.g, 0, C.byref(h)))
        screen = np.empty((self.height, self.width, 4), np.uint8)
        avg = C.c_float(0)
        _lib.check(self.L.ct_tonemap_buffer(h, C.c_void_p(self.device_ptr(CT_ADAPTIVE_MEAN)), exposure, screen.ctypes.data_as(C.c_void_p),
                                            C.byref(avg)), h)
        return screen, float(avg.value)


class _ShardHandle:
    """What AdaptiveFrame needs of a tracer, for a handle the group owns."""

    def __init__(self, h):
        self.h = h
