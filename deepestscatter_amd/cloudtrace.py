"""Thin object wrapper over the C ABI (include/cloudtrace.h): one `CloudTracer` = one CtHandle.

This is plumbing only -- every numeric result comes from libcloudtrace.so (HIP kernels).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from pathlib import Path

import numpy as np

from . import _lib
from ._lib import (CT_BUF_DENSITY, CT_BUF_FRAME, CT_BUF_INSCATTER, CT_BUF_M2, CT_BUF_MEAN, CT_BUF_SCREEN,
                   CtCounters, CtFetchCounters, CtScene, check)

MIE_FILE = Path(__file__).resolve().parent / "data" / "mie_raw.f32"

# Tasks.cpp:52-65
LIGHT_DIRECTIONS = {
    "Front": (-0.586, -0.766, -0.271),
    "Side": (-0.03, -0.25, 0.8),
    "Back": (0.586, -0.766, -0.271),
}


def load_mie_raw() -> tuple[np.ndarray, np.ndarray]:
    """The two 4096-entry Lorenz-Mie tables (data of Mie.cpp:8-8203): (mie, choppedMie)."""
    raw = np.fromfile(MIE_FILE, dtype="<f4")
    if raw.size != 8192:
        raise RuntimeError(f"{MIE_FILE} is corrupt")
    return np.ascontiguousarray(raw[:4096]), np.ascontiguousarray(raw[4096:])


# Gpu::PointRadianceTask, PointRadianceTask.h:70-77 (40 bytes)
POINT_TASK_DTYPE = np.dtype([("id", "<i4"), ("experimentCount", "<u4"), ("radiance", "<f4"),
                             ("runningVariance", "<f4"), ("position", "<f4", 3), ("direction", "<f4", 3)])
assert POINT_TASK_DTYPE.itemsize == 40


def make_point_tasks(positions, directions, ids=None) -> np.ndarray:
    """PointRadianceTask(id, position, direction) x N (PointRadianceTask.h:15-18)."""
    positions = np.asarray(positions, np.float32).reshape(-1, 3)
    directions = np.asarray(directions, np.float32).reshape(-1, 3)
    t = np.zeros(len(positions), POINT_TASK_DTYPE)
    t["id"] = np.arange(len(positions)) if ids is None else ids
    t["position"] = positions
    t["direction"] = directions
    return t


def _p(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def calculate_camera_variables(eye, lookat, up, hfov_deg: float, aspect_ratio: float):
    """sutil::calculateCameraVariables(..., fov_is_vertical=false), sutil.cpp:501-524."""
    e, la, u = (np.asarray(v, np.float32) for v in (eye, lookat, up))
    U, V, W = (np.empty(3, np.float32) for _ in range(3))
    check(_lib.load().ct_calculate_camera_variables(_p(e), _p(la), _p(u), hfov_deg, aspect_ratio, _p(U), _p(V), _p(W)))
    return U, V, W


def quantize_volume(grid: np.ndarray) -> np.ndarray:
    """Resources::loadVolumeBuffer's quantiser (Resources.cpp:92-141): float [Z,Y,X] payload ->
    uint8 [Z+2,Y+2,X+2] texture with a zero border."""
    grid = np.ascontiguousarray(grid, np.float32)
    nz, ny, nx = grid.shape
    pd = np.array([nx, ny, nz], np.uint32)
    out = np.empty((nz + 2, ny + 2, nx + 2), np.uint8)
    check(_lib.load().ct_quantize_volume(_p(grid), _p(pd), _p(out)))
    return out


def load_vdb(path) -> np.ndarray:
    """Resources::loadVolumeBuffer for a .vdb file (Resources.cpp:82-143; ct_load_vdb): -> uint8 [Z,Y,X] texture."""
    L = _lib.load()
    dims = np.zeros(3, np.uint32)
    n = C.c_size_t(0)
    err = C.create_string_buffer(512)
    rc = L.ct_load_vdb(str(path).encode(), _p(dims), None, 0, C.byref(n), err, 512)
    if rc != _lib.CT_OK:
        raise _lib.CloudTraceError(rc, err.value.decode("utf-8", "replace"))
    out = np.empty((int(dims[2]), int(dims[1]), int(dims[0])), np.uint8)
    rc = L.ct_load_vdb(str(path).encode(), _p(dims), _p(out), out.nbytes, C.byref(n), err, 512)
    if rc != _lib.CT_OK:
        raise _lib.CloudTraceError(rc, err.value.decode("utf-8", "replace"))
    return out


def generate_mipmaps(level0: np.ndarray) -> list[np.ndarray]:
    """Resources::generateMipmaps (Resources.cpp:169-209): list of uint8 [z,y,x] levels."""
    level0 = np.ascontiguousarray(level0, np.uint8)
    nz, ny, nx = level0.shape
    dims = np.array([nx, ny, nz], np.uint32)
    L = _lib.load()
    levels, total = C.c_uint32(0), C.c_size_t(0)
    offs = (C.c_size_t * 32)()
    check(L.ct_generate_mipmaps(_p(level0), _p(dims), None, 0, C.byref(levels), C.byref(total), offs))
    buf = np.empty(total.value, np.uint8)
    check(L.ct_generate_mipmaps(_p(level0), _p(dims), _p(buf), buf.size, C.byref(levels), C.byref(total), offs))
    out = []
    for l in range(levels.value):
        shape = (max(nz >> l, 1), max(ny >> l, 1), max(nx >> l, 1))
        n = int(np.prod(shape))
        out.append(buf[offs[l]:offs[l] + n].reshape(shape).copy())
    return out


def make_procedural_cloud(n: int, seed: int = 0xC10D5EED) -> np.ndarray:
    """Synthetic benchmark cloud of SURVEY.md section 8(d): uint8 [n,n,n] texture."""
    out = np.empty((n, n, n), np.uint8)
    check(_lib.load().ct_make_procedural_cloud(n, seed & 0xFFFFFFFF, _p(out)))
    return out


def tile_owner(tx: int, ty: int, shard_count: int) -> int:
    return int(_lib.load().ct_tile_owner(tx, ty, shard_count))


def debug_allocations() -> dict:
    """ct_debug_allocations: the device and pinned host buffers the library holds in this process right now, and their bytes."""
    v = (C.c_uint64 * 4)()
    check(_lib.load().ct_debug_allocations(v))
    return dict(zip(("device_buffers", "device_bytes", "pinned_buffers", "pinned_bytes"), (int(x) for x in v)))


def shard_mask(width: int, height: int, shard_index: int, shard_count: int) -> np.ndarray:
    """bool [H, W]: pixels whose 8x8 tile belongs to `shard_index`."""
    ty, tx = np.meshgrid(np.arange(height) // 8, np.arange(width) // 8, indexing="ij")
    if shard_count <= 1:
        return np.ones((height, width), bool)
    return ((tx + 3 * ty) % shard_count) == shard_index


def shard_tiles(width: int, height: int, shard_index: int, shard_count: int) -> np.ndarray:
    """ct_shard_tiles: the shard's 8x8 tiles as ty * tiles_x + tx, ascending (uint32): the order the sharded network renderer
    takes them in."""
    L = _lib.load()
    n = C.c_uint32(0)
    rc = L.ct_shard_tiles(width, height, shard_index, shard_count, None, 0, C.byref(n))
    if rc != _lib.CT_OK:
        raise _lib.CloudTraceError(rc, "ct_shard_tiles: an empty frame, or a shard index that is not below the shard count")
    out = np.empty(n.value, np.uint32)
    rc = L.ct_shard_tiles(width, height, shard_index, shard_count, _p(out) if n.value else None, n.value, C.byref(n))
    if rc != _lib.CT_OK:
        raise _lib.CloudTraceError(rc, "ct_shard_tiles")
    return out


@dataclass
class SceneParams:
    """Defaults = the reference's hard-coded configuration (SURVEY.md section 5 'config')."""
    width: int = 512                       # Tasks.cpp:49
    height: int = 256                      # Tasks.cpp:50
    mode: int = 0                          # SunAndSkyAllScatter, Tasks.cpp:92
    estimator: int = 0
    cloud_size_m: float = 7000.0           # main.cpp:63
    mean_free_path_m: float = 10.0         # SceneDescription.h:80
    sample_step: float = 1.0 / 512.0       # installers.cpp:86
    max_depth: int = 2000                  # cloudRadianceMaterials.cu:4
    light_direction: tuple = LIGHT_DIRECTIONS["Side"]
    light_color: tuple = (1.0, 1.0, 1.0)   # installers.cpp:99
    light_intensity: float = 1e6           # installers.cpp:100
    device: int = 0
    shard_index: int = 0
    shard_count: int = 1
    flags: int = 0


def make_scene(density: np.ndarray, p: SceneParams):
    """-> (CtScene, objects that must stay alive until ct_create / ct_group_create has copied the host data)."""
    density = np.ascontiguousarray(density, np.uint8)
    if density.ndim != 3:
        raise ValueError("density must be uint8 [Z, Y, X]")
    mie, chopped = load_mie_raw()
    s = CtScene()
    s.abi_version = _lib.CT_ABI_VERSION
    nz, ny, nx = density.shape
    s.dims[:] = (nx, ny, nz)
    s.density_host = density.ctypes.data
    s.cloud_size_m = p.cloud_size_m
    s.mean_free_path_m = p.mean_free_path_m
    s.sample_step = p.sample_step
    s.mode = p.mode
    s.estimator = p.estimator
    s.max_depth = p.max_depth
    s.light_direction[:] = p.light_direction
    s.light_color[:] = p.light_color
    s.light_intensity = p.light_intensity
    s.width, s.height = p.width, p.height
    s.mie_host = mie.ctypes.data
    s.chopped_mie_host = chopped.ctypes.data
    s.mie_count = 4096
    s.device = p.device
    s.shard_index, s.shard_count = p.shard_index, p.shard_count
    s.flags = p.flags
    return s, (density, mie, chopped)


def _light_args(direction, color):
    """float32[3] arrays for ct_set_light; None stays None (the library answers a NULL direction itself)."""
    d = None if direction is None else np.ascontiguousarray(direction, np.float32).reshape(3)
    c = None if color is None else np.ascontiguousarray(color, np.float32).reshape(3)
    return d, c


class CloudTracer:
    """Owns one CtHandle.  `density` is the uint8 [Z,Y,X] texture incl. its zero border."""

    def __init__(self, density: np.ndarray, params: SceneParams | None = None, **kw):
        self.L = _lib.load()
        self.params = params or SceneParams(**kw)
        s, keep = make_scene(density, self.params)
        self.dims = tuple(int(v) for v in s.dims)
        self.width, self.height = self.params.width, self.params.height
        h = C.c_void_p()
        rc = self.L.ct_create(C.byref(s), C.byref(h))
        del keep
        check(rc, None)
        self.h = h
        self._light = tuple(float(v) for v in self.params.light_direction)   # as given; light_direction() normalises it

    # -- lifetime -----------------------------------------------------------------------------
    def close(self):
        if getattr(self, "h", None):
            self.L.ct_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- ARenderer verbs ------------------------------------------------------------------------
    def set_camera(self, eye, U, V, W):
        a = [np.asarray(v, np.float32) for v in (eye, U, V, W)]
        check(self.L.ct_set_camera(self.h, *[_p(v) for v in a]), self.h)

    def set_light(self, direction, color=None, intensity: float = 1e6):
        """ct_set_light: a new light on the live handle -- the shadow volume and what is built from it are redone, the
        density layouts, tables and buffers stay.  `color=None` keeps the colour.  The image is not cleared: reset() next."""
        d, c = _light_args(direction, color)
        check(self.L.ct_set_light(self.h, _p(d) if d is not None else None, _p(c) if c is not None else None, intensity), self.h)
        self._light = tuple(float(v) for v in d)

    def render_subframe(self, subframe_id: int, out_dev_ptr: int | None = None):
        check(self.L.ct_render_subframe(self.h, subframe_id, C.c_void_p(out_dev_ptr) if out_dev_ptr else None), self.h)

    def accumulate(self, subframe_id: int, frame_dev_ptr: int | None = None):
        check(self.L.ct_accumulate(self.h, subframe_id, C.c_void_p(frame_dev_ptr) if frame_dev_ptr else None), self.h)

    def render_accumulate(self, first_subframe_id: int, count: int):
        check(self.L.ct_render_accumulate(self.h, first_subframe_id, count), self.h)

    def render_accumulate_async(self, first_subframe_id: int, count: int):
        """Enqueue a batch and return (ct_render_accumulate_async): its paths may finish in later launches, its accumulate
        kernel follows them; anything that waits (synchronize, mean, tonemap ...) brings the image up to date."""
        check(self.L.ct_render_accumulate_async(self.h, first_subframe_id, count), self.h)

    def synchronize(self):
        check(self.L.ct_synchronize(self.h), self.h)

    def point_radiance_launch(self, tasks: np.ndarray, first_frame_id: int, launches: int) -> np.ndarray:
        """`launches` launches of estimateEmission (pointEmissionCamera.cu:20-40) over `tasks`
        (POINT_TASK_DTYPE), updated in place and returned."""
        assert tasks.dtype == POINT_TASK_DTYPE and tasks.flags.c_contiguous
        check(self.L.ct_point_radiance_launch(self.h, _p(tasks), len(tasks), first_frame_id, launches), self.h)
        return tasks

    def radiance_collector(self, positions, directions, **params):
        """A collector.DeviceRadianceCollector on this handle (ct_collector_*): RadianceCollector's loop over these tasks with
        replication, merge, stopping rule and re-packing on the device.  params: batch_start_id, max_thread_count,
        launches_per_update, rel_tol, abs_tol, zero_samples (default: the reference's)."""
        from .collector import DeviceRadianceCollector
        return DeviceRadianceCollector(self, positions, directions, **params)

    def adaptive_frame(self, round_samples: int = 10, max_samples: int = 1000, min_samples: int = 100, rel_tol: float = 2e-2,
                       abs_tol: float = 1e-2, chunk_pixels: int = 0, pass_subframes: int = 0, shard: bool = False):
        """An adaptive.AdaptiveFrame on this handle (ct_adaptive_frame_*): the image of the current pose and light in rounds of
        `round_samples` subframes that go only to the pixels which have not yet passed Camera::isConverged's test (tested from
        `min_samples` on), at most `max_samples` per pixel.  The handle's own image is not touched.  Defaults: the reference's
        cadence, minimum and tolerances.  shard: ct_adaptive_frame_create_shard -- the frame of this tracer's own pixels
        (shard_index of shard_count), zero elsewhere; without it a sharded tracer is refused."""
        from .adaptive import AdaptiveFrame
        return AdaptiveFrame(self, round_samples, max_samples, min_samples, rel_tol, abs_tol, chunk_pixels, pass_subframes, shard)

    def generate_scatter_samples(self, count: int, batch_seed: int = 0):
        """generatePoints + firstScatterPosition: -> (positions [count,3], view directions [count,3])."""
        pos = np.empty((count, 3), np.float32)
        d = np.empty((count, 3), np.float32)
        check(self.L.ct_generate_scatter_samples(self.h, count, batch_seed & 0xFFFFFFFF, _p(pos), _p(d)), self.h)
        return pos, d

    def collect_descriptors(self, positions: np.ndarray, directions: np.ndarray) -> np.ndarray:
        """setupHierarchicalDescriptor (DisneyDescriptor.cuh:71-112) for (position, view direction) samples:
        -> uint8 [count, 10, 9, 5, 5] (layer, z, y, x), the `grid` bytes of Persistance::DisneyDescriptor."""
        pos = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(directions, np.float32).reshape(-1, 3)
        if len(pos) != len(d):
            raise ValueError("positions and directions differ in length")
        out = np.empty((len(pos), 10, 9, 5, 5), np.uint8)
        check(self.L.ct_collect_descriptors(self.h, _p(pos), _p(d), len(pos), _p(out)), self.h)
        return out

    def descriptor_frame(self, subframe_id: int, rect=None, capacity: int | None = None):
        """ct_descriptor_frame: the network's input for the pixels of `rect` = (x0, y0, x1, y1) (half-open; None = the whole
        frame) -- per pixel whose primary ray scatters in the cloud, the first scatter position and the descriptor there, in
        the rect's row-major order, without leaving the device.
        -> (descriptors uint8 [n,10,9,5,5], positions float32 [n,3], directions float32 [n,3], pixels int32 [n] = y * width + x),
        torch tensors on the handle's device, cut to the number of records.  `capacity` (default: the rect's area) is what the
        tensors are allocated for; fewer than the rect's valid pixels raises CloudTraceError(CT_E_INVAL) whose `needed` is
        their number."""
        import torch
        x0, y0, x1, y1 = (int(v) for v in (rect if rect is not None else (0, 0, self.width, self.height)))
        r = np.array([x0, y0, x1, y1], np.int64)
        if (r < 0).any() or (r >= 2 ** 32).any():
            raise _lib.CloudTraceError(_lib.CT_E_INVAL, "descriptor_frame: rect out of range")
        r = r.astype(np.uint32)
        area = max(x1 - x0, 0) * max(y1 - y0, 0)
        # (a rect never yields more records than it has pixels, and the library refuses one of more than 2^20)
        capacity = min(area if capacity is None else int(capacity), area, 1 << 20)
        if capacity < 0:
            raise ValueError("capacity must not be negative")
        dev = torch.device("cuda", self.params.device)
        n_alloc = max(capacity, 1)
        desc = torch.empty((n_alloc, 10, 9, 5, 5), dtype=torch.uint8, device=dev)
        pos = torch.empty((n_alloc, 3), dtype=torch.float32, device=dev)
        d = torch.empty((n_alloc, 3), dtype=torch.float32, device=dev)
        pix = torch.empty((n_alloc,), dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)      # the library writes them on the handle's stream, not on torch's
        n = C.c_uint32(0)
        rc = self.L.ct_descriptor_frame(self.h, subframe_id & 0xFFFFFFFF, _p(r) if rect is not None else None,
                                        min(capacity, 0xFFFFFFFF), C.c_void_p(desc.data_ptr()), C.c_void_p(pos.data_ptr()),
                                        C.c_void_p(d.data_ptr()), C.c_void_p(pix.data_ptr()), C.byref(n))
        if rc != _lib.CT_OK:
            msg = self.L.ct_last_error(self.h)
            e = _lib.CloudTraceError(rc, msg.decode("utf-8", "replace") if msg else "")
            e.needed = int(n.value)
            raise e
        k = int(n.value)
        return desc[:k], pos[:k], d[:k], pix[:k]

    def descriptor_frame_time(self):
        """-> (first flights + compaction ms, descriptor gather ms) of the last descriptor_frame (ct_debug_descriptor_frame_time)."""
        a, b = C.c_double(0), C.c_double(0)
        check(self.L.ct_debug_descriptor_frame_time(self.h, C.byref(a), C.byref(b)), self.h)
        return float(a.value), float(b.value)

    def network_frame(self, net, subframe_id: int, rect=None):
        """The network's picture of `rect` (None = the whole frame): descriptor_frame, aux = dot(view direction, the direction
        the light travels), net.eval, and the results scattered by the pixel list.
        -> (float32 torch tensor [rect height, rect width] on the handle's device, 0 at the pixels without a record; records).
        `net` is a deepestscatter_amd.network.Network of this tracer with one aux input."""
        import torch
        if net.shape.aux != 1:
            raise ValueError(f"network_frame feeds one aux input (the light angle); this network has {net.shape.aux}")
        x0, y0, x1, y1 = (int(v) for v in (rect if rect is not None else (0, 0, self.width, self.height)))
        desc, _, view, pix = self.descriptor_frame(subframe_id, rect=rect)
        count = int(pix.shape[0])
        image = torch.zeros(((y1 - y0) * (x1 - x0),), dtype=torch.float32, device=desc.device)
        if count:
            light = torch.tensor(self.light_direction(), dtype=torch.float32, device=desc.device)
            aux = (view * light).sum(dim=1).contiguous()
            out = torch.empty((count,), dtype=torch.float32, device=desc.device)
            torch.cuda.synchronize(desc.device)      # the library reads and writes them on the handle's stream, not on torch's
            net.eval(desc.data_ptr(), aux.data_ptr(), count, out.data_ptr())
            p = pix.to(torch.int64)
            image[(p // self.width - y0) * (x1 - x0) + (p % self.width - x0)] = out
        return image.reshape(y1 - y0, x1 - x0), count

    @staticmethod
    def _network_render_params(transform, rgb_scale, band_pixels, direct: bool = False) -> "_lib.CtNetworkRender":
        names = {"linear": _lib.CT_NET_OUT_LINEAR, "expm1": _lib.CT_NET_OUT_EXPM1}
        t = names.get(transform, transform) if isinstance(transform, str) else transform
        if isinstance(t, str):
            raise _lib.CloudTraceError(_lib.CT_E_INVAL, f"network render: unknown transform {transform!r} (linear | expm1)")
        p = _lib.CtNetworkRender()
        p.abi_version = _lib.CT_ABI_VERSION
        p.transform = int(t) | (_lib.CT_NET_ADD_SINGLE_SCATTER if direct else 0)   # (an integer passes through as it is)
        p.rgb_scale[:] = [float(v) for v in rgb_scale]
        p.band_pixels = int(band_pixels)
        return p

    def network_render_subframe(self, net, subframe_id: int, transform="linear", rgb_scale=(1.0, 1.0, 1.0), band_pixels: int = 0,
                                out=None, direct: bool = False):
        """ct_network_render_subframe: the network's frame of one subframe -- per pixel with a first-scatter record
        rgb_scale * max(L, 0) with L = out ("linear") or expf(out) - 1 ("expm1"), alpha 1; (0, 0, 0, 1) elsewhere -- into the
        handle's CT_BUF_FRAME and into a float32 torch tensor [H, W, 4] on the handle's device, which is returned (`out`: a
        tensor of that shape to write into; False: CT_BUF_FRAME only, returns None).  `net`: a deepestscatter_amd.network.Network
        of this tracer with one aux input.  band_pixels: pixels handled at once (0 = 2^20); the image does not depend on it.
        direct=True (CT_NET_ADD_SINGLE_SCATTER): a pixel with a record also gets the sun's single-scatter term of that pixel and
        subframe -- what a CT_MODE_SUN_SINGLE_SCATTER tracer renders there -- added behind the scaled network output, so that a
        network trained on the multiple-scatter labels gives the path tracer's picture."""
        return self._network_render_subframe(self.L.ct_network_render_subframe, net.n, subframe_id, transform, rgb_scale, band_pixels,
                                             out, direct)

    def _network_render_subframe(self, entry, net, subframe_id, transform, rgb_scale, band_pixels, out, direct):
        p = self._network_render_params(transform, rgb_scale, band_pixels, direct)
        ptr = None
        if out is not False:
            import torch
            dev = torch.device("cuda", self.params.device)
            if out is None:
                out = torch.empty((self.height, self.width, 4), dtype=torch.float32, device=dev)
            if tuple(out.shape) != (self.height, self.width, 4) or out.dtype != torch.float32 or not out.is_contiguous():
                raise ValueError("out must be a contiguous float32 tensor [H, W, 4]")
            torch.cuda.synchronize(dev)      # the library writes it on the handle's stream, not on torch's
            ptr = C.c_void_p(out.data_ptr())
        check(entry(self.h, net, C.byref(p), subframe_id & 0xFFFFFFFF, ptr), self.h)
        return None if out is False else out

    def network_render_accumulate(self, net, first_subframe_id: int, count: int, transform="linear", rgb_scale=(1.0, 1.0, 1.0),
                                  band_pixels: int = 0, direct: bool = False):
        """ct_network_render_accumulate: network_render_subframe(id) + accumulate(id) for id = first .. first + count - 1, fused
        (no frame is materialised); mean, M2 and the subframe count end exactly as that loop leaves them.  direct: as there."""
        p = self._network_render_params(transform, rgb_scale, band_pixels, direct)
        check(self.L.ct_network_render_accumulate(self.h, net.n, C.byref(p), first_subframe_id & 0xFFFFFFFF, count), self.h)

    def network_render_shard_subframe(self, net, subframe_id: int, transform="linear", rgb_scale=(1.0, 1.0, 1.0), band_pixels: int = 0,
                                      out=None, direct: bool = False):
        """ct_network_render_shard_subframe: network_render_subframe on a tracer of any shard_count -- the pixels of the shard's
        own tiles are the unsharded frame's, foreign pixels (0, 0, 0, 0) -- rendered tile band by tile band (band_pixels / 64
        tiles at once).  With shard_count == 1 the bits are network_render_subframe's."""
        return self._network_render_subframe(self.L.ct_network_render_shard_subframe, net.n, subframe_id, transform, rgb_scale,
                                             band_pixels, out, direct)

    def network_render_shard_accumulate(self, net, first_subframe_id: int, count: int, transform="linear", rgb_scale=(1.0, 1.0, 1.0),
                                        band_pixels: int = 0, direct: bool = False):
        """ct_network_render_shard_accumulate: network_render_accumulate on a tracer of any shard_count; foreign pixels of mean
        and M2 stay exactly 0, so the sum over the shards is the unsharded image."""
        p = self._network_render_params(transform, rgb_scale, band_pixels, direct)
        check(self.L.ct_network_render_shard_accumulate(self.h, net.n, C.byref(p), first_subframe_id & 0xFFFFFFFF, count), self.h)

    # -- the network baked into a probe table (ct_network_bake, ct_baked_render_*) ------------------------------------
    def network_bake(self, net, grid, azimuths: int, cosines: int, sparse: bool = False, compact: bool = False):
        """ct_network_bake -> deepestscatter_amd.network.Bake: `net` evaluated on grid[0] x grid[1] x grid[2] position nodes x
        `azimuths` (a multiple of 4) x `cosines` polar nodes, for the light as it is now.  sparse: ct_network_bake_sparse, which
        bakes only the probes a first flight can reach; every frame is the same.  compact: ct_network_bake_compact, which also
        stores only those probes (the 2^26 limit then bounds what is stored); `sparse` and `compact` together: ValueError."""
        from .network import Bake
        if sparse and compact:
            raise ValueError("network_bake: sparse or compact, not both")
        return Bake(self, net, grid, azimuths, cosines, sparse, compact)

    def traced_bake(self, grid, azimuths: int, cosines: int, samples: int, sparse: bool = False, compact: bool = False):
        """ct_bake_traced -> deepestscatter_amd.network.Bake: the probe table of network_bake's grid filled with the means of
        `samples` experiments of the path tracer's point estimator (multiply scattered sun radiance) per entry, no network.
        baked_render_*(direct=True) on it renders the path tracer's total up to the table's resolution; Bake.trace_more refines
        it, Bake.retrace follows set_light.  `sparse` and `compact` as in network_bake."""
        from .network import Bake
        if sparse and compact:
            raise ValueError("traced_bake: sparse or compact, not both")
        return Bake(self, None, grid, azimuths, cosines, sparse, compact, samples=int(samples))

    def traced_bake_adaptive(self, grid, azimuths: int, cosines: int, round_samples: int, max_samples: int, rel_tol: float = 2e-2,
                             abs_tol: float = 1e-4, zero_samples: int = 100000, sparse: bool = False, compact: bool = False):
        """ct_bake_traced_adaptive -> deepestscatter_amd.network.Bake: traced_bake's table, traced in rounds of `round_samples`
        experiments that go only to the entries which have not yet passed the reference's stopping rule (95 % confidence interval
        below rel_tol of the mean or below abs_tol; a zero entry after zero_samples experiments), at most `max_samples` per entry.
        Bake.counts / m2 / adaptive_info describe the result, Bake.trace_adaptive_more raises the cap, Bake.retrace_adaptive
        follows set_light.  With the default zero_samples a dense bake runs every empty node to the cap: use sparse or compact."""
        from .network import AdaptiveParams, Bake
        if sparse and compact:
            raise ValueError("traced_bake_adaptive: sparse or compact, not both")
        return Bake(self, None, grid, azimuths, cosines, sparse, compact,
                    adaptive=AdaptiveParams(int(round_samples), int(max_samples), float(rel_tol), float(abs_tol), int(zero_samples)))

    def load_bake(self, path):
        """ct_bake_load -> deepestscatter_amd.network.Bake: the bake that Bake.save wrote to `path`, on this tracer, which must
        hold the same cloud, scene floats, estimator and CT_FLAG_TEX_FIXED8 bit.  A traced or adaptive bake continues from where
        it was saved (Bake.trace_more / trace_adaptive_more); a bake saved under another light loads stale (info["current"] False)."""
        from .network import Bake
        return Bake.load(self, path)

    def volume_hash(self) -> int:
        """ct_debug_volume_hash: the hash of this tracer's quantised density that a bake file carries."""
        v = C.c_uint64(0)
        check(self.L.ct_debug_volume_hash(self.h, C.byref(v)), self.h)
        return int(v.value)

    def bake_mask(self, grid):
        """ct_debug_bake_mask: the sparse bake's mask of a grid (Nx, Ny, Nz) on this handle, no network needed
        -> (cells uint8 [Nz-1, Ny-1, Nx-1], nodes uint8 [Nz, Ny, Nx], the active node indices uint32, ascending)."""
        nx, ny, nz = (int(v) for v in grid)
        g = np.array([nx, ny, nz], np.int64)
        if (g < 0).any() or (g >= 2 ** 32).any():
            raise _lib.CloudTraceError(_lib.CT_E_INVAL, "bake_mask: grid out of range")
        g = g.astype(np.uint32)
        n = C.c_uint32(0)
        ok = bool((g >= 2).all() and (g <= 256).all())                      # (the library refuses the others before it reads the arrays)
        cells = np.empty((nz - 1, ny - 1, nx - 1) if ok else (0, 0, 0), np.uint8)
        nodes = np.empty((nz, ny, nx) if ok else (0, 0, 0), np.uint8)
        active = np.empty(max(nodes.size, 1), np.uint32)
        check(self.L.ct_debug_bake_mask(self.h, _p(g), _p(cells), _p(nodes), _p(active), nodes.size, C.byref(n)), self.h)
        return cells, nodes, active[:n.value].copy()

    def bake_lookup(self, bake, positions, directions):
        """ct_debug_bake_lookup: the table lookup for float32 torch tensors [n, 3] on the handle's device -> float32 tensor [n]."""
        import torch
        w, d = positions.contiguous(), directions.contiguous()
        for t in (w, d):
            if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 3 or t.shape[0] != w.shape[0]:
                raise ValueError("positions and directions must be float32 tensors [n, 3]")
        out = torch.empty((w.shape[0],), dtype=torch.float32, device=w.device)
        torch.cuda.synchronize(w.device)
        n = int(w.shape[0])
        check(self.L.ct_debug_bake_lookup(self.h, bake.b, C.c_void_p(w.data_ptr()) if n else None, C.c_void_p(d.data_ptr()) if n else None, n,
                                          C.c_void_p(out.data_ptr()) if n else None), self.h)
        return out

    def baked_render_subframe(self, bake, subframe_id: int, transform="linear", rgb_scale=(1.0, 1.0, 1.0), band_pixels: int = 0,
                              out=None, direct: bool = False):
        """ct_baked_render_subframe: network_render_subframe with a record's output interpolated from `bake`."""
        return self._network_render_subframe(self.L.ct_baked_render_subframe, bake.b, subframe_id, transform, rgb_scale, band_pixels,
                                             out, direct)

    def baked_render_accumulate(self, bake, first_subframe_id: int, count: int, transform="linear", rgb_scale=(1.0, 1.0, 1.0),
                                band_pixels: int = 0, direct: bool = False):
        """ct_baked_render_accumulate: network_render_accumulate with the table; all subframes are enqueued and waited for once."""
        p = self._network_render_params(transform, rgb_scale, band_pixels, direct)
        check(self.L.ct_baked_render_accumulate(self.h, bake.b, C.byref(p), first_subframe_id & 0xFFFFFFFF, count), self.h)

    def baked_render_shard_subframe(self, bake, subframe_id: int, transform="linear", rgb_scale=(1.0, 1.0, 1.0), band_pixels: int = 0,
                                    out=None, direct: bool = False):
        """ct_baked_render_shard_subframe: baked_render_subframe on a tracer of any shard_count (foreign pixels (0, 0, 0, 0))."""
        return self._network_render_subframe(self.L.ct_baked_render_shard_subframe, bake.b, subframe_id, transform, rgb_scale,
                                             band_pixels, out, direct)

    def baked_render_shard_accumulate(self, bake, first_subframe_id: int, count: int, transform="linear", rgb_scale=(1.0, 1.0, 1.0),
                                      band_pixels: int = 0, direct: bool = False):
        """ct_baked_render_shard_accumulate: baked_render_accumulate on a tracer of any shard_count."""
        p = self._network_render_params(transform, rgb_scale, band_pixels, direct)
        check(self.L.ct_baked_render_shard_accumulate(self.h, bake.b, C.byref(p), first_subframe_id & 0xFFFFFFFF, count), self.h)

    # -- hybrid frames (ct_baked_render_hybrid_*): the path tracer's path through `depth` collisions, then the bake ------------
    def baked_render_hybrid_subframe(self, bake, depth: int, subframe_id: int, transform="linear", rgb_scale=(1.0, 1.0, 1.0),
                                     band_pixels: int = 0, out=None, direct: bool = True):
        """ct_baked_render_hybrid_subframe: baked_render_subframe with the mode-0 path followed through its first `depth` (1 .. 64,
        below max_depth) collisions, their NEE terms added as the path tracer adds them, and `bake` read at collision `depth`
        along the direction the path arrived in.  depth 1 is baked_render_subframe; from depth 2 on `direct` must be True."""
        def entry(h, b, p, sid, ptr):
            return self.L.ct_baked_render_hybrid_subframe(h, b, p, int(depth) & 0xFFFFFFFF, sid, ptr)
        return self._network_render_subframe(entry, bake.b, subframe_id, transform, rgb_scale, band_pixels, out, direct)

    def baked_render_hybrid_accumulate(self, bake, depth: int, first_subframe_id: int, count: int, transform="linear",
                                       rgb_scale=(1.0, 1.0, 1.0), band_pixels: int = 0, direct: bool = True):
        """ct_baked_render_hybrid_accumulate: baked_render_hybrid_subframe(id) + accumulate(id) for the ids, fused."""
        p = self._network_render_params(transform, rgb_scale, band_pixels, direct)
        check(self.L.ct_baked_render_hybrid_accumulate(self.h, bake.b, C.byref(p), int(depth) & 0xFFFFFFFF, first_subframe_id & 0xFFFFFFFF,
                                                       count), self.h)

    def baked_render_hybrid_shard_subframe(self, bake, depth: int, subframe_id: int, transform="linear", rgb_scale=(1.0, 1.0, 1.0),
                                           band_pixels: int = 0, out=None, direct: bool = True):
        """ct_baked_render_hybrid_shard_subframe: baked_render_hybrid_subframe on a tracer of any shard_count (foreign pixels
        (0, 0, 0, 0))."""
        def entry(h, b, p, sid, ptr):
            return self.L.ct_baked_render_hybrid_shard_subframe(h, b, p, int(depth) & 0xFFFFFFFF, sid, ptr)
        return self._network_render_subframe(entry, bake.b, subframe_id, transform, rgb_scale, band_pixels, out, direct)

    def baked_render_hybrid_shard_accumulate(self, bake, depth: int, first_subframe_id: int, count: int, transform="linear",
                                             rgb_scale=(1.0, 1.0, 1.0), band_pixels: int = 0, direct: bool = True):
        """ct_baked_render_hybrid_shard_accumulate: baked_render_hybrid_accumulate on a tracer of any shard_count."""
        p = self._network_render_params(transform, rgb_scale, band_pixels, direct)
        check(self.L.ct_baked_render_hybrid_shard_accumulate(self.h, bake.b, C.byref(p), int(depth) & 0xFFFFFFFF,
                                                             first_subframe_id & 0xFFFFFFFF, count), self.h)

    def baked_render_time(self) -> float:
        """GPU milliseconds of the last baked_render_* call (ct_debug_baked_render_time)."""
        ms = C.c_double(0)
        check(self.L.ct_debug_baked_render_time(self.h, C.byref(ms)), self.h)
        return float(ms.value)

    def network_scratch(self) -> dict:
        """ct_debug_network_scratch: the device addresses and capacities of the network renderer's scratch (a warm call leaves
        them as they are)."""
        v = (C.c_uint64 * 12)()
        check(self.L.ct_debug_network_scratch(self.h, v), self.h)
        names = ("found", "waves", "pos", "dir", "aux", "out", "desc", "direct", "tiles", "band_cap", "desc_cap", "direct_cap")
        return {k: int(x) for k, x in zip(names, v)}

    def network_aux(self, directions):
        """ct_debug_network_aux: the renderer's aux input dot(direction, the direction the light travels) for a float32 torch
        tensor [n, 3] on the handle's device -> float32 tensor [n]."""
        import torch
        d = directions.contiguous()
        if d.dtype != torch.float32 or d.dim() != 2 or d.shape[1] != 3:
            raise ValueError("directions must be a float32 tensor [n, 3]")
        aux = torch.empty((d.shape[0],), dtype=torch.float32, device=d.device)
        torch.cuda.synchronize(d.device)
        check(self.L.ct_debug_network_aux(self.h, C.c_void_p(d.data_ptr()) if d.shape[0] else None, int(d.shape[0]),
                                          C.c_void_p(aux.data_ptr()) if d.shape[0] else None), self.h)
        return aux

    def network_render_time(self):
        """-> (first flights + compaction, descriptor gather, network, aux + compose / accumulate) GPU milliseconds of the last
        network_render_subframe / network_render_accumulate, summed over its bands and subframes (ct_debug_network_render_time)."""
        ms = (C.c_double * 4)()
        check(self.L.ct_debug_network_render_time(self.h, ms), self.h)
        return tuple(float(v) for v in ms)

    def light_direction(self) -> np.ndarray:
        """The direction the light travels, as the library normalises it (twice, like the reference: ct_set_light)."""
        v = np.asarray(self._light, np.float32)
        for _ in range(2):
            v = v * (np.float32(1) / np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2], dtype=np.float32))
        return v

    def reset(self):
        check(self.L.ct_reset(self.h), self.h)

    def tonemap(self, exposure: float = 0.4):
        """-> (uint8 [H,W,4] screen, average luminance)."""
        screen = np.empty((self.height, self.width, 4), np.uint8)
        avg = C.c_float(0)
        check(self.L.ct_tonemap(self.h, exposure, _p(screen), C.byref(avg)), self.h)
        return screen, float(avg.value)

    def tonemap_async(self, exposure: float = 0.4):
        """ct_tonemap_async: the display update enqueued behind the batches in flight; the screen stays on the device
        (download(CT_BUF_SCREEN) after synchronize())."""
        check(self.L.ct_tonemap_async(self.h, exposure), self.h)

    def set_render_ahead(self, subframes: int):
        """ct_set_render_ahead: enqueued calls of fewer subframes than this are served by launches of this many, each call
        accumulating its own share (the reference's 10-subframe display cadence at the speed of long launches)."""
        check(self.L.ct_set_render_ahead(self.h, subframes), self.h)

    def rendered_subframes(self) -> int:
        n = C.c_uint32(0)
        check(self.L.ct_rendered_subframes(self.h, C.byref(n)), self.h)
        return int(n.value)

    def set_stop_when_converged(self, cadence: int = 10, min_subframes: int = 100):
        """ct_set_stop_when_converged: Camera::isConverged tested on the device behind every `cadence`-th subframe; the running
        mean freezes at the first count that passes (the reference's stopping point, Camera.cpp:179,232-268)."""
        check(self.L.ct_set_stop_when_converged(self.h, cadence, min_subframes), self.h)

    def converged_at(self):
        """-> (subframes the image was frozen at or 0, count of the last finished test, its unconverged pixels); never waits."""
        a, b, c = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
        check(self.L.ct_converged_at(self.h, C.byref(a), C.byref(b), C.byref(c)), self.h)
        return int(a.value), int(b.value), int(c.value)

    def is_converged(self):
        ok, bad = C.c_int32(0), C.c_uint64(0)
        check(self.L.ct_is_converged(self.h, C.byref(ok), C.byref(bad)), self.h)
        return bool(ok.value), int(bad.value)

    def tonemap_buffer(self, mean_dev_ptr: int, exposure: float = 0.4):
        """ct_tonemap_buffer: the tonemap of a caller-owned W*H float4 device buffer (a merged multi-GPU frame)."""
        screen = np.empty((self.height, self.width, 4), np.uint8)
        avg = C.c_float(0)
        check(self.L.ct_tonemap_buffer(self.h, C.c_void_p(mean_dev_ptr), exposure, _p(screen), C.byref(avg)), self.h)
        return screen, float(avg.value)

    def is_converged_buffers(self, mean_dev_ptr: int, m2_dev_ptr: int, subframes: int):
        ok, bad = C.c_int32(0), C.c_uint64(0)
        check(self.L.ct_is_converged_buffers(self.h, C.c_void_p(mean_dev_ptr), C.c_void_p(m2_dev_ptr), subframes,
                                             C.byref(ok), C.byref(bad)), self.h)
        return bool(ok.value), int(bad.value)

    # -- data ---------------------------------------------------------------------------------------
    def download(self, which: int) -> np.ndarray:
        n = C.c_size_t(0)
        check(self.L.ct_buffer_bytes(self.h, which, C.byref(n)), self.h)
        if which in (CT_BUF_MEAN, CT_BUF_M2, CT_BUF_FRAME):
            out = np.empty((self.height, self.width, 4), np.float32)
        elif which == CT_BUF_SCREEN:
            out = np.empty((self.height, self.width, 4), np.uint8)
        else:
            nx, ny, nz = self.dims
            out = np.empty((nz, ny, nx), np.uint8)
        assert out.nbytes == n.value
        check(self.L.ct_download(self.h, which, _p(out), out.nbytes), self.h)
        return out

    def upload(self, which: int, data: np.ndarray):
        """ct_upload: set the running mean or M2 (checkpoint / resume, with set_subframes)."""
        a = np.ascontiguousarray(data, np.float32)
        check(self.L.ct_upload(self.h, which, _p(a), a.nbytes), self.h)

    @staticmethod
    def _state_path(path):
        """np.savez appends '.npz' to a name without it; np.load does not: both sides use the same file name."""
        from pathlib import Path
        p = Path(path)
        return p if p.suffix == ".npz" else p.with_name(p.name + ".npz")

    def save_state(self, path):
        """(mean, M2, subframe count) -> .npz: everything a progressive render needs to continue exactly.  The count is that of
        the samples IN the buffers: with ct_set_stop_when_converged the running mean freezes at the reference's stopping count
        while the host goes on submitting (and ct_subframes goes on counting) -- then the frozen count is what is saved."""
        n = C.c_uint32(0)
        check(self.L.ct_subframes(self.h, C.byref(n)), self.h)
        mean, m2 = self.mean(), self.m2()          # (these wait: the counts read here and below are what the buffers hold)
        frozen_at = self.converged_at()[0]
        count = frozen_at if frozen_at else n.value
        np.savez(self._state_path(path), mean=mean, m2=m2, subframes=np.uint32(count))

    def load_state(self, path) -> int:
        """The reverse: the handle continues with subframe `count + 1`.  A handle whose image had frozen is released (ct_upload
        and ct_set_subframes clear the flag: the image they describe is a new one)."""
        with np.load(self._state_path(path)) as z:
            self.upload(CT_BUF_MEAN, z["mean"])
            self.upload(CT_BUF_M2, z["m2"])
            n = int(z["subframes"])
        self.set_subframes(n)
        return n

    def track_lines(self, enable: bool = True):
        """ct_debug_track_lines: record which 128-B lines of the density and shadow arrays the launches read (CT_STATS=1)."""
        check(self.L.ct_debug_track_lines(self.h, 1 if enable else 0), self.h)

    def touched_lines(self, clear: bool = False) -> dict:
        out = (C.c_uint64 * 4)()
        check(self.L.ct_debug_touched_lines(self.h, out, 1 if clear else 0), self.h)
        return {"density_lines_touched": int(out[0]), "shadow_lines_touched": int(out[1]), "density_lines": int(out[2]), "shadow_lines": int(out[3]),
                "touched_MiB": (int(out[0]) + int(out[1])) * 128 / 2 ** 20}

    def mean(self):
        return self.download(CT_BUF_MEAN)

    def m2(self):
        return self.download(CT_BUF_M2)

    def frame(self):
        return self.download(CT_BUF_FRAME)

    def inscatter(self):
        return self.download(CT_BUF_INSCATTER)

    def copy_to_device(self, which: int, dst_dev_ptr: int, nbytes: int):
        """D2D copy of a handle buffer into caller-owned device memory (e.g. a torch tensor)."""
        check(self.L.ct_copy_to_device(self.h, which, C.c_void_p(dst_dev_ptr), nbytes), self.h)

    def copy_to_device_async(self, which: int, dst_dev_ptr: int, nbytes: int):
        """The same, enqueued on the handle's stream behind the accumulate kernels, not waited for."""
        check(self.L.ct_copy_to_device_async(self.h, which, C.c_void_p(dst_dev_ptr), nbytes), self.h)

    def device_ptr(self, which: int) -> int:
        p = C.c_void_p()
        check(self.L.ct_device_ptr(self.h, which, C.byref(p)), self.h)
        return int(p.value)

    @property
    def subframes(self) -> int:
        n = C.c_uint32(0)
        check(self.L.ct_subframes(self.h, C.byref(n)), self.h)
        return int(n.value)

    def set_subframes(self, n: int):
        check(self.L.ct_set_subframes(self.h, n), self.h)

    def counters(self) -> dict:
        c = CtCounters()
        check(self.L.ct_counters(self.h, C.byref(c)), self.h)
        return c.as_dict()

    def fetch_counters(self) -> dict:
        """What the kernels issued for the lookups `counters()` reports (ct_fetch_counters)."""
        c = CtFetchCounters()
        check(self.L.ct_fetch_counters(self.h, C.byref(c)), self.h)
        return c.as_dict()

    def debug_invariants(self) -> dict:
        """Path conservation / sample integrity tallies (ct_debug_invariants)."""
        out = np.zeros(8, np.uint64)
        check(self.L.ct_debug_invariants(self.h, _p(out)), self.h)
        names = ["armed", "checks", "violations", "samples_without_alpha_1", "dealt", "resumed", "written", "suspended"]
        return {n: int(v) for n, v in zip(names, out)}

    def debug_pixel_classes(self) -> dict:
        """This shard's pixels of the current pose by class, and the lookups of one sample of every through pixel, summed
        (ct_debug_pixel_classes)."""
        out = np.zeros(4, np.uint64)
        check(self.L.ct_debug_pixel_classes(self.h, _p(out)), self.h)
        return {n: int(v) for n, v in zip(["misses", "listed", "through", "through_steps"], out)}

    def debug_pixel_class_plane(self) -> tuple[np.ndarray, np.ndarray]:
        """(class uint8 [H, W], steps uint32 [H, W]) of every pixel of the frame (ct_debug_pixel_class_plane)."""
        out = np.zeros(self.params.width * self.params.height, np.uint32)
        check(self.L.ct_debug_pixel_class_plane(self.h, _p(out), out.size), self.h)
        out = out.reshape(self.params.height, self.params.width)
        return (out >> 30).astype(np.uint8), out & np.uint32(0x3FFFFFFF)

    def debug_memory(self) -> dict:
        """Bytes of the volume representations on the device (ct_debug_memory)."""
        out = np.zeros(8, np.uint64)
        check(self.L.ct_debug_memory(self.h, _p(out)), self.h)
        names = ["raw_texture", "density_bricks", "inscatter_bricks", "march_bricks_dense", "march_bricks_stored", "sparse",
                 "row_table", "coarse_clearance"]
        return {n: int(v) for n, v in zip(names, out)}

    def delta_grid(self) -> dict:
        """The DELTA estimator's majorant grid and kernel variant (ct_debug_delta_grid)."""
        out = np.zeros(8, np.uint32)
        check(self.L.ct_debug_delta_grid(self.h, _p(out)), self.h)
        return {"cell": int(out[0]), "stored": tuple(int(v) for v in out[1:4]), "origin": tuple(int(v) for v in out[4:7]),
                "nee": int(out[7] & 0xff), "interior": bool(out[7] & 0x100)}

    def march_meta(self) -> dict:
        """The march bricks' row meta bytes (ct_debug_march_meta): "meta"[z, y, bx] is the byte of the row of base texels
        x = 3 bx - bias_x .. +2, y - bias, z - bias (dense bricks; None when sparse)."""
        geom = np.zeros(8, np.uint32)
        check(self.L.ct_debug_march_meta(self.h, _p(geom), C.c_void_p(), 0), self.h)
        d = {"radius": int(geom[0]), "bias_x": int(geom[1]), "bias": int(geom[2]),
             "bricks": tuple(int(v) for v in geom[3:6]), "sparse": bool(geom[6]), "meta": None}
        if not d["sparse"]:
            gx, gy, gz = d["bricks"]
            meta = np.zeros((gz * 4, gy * 4, gx), np.uint8)
            check(self.L.ct_debug_march_meta(self.h, _p(geom), _p(meta), meta.size), self.h)
            d["meta"] = meta
        return d

    LAYOUTS = ("density_bricks", "shadow_bricks", "march_bricks", "march_rows", "march_coarse", "twin_bricks", "majorant_cells",
               "majorant_codes", "mip_pyramid")

    def layout(self, which) -> tuple[np.ndarray, dict]:
        """The device bytes of one volume layout as stored, and the geometry that indexes it (ct_debug_layout): `which` is a
        name of LAYOUTS or a CT_LAYOUT_* value.  Bricks come as uint8 [bz, by, bx, 128] (sparse march bricks: [stored brick,
        128]), the row table as uint32 [bz, by, 2], the coarse grid and the majorant cells / codes as uint8 [z, y, x], the mip
        pyramid as its raw bytes, level after level (geometry: "levels" and the level-0 "dims" x, y, z).  A layout the handle
        does not have raises CloudTraceError(CT_E_INVAL)."""
        which = self.LAYOUTS.index(which) if isinstance(which, str) else int(which)
        geom, n = np.zeros(16, np.uint32), C.c_size_t(0)
        check(self.L.ct_debug_layout(self.h, which, _p(geom), C.c_void_p(), 0, C.byref(n)), self.h)
        g = [int(v) for v in geom]
        raw = np.zeros(n.value, np.uint8)
        check(self.L.ct_debug_layout(self.h, which, _p(geom), _p(raw), raw.size, C.byref(n)), self.h)
        if which in (_lib.CT_LAYOUT_DENSITY_BRICKS, _lib.CT_LAYOUT_SHADOW_BRICKS, _lib.CT_LAYOUT_TWIN_BRICKS):
            d = {"bias": g[0], "bricks": tuple(g[1:4])}
            return raw.reshape(g[3], g[2], g[1], 128), d
        if which == _lib.CT_LAYOUT_MARCH_BRICKS:
            d = {"bias_x": g[0], "bias": g[1], "bricks": tuple(g[2:5]), "sparse": bool(g[5])}
            return (raw.reshape(-1, 128) if d["sparse"] else raw.reshape(g[4], g[3], g[2], 128)), d
        if which == _lib.CT_LAYOUT_MARCH_ROWS:
            return raw.view(np.uint32).reshape(g[1], g[0], 2), {"rows": (g[0], g[1])}
        if which == _lib.CT_LAYOUT_MARCH_COARSE:
            return raw.reshape(g[3], g[2], g[1]), {"shift": g[0], "cells": tuple(g[1:4]), "bias": g[4]}
        if which == _lib.CT_LAYOUT_MIP_PYRAMID:
            return raw, {"levels": g[0], "dims": tuple(g[1:4])}
        d = {"cell": g[0], "div": g[1], "stored": tuple(g[2:5]), "origin": tuple(g[5:8]), "virtual": tuple(g[8:11]), "bias": g[11]}
        return raw.reshape(g[4], g[3], g[2]), d

    def kernel_time(self):
        """-> (estimator kernel ms, accumulate kernel ms, estimator launches) since create/reset."""
        a, b, n = C.c_double(0), C.c_double(0), C.c_uint64(0)
        check(self.L.ct_kernel_time(self.h, C.byref(a), C.byref(b), C.byref(n)), self.h)
        return float(a.value), float(b.value), int(n.value)

    def set_stream(self, hip_stream: int | None):
        check(self.L.ct_set_stream(self.h, C.c_void_p(hip_stream) if hip_stream else None), self.h)

    def debug_stats(self) -> dict:
        """Scheduler diagnostics (only filled when the process runs with CT_STATS=1)."""
        out = np.zeros(64, np.uint64)
        check(self.L.ct_debug_stats(self.h, _p(out)), self.h)
        names = ["regen_phases", "regen_lanes", "march_phases", "march_lanes", "scatter_phases", "scatter_lanes",
                 "fetched_steps", "fetched_zero_cells", "skipped_steps", "zero_cells_nonfree_brick",
                 "zero_cells_free_brick_d1", "skip_loop_wave_iterations", "nee_footprints_reused", "waves",
                 "stolen_jobs", "max_scheduler_visits_of_a_wave"]
        d = {n: int(v) for n, v in zip(names, out)}
        # waves by the time they ended (5 ms bins from their own start), and by how long they kept
        # running after they had found the job queue empty (0.5 ms bins)
        d["wave_end_hist_5ms"] = [int(v) for v in out[16:40]]
        d["wave_end_minus_drained_hist_0p5ms"] = [int(v) for v in out[40:64]]
        ex = np.zeros(82, np.uint64)
        check(self.L.ct_debug_stats_ex(self.h, _p(ex), 82), self.h)
        # of the march fetches: the lane's previous fetch was in the same 128-B brick line / a lower lane of the wave
        # fetches the same line in the same instruction (what a brick cache in LDS could find: DESIGN.md 4.3)
        d["march_fetch_same_line_as_lanes_previous"] = int(ex[68])
        d["march_fetch_line_shared_with_a_lower_lane"] = int(ex[69])
        # of the NEE lookups (MARCH): those whose footprint was known to be zero (shadow-zero row) and not loaded; they are
        # counted in nee_footprints_reused too
        d["nee_lookups_skipped_shadow_zero"] = int(ex[72])
        # MARCH free-space skips of at least one step, and the burst steps in which a lane replayed some of a skip's adds
        # (more of these than skips: skips longer than CT_MARCH_REPLAY_MAX were spread over several burst steps);
        # skip_loop_wave_iterations counts the replay blocks the waves executed
        d["free_space_skips"] = int(ex[73])
        d["replay_lane_steps"] = int(ex[74])
        # MARCH schedule mix: scheduler visits of all waves, the idle lanes they found (summed), the march bursts and the rule
        # that ended each (the step count, too few marching lanes, burst_scatter, the rule of a drained wave)
        d["scheduler_visits"] = int(ex[75])
        d["idle_lanes_at_visits"] = int(ex[76])
        d["march_bursts"] = int(ex[77])
        d["bursts_ended_by"] = {"step_count": int(ex[78]), "march_min": int(ex[79]), "burst_scatter": int(ex[80]),
                                "tail_rule": int(ex[81])}
        d["raw"] = [int(v) for v in out]
        d["watchdog"] = int(out[63])     # exchange kernels: waves that gave up on a bounded wait (must be 0)
        return d

    def debug_suspended(self) -> int:
        """Paths handed from one async launch to the next so far."""
        n = C.c_uint64(0)
        check(self.L.ct_debug_suspended(self.h, C.byref(n)), self.h)
        return int(n.value)

    def debug_math_selftest(self, which: int) -> dict:
        """ct_debug_math_selftest: 0 = reciprocal, 1 = square root, 2 = expf_inrange, 3 = logf_above_one, 4 = floor_to_int,
        5 = fract_ -> {tested, mismatches, first_bad_bits}."""
        out = np.zeros(3, np.uint64)
        check(self.L.ct_debug_math_selftest(self.h, which, _p(out)), self.h)
        return {"tested": int(out[0]), "mismatches": int(out[1]), "first_bad_bits": int(out[2])}

    def debug_math_eval(self, fn: int, a: np.ndarray, b: np.ndarray | None = None) -> tuple[np.ndarray, np.ndarray]:
        """ct_debug_math_eval: scalar function `fn` (the table in cloudtrace.h) of the device code on the operand bit
        patterns a (and b): uint32 arrays in, the two results' bit patterns (r0, r1) as uint32 arrays out."""
        a = np.ascontiguousarray(a, np.uint32).reshape(-1)
        inp = np.zeros((a.size, 2), np.uint32)
        inp[:, 0] = a
        if b is not None:
            inp[:, 1] = np.ascontiguousarray(b, np.uint32).reshape(-1)
        out = np.empty_like(inp)
        check(self.L.ct_debug_math_eval(self.h, fn, _p(inp), a.size, _p(out)), self.h)
        return out[:, 0].copy(), out[:, 1].copy()

    def debug_cdf_inversion(self, first_u24: int, count: int) -> np.ndarray:
        out = np.empty(count, np.uint32)
        check(self.L.ct_debug_cdf_inversion(self.h, first_u24, count, _p(out)), self.h)
        return out


class TracerGroup:
    """Owns one CtGroup: a multi-GPU job driven by ONE process below the C ABI (ct_group_*; RCCL frame reduce).
    `devices` may repeat a device to rehearse an N-GPU job on fewer GPUs (merged without a collective then)."""

    def __init__(self, density: np.ndarray, devices, params: SceneParams | None = None, **kw):
        self.L = _lib.load()
        self.params = params or SceneParams(**kw)
        s, keep = make_scene(density, self.params)
        self.width, self.height = self.params.width, self.params.height
        dev = np.asarray(list(devices), np.int32)
        g = C.c_void_p()
        rc = self.L.ct_group_create(C.byref(s), _p(dev), len(dev), C.byref(g))
        del keep
        if rc != _lib.CT_OK:
            msg = self.L.ct_group_last_error(None)
            raise _lib.CloudTraceError(rc, msg.decode("utf-8", "replace") if msg else "")
        self.g = g

    def _check(self, rc):
        if rc != _lib.CT_OK:
            msg = self.L.ct_group_last_error(self.g)
            raise _lib.CloudTraceError(rc, msg.decode("utf-8", "replace") if msg else "")

    def close(self):
        if getattr(self, "g", None):
            for net in list(getattr(self, "_bakes", ())) + list(getattr(self, "_networks", ())) + list(getattr(self, "_adaptive_frames", ())):
                net.close()       # (a group's bakes, networks and adaptive frames go before the group)
            self.L.ct_group_destroy(self.g)
            self.g = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_camera(self, eye, U, V, W):
        a = [np.asarray(v, np.float32) for v in (eye, U, V, W)]
        self._check(self.L.ct_group_set_camera(self.g, *[_p(v) for v in a]))

    def set_light(self, direction, color=None, intensity: float = 1e6):
        """ct_group_set_light: CloudTracer.set_light on every shard; reset() next."""
        d, c = _light_args(direction, color)
        self._check(self.L.ct_group_set_light(self.g, _p(d) if d is not None else None, _p(c) if c is not None else None, intensity))

    def render_accumulate(self, first_subframe_id: int, count: int):
        self._check(self.L.ct_group_render_accumulate(self.g, first_subframe_id, count))

    def network(self, module_or_weights, width: int | None = None, aux: int | None = None, head_layers: int | None = None):
        """ct_group_network_create: the network on every shard's device -> GroupNetwork (arguments as network.Network's)."""
        return GroupNetwork(self, module_or_weights, width, aux, head_layers)

    def network_render_accumulate(self, net, first_subframe_id: int, count: int, transform="linear", rgb_scale=(1.0, 1.0, 1.0),
                                  band_pixels: int = 0, direct: bool = False):
        """ct_group_network_render_accumulate: CloudTracer.network_render_shard_accumulate on every shard, each shard on a host
        thread of its own; mean(), m2(), tonemap() and is_converged() then give what one unsharded tracer gives."""
        p = CloudTracer._network_render_params(transform, rgb_scale, band_pixels, direct)
        self._check(self.L.ct_group_network_render_accumulate(self.g, net.gn if net is not None else None, C.byref(p),
                                                              first_subframe_id & 0xFFFFFFFF, count))

    # -- bakes on the group (ct_group_bake_*): built across the shards, complete on every shard ------------------------
    @staticmethod
    def _bake_args(who, grid, azimuths, cosines, sparse, compact):
        if sparse and compact:
            raise ValueError(f"{who}: sparse or compact, not both")
        d = _lib.CtBakeDesc(_lib.CT_ABI_VERSION, (C.c_uint32 * 3)(*[int(v) for v in grid]), int(azimuths), int(cosines))
        return d, _lib.CT_BAKE_COMPACT if compact else _lib.CT_BAKE_SPARSE if sparse else _lib.CT_BAKE_DENSE

    def network_bake(self, net, grid, azimuths: int, cosines: int, sparse: bool = False, compact: bool = False):
        """ct_group_network_bake -> deepestscatter_amd.network.GroupBake: CloudTracer.network_bake of the GroupNetwork `net`, every
        shard baking its span of the nodes; every shard then holds the single-GPU bake, bit for bit."""
        from .network import GroupBake
        d, kind = self._bake_args("network_bake", grid, azimuths, cosines, sparse, compact)
        gb = C.c_void_p()
        self._check(self.L.ct_group_network_bake(self.g, net.gn if net is not None else None, C.byref(d), kind, C.byref(gb)))
        return GroupBake(self, gb)

    def traced_bake(self, grid, azimuths: int, cosines: int, samples: int, sparse: bool = False, compact: bool = False):
        """ct_group_bake_traced -> GroupBake: CloudTracer.traced_bake with every shard tracing its span of the nodes."""
        from .network import GroupBake
        d, kind = self._bake_args("traced_bake", grid, azimuths, cosines, sparse, compact)
        gb = C.c_void_p()
        self._check(self.L.ct_group_bake_traced(self.g, C.byref(d), kind, int(samples), C.byref(gb)))
        return GroupBake(self, gb)

    def traced_bake_adaptive(self, grid, azimuths: int, cosines: int, round_samples: int, max_samples: int, rel_tol: float = 2e-2,
                             abs_tol: float = 1e-4, zero_samples: int = 100000, sparse: bool = False, compact: bool = False):
        """ct_group_bake_traced_adaptive -> GroupBake: CloudTracer.traced_bake_adaptive with every shard running its own rounds over
        its span; a shard whose entries all stop early ends sooner."""
        from .network import GroupBake
        d, kind = self._bake_args("traced_bake_adaptive", grid, azimuths, cosines, sparse, compact)
        p = _lib.CtBakeAdaptive(_lib.CT_ABI_VERSION, int(round_samples), int(max_samples), int(zero_samples), float(rel_tol), float(abs_tol))
        gb = C.c_void_p()
        self._check(self.L.ct_group_bake_traced_adaptive(self.g, C.byref(d), kind, C.byref(p), C.byref(gb)))
        return GroupBake(self, gb)

    def load_bake(self, path):
        """ct_group_bake_load -> GroupBake: CloudTracer.load_bake on every shard; a single-GPU file loads on a group and continues
        under the group's span rule."""
        import os
        from .network import GroupBake
        gb = C.c_void_p()
        self._check(self.L.ct_group_bake_load(self.g, os.fsencode(path), C.byref(gb)))
        return GroupBake(self, gb)

    def baked_render_accumulate(self, bake, first_subframe_id: int, count: int, transform="linear", rgb_scale=(1.0, 1.0, 1.0),
                                band_pixels: int = 0, direct: bool = False):
        """ct_group_baked_render_accumulate: CloudTracer.baked_render_shard_accumulate of the GroupBake `bake` on every shard, each
        on a host thread of its own; mean(), m2() and tonemap() then give what baked_render_accumulate gives on one tracer."""
        p = CloudTracer._network_render_params(transform, rgb_scale, band_pixels, direct)
        self._check(self.L.ct_group_baked_render_accumulate(self.g, bake.gb if bake is not None else None, C.byref(p),
                                                            first_subframe_id & 0xFFFFFFFF, count))

    def baked_render_hybrid_accumulate(self, bake, depth: int, first_subframe_id: int, count: int, transform="linear",
                                       rgb_scale=(1.0, 1.0, 1.0), band_pixels: int = 0, direct: bool = True):
        """ct_group_baked_render_hybrid_accumulate: CloudTracer.baked_render_hybrid_shard_accumulate of the GroupBake `bake` on
        every shard; mean(), m2() and tonemap() then give what baked_render_hybrid_accumulate gives on one tracer."""
        p = CloudTracer._network_render_params(transform, rgb_scale, band_pixels, direct)
        self._check(self.L.ct_group_baked_render_hybrid_accumulate(self.g, bake.gb if bake is not None else None, C.byref(p),
                                                                   int(depth) & 0xFFFFFFFF, first_subframe_id & 0xFFFFFFFF, count))

    def adaptive_frame(self, **params):
        """ct_group_adaptive_frame_create -> adaptive.GroupAdaptiveFrame: CloudTracer.adaptive_frame's image with every shard
        running its own rounds over its own pixels (params as there: round_samples, max_samples, min_samples, rel_tol, abs_tol,
        chunk_pixels, pass_subframes); the merged frame is the unsharded tracer's, bit for bit."""
        from .adaptive import GroupAdaptiveFrame
        return GroupAdaptiveFrame(self, **params)

    def handle(self, index: int):
        """ct_group_handle: shard `index`'s CtHandle (owned by the group), for the entry points that take one."""
        h = C.c_void_p()
        self._check(self.L.ct_group_handle(self.g, index, C.byref(h)))
        return h

    def reset(self):
        self._check(self.L.ct_group_reset(self.g))

    def merge(self):
        self._check(self.L.ct_group_merge(self.g))

    def _download(self, which):
        out = np.empty((self.height, self.width, 4), np.float32)
        self._check(self.L.ct_group_download(self.g, which, _p(out), out.nbytes))
        return out

    def mean(self):
        return self._download(CT_BUF_MEAN)

    def m2(self):
        return self._download(CT_BUF_M2)

    def tonemap(self, exposure: float = 0.4):
        screen = np.empty((self.height, self.width, 4), np.uint8)
        avg = C.c_float(0)
        self._check(self.L.ct_group_tonemap(self.g, exposure, _p(screen), C.byref(avg)))
        return screen, float(avg.value)

    def is_converged(self):
        ok, bad = C.c_int32(0), C.c_uint64(0)
        self._check(self.L.ct_group_is_converged(self.g, C.byref(ok), C.byref(bad)))
        return bool(ok.value), int(bad.value)

    def counters(self) -> dict:
        c = CtCounters()
        self._check(self.L.ct_group_counters(self.g, C.byref(c)))
        return c.as_dict()


class GroupNetwork:
    """A CtGroupNetwork: one CtNetwork per shard of a TracerGroup (TracerGroup.network).  Closed with, or before, its group."""

    def __init__(self, group: TracerGroup, module_or_weights, width=None, aux=None, head_layers=None):
        from . import network as N
        self.L, self.group = group.L, group
        if hasattr(module_or_weights, "blocks"):
            self.shape = module_or_weights.shape
            weights = N.pack_weights(module_or_weights)
        else:
            self.shape = N.NetworkShape(*(d if v is None else int(v) for v, d in zip((width, aux, head_layers), (200, 1, 3))))
            weights = np.ascontiguousarray(module_or_weights, np.float32).reshape(-1)
        d = _lib.CtNetworkDesc(_lib.CT_ABI_VERSION, N.BLOCKS, self.shape.width, self.shape.aux, self.shape.head_layers,
                               weights.ctypes.data_as(C.c_void_p), weights.size)
        gn = C.c_void_p()
        group._check(self.L.ct_group_network_create(group.g, C.byref(d), C.byref(gn)))
        self.gn = gn
        group.__dict__.setdefault("_networks", []).append(self)

    def close(self):
        if getattr(self, "gn", None):
            self.L.ct_group_network_destroy(self.gn)
            self.gn = None
            if self in getattr(self.group, "_networks", []):
                self.group._networks.remove(self)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def algorithmic_bytes(counters: dict, pixels_times_spp: int) -> int:
    """8 B per trilinear lookup (density or shadow volume) + 64 B per
    pixel per subframe of accumulation."""
    return 8 * (counters["density_lookups"] + counters["inscatter_lookups"]) + 64 * pixels_times_spp
