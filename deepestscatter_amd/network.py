"""The scattering network that ct_network_eval runs on descriptor records (include/cloudtrace.h, "the scattering network").

The network is THIS PROJECT'S DEFINITION: the reference's DisneyModel.py was not available, so this is the progressive-feed
residual MLP of the paper the reference implements (Kallweit et al. 2017), parameterised by its shapes.

    ScatterNet          the torch.nn.Module a user trains or loads a state dict into (float32, no rounding)
    pack_weights        its parameters as the flat float32 array of CtNetworkDesc.weights_host
    reference_forward   numpy, with the rounding points of the definition: what the device is held to
    Network             a CtNetwork on a CloudTracer's device
    render_values       numpy restatement of what ct_network_render_* makes of the outputs (transform, clamp, rgb scale)
    Bake                a CtBake: the network evaluated on a probe grid (ct_network_bake), which ct_baked_render_* interpolate
    bake_azimuth / bake_lookup_reference   numpy float32 restatement of the table lookup: what the device is held to
    bake_mask_reference numpy restatement of the sparse bake's mask (ct_network_bake_sparse): cells, nodes and the margin M
    bake_slots_reference numpy restatement of the compact bake's slot index (ct_network_bake_compact)
    point_fold_var_reference / point_converged_reference   numpy restatement of an adaptive traced bake's fold and stopping rule
    bake_file_dtype / write_bake_file_reference / read_bake_file_reference   numpy restatement of the bake file (ct_bake_save)
    volume_hash_reference / half_round_reference   the file's volume hash; ct_bake_half's rounding and refusal rule
    bake_file_info      ct_bake_file_info: a bake file checked without a device
    save_weights / load_weights   the weight file `cloudtrace --network` reads

State-dict names (the mapping an exported model needs): blocks.k.fc1 = W1_k, c1_k; blocks.k.fc2 = W2_k, c2_k (k = 0 .. 9);
head.i = V_i, d_i (i = 0 .. H - 2); out = v, d.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import check

BLOCKS = 10          # CT_DESCRIPTOR_LAYERS
LAYER_BYTES = 225    # CT_DESCRIPTOR_LAYER_SIZE
RECORD_BYTES = BLOCKS * LAYER_BYTES


@dataclass(frozen=True)
class NetworkShape:
    width: int = 200
    aux: int = 1
    head_layers: int = 3

    def fan_in(self, block: int) -> int:
        return (self.width if block else 0) + LAYER_BYTES + self.aux

    def weight_count(self) -> int:
        w = self.width
        blocks = sum(w * self.fan_in(k) + w + w * w + w for k in range(BLOCKS))
        return blocks + (self.head_layers - 1) * (w * w + w) + w + 1

    def macs(self) -> int:
        """Multiply-adds per record (the biases are not counted)."""
        w = self.width
        return sum(w * self.fan_in(k) + w * w for k in range(BLOCKS)) + (self.head_layers - 1) * w * w + w


def bf16_round(x) -> np.ndarray:
    """float32 -> bf16 -> float32, round to nearest, ties to even; a NaN stays a NaN (as ct_debug_bf16_round)."""
    a = np.ascontiguousarray(x, np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = np.where(nan, (u | 0x400000) & 0xFFFF0000, r)
    return r.astype(np.uint32).view(np.float32).reshape(a.shape)


def _torch_module():
    import torch

    class _Block(torch.nn.Module):
        def __init__(self, fan_in, width):
            super().__init__()
            self.fc1 = torch.nn.Linear(fan_in, width)
            self.fc2 = torch.nn.Linear(width, width)

    class ScatterNet(torch.nn.Module):
        """forward(descriptors uint8 [n, 10, ...] or [n, 2250], aux float [n, A] or None) -> [n]."""

        def __init__(self, width: int = 200, aux: int = 1, head_layers: int = 3):
            super().__init__()
            self.shape = NetworkShape(width, aux, head_layers)
            self.blocks = torch.nn.ModuleList(_Block(self.shape.fan_in(k), width) for k in range(BLOCKS))
            self.head = torch.nn.ModuleList(torch.nn.Linear(width, width) for _ in range(head_layers - 1))
            self.out = torch.nn.Linear(width, 1)

        def forward(self, descriptors, aux=None):
            dtype = self.out.weight.dtype
            n = descriptors.shape[0]
            b = descriptors.reshape(n, BLOCKS, LAYER_BYTES).to(dtype) / 255.0
            a = aux.reshape(n, self.shape.aux).to(dtype) if self.shape.aux else b.new_zeros((n, 0))
            relu = torch.nn.functional.relu
            z = None
            for k, blk in enumerate(self.blocks):
                x = torch.cat([b[:, k], a] if z is None else [z, b[:, k], a], dim=1)
                h = relu(blk.fc1(x))
                z = relu(blk.fc2(h)) if z is None else relu(z + blk.fc2(h))
            for layer in self.head:
                z = relu(layer(z))
            return self.out(z)[:, 0]

    return ScatterNet


def __getattr__(name):
    # ScatterNet needs torch, which the rest of this module (and the CPU-only users of the package) does not
    if name == "ScatterNet":
        cls = _torch_module()
        globals()["ScatterNet"] = cls
        return cls
    raise AttributeError(name)


def pack_weights(module) -> np.ndarray:
    """The flat float32 array of CtNetworkDesc.weights_host: block after block W1, c1, W2, c2, then the head, each matrix before
    its bias."""
    layers = []
    for blk in module.blocks:
        layers += [blk.fc1, blk.fc2]
    layers += list(module.head) + [module.out]
    parts = []
    for layer in layers:
        parts.append(layer.weight.detach().cpu().numpy().astype(np.float32).reshape(-1))
        parts.append(layer.bias.detach().cpu().numpy().astype(np.float32).reshape(-1))
    flat = np.concatenate(parts)
    assert flat.size == module.shape.weight_count()
    return flat


def unpack_weights(weights, shape: NetworkShape):
    """-> [(W [out, in], bias [out])] in the array's order: W1_0, W2_0, W1_1, ... , V_i ..., v."""
    w = np.ascontiguousarray(weights, np.float32).reshape(-1)
    if w.size != shape.weight_count():
        raise ValueError(f"{w.size} weights, the shapes imply {shape.weight_count()}")
    dims = []
    for k in range(BLOCKS):
        dims += [(shape.width, shape.fan_in(k)), (shape.width, shape.width)]
    dims += [(shape.width, shape.width)] * (shape.head_layers - 1) + [(1, shape.width)]
    out, at = [], 0
    for rows, cols in dims:
        W = w[at:at + rows * cols].reshape(rows, cols)
        at += rows * cols
        out.append((W, w[at:at + rows]))
        at += rows
    return out


def reference_forward(weights, desc: NetworkShape, descriptors_u8, aux, accumulate=np.float64, rounding: bool = True) -> np.ndarray:
    """The rounded model on the CPU: bf16 weights (byte columns as bf16(w / 255)), bytes as integers, aux / h / z rounded to
    bf16 when produced, a layer's products and float32 bias summed in `accumulate`, out in float32's range as `accumulate`.
    accumulate=np.float64 is the definition the device is held to, np.float32 the restatement whose distance from it sets the
    tolerance.  rounding=False (tests only) is the plain network in `accumulate`: ScatterNet.forward."""
    acc = np.dtype(accumulate)
    rnd = (lambda v: bf16_round(np.asarray(v, np.float32)).astype(acc)) if rounding else (lambda v: np.asarray(v, acc))
    layers = unpack_weights(weights, desc)
    n = len(descriptors_u8)
    b = np.asarray(descriptors_u8, np.uint8).reshape(n, BLOCKS, LAYER_BYTES).astype(acc)
    a = rnd(np.asarray(aux, np.float32).reshape(n, desc.aux)) if desc.aux else np.zeros((n, 0), acc)

    def matrix(W, byte_first=None):
        W = np.array(W, np.float32)
        if byte_first is not None:
            cols = slice(byte_first, byte_first + LAYER_BYTES)
            if rounding:
                W[:, cols] = W[:, cols] / np.float32(255.0)
            else:
                W = W.astype(acc)
                W[:, cols] = W[:, cols] / acc.type(255.0)
        return rnd(W)

    def linear(x, W, c):
        return x @ W.T + c.astype(acc)

    z = None
    for k in range(BLOCKS):
        (W1, c1), (W2, c2) = layers[2 * k], layers[2 * k + 1]
        x = np.concatenate([b[:, k], a] if z is None else [z, b[:, k], a], axis=1)
        h = rnd(np.maximum(linear(x, matrix(W1, desc.width if k else 0), c1), 0))
        y = linear(h, matrix(W2), c2)
        z = rnd(np.maximum(y if z is None else z + y, 0))
    for W, c in layers[2 * BLOCKS:-1]:
        z = rnd(np.maximum(linear(z, matrix(W), c), 0))
    W, c = layers[-1]
    return linear(z, matrix(W), c)[:, 0]


def render_values(out, transform="linear", rgb_scale=(1.0, 1.0, 1.0), expf=None, direct=None) -> np.ndarray:
    """The pixel values ct_network_render_* makes of network outputs, restated in numpy float32: L = out ("linear") or
    expf(out) - 1 ("expm1"), g = L if L > 0 else 0 (so a NaN gives 0), pixel = (rgb_scale * g, 1) -> float32 [n, 4].
    `expf`: a float -> float function standing for the library's ct_expf (include/ct_fmath.h); "expm1" needs one (np.exp is
    not bit-identical to it).  `direct`: float32 [n, 3], the single-scatter term of CT_NET_ADD_SINGLE_SCATTER per record, added
    to the rgb after the scale, in float32."""
    o = np.ascontiguousarray(out, np.float32).reshape(-1)
    if transform in ("linear", 0):
        L = o
    elif transform in ("expm1", 1):
        if expf is None:
            raise ValueError("render_values: the expm1 transform needs an expf function")
        L = np.array([np.float32(expf(float(v))) for v in o], np.float32) - np.float32(1.0)
    else:
        raise ValueError(f"render_values: unknown transform {transform!r} (linear | expm1)")
    with np.errstate(invalid="ignore"):
        g = np.where(L > 0, L, np.float32(0)).astype(np.float32)
    s = np.asarray(rgb_scale, np.float32).reshape(3)
    px = np.empty((o.size, 4), np.float32)
    px[:, :3] = s[None, :] * g[:, None]
    px[:, 3] = 1.0
    if direct is not None:
        px[:, :3] += np.ascontiguousarray(direct, np.float32).reshape(o.size, 3)
    return px


def bake_azimuth(directions, axis_a, axis_b) -> np.ndarray:
    """The azimuth t in [0, 4] of float32 directions [n, 3] around the light axis, in the frame (axis_a, axis_b) of a CtBakeInfo:
    px = d . a, py = d . b (left to right), s = |px| + |py|, t = 0 when s is 0 or not finite, else p = px / s and
    t = 1 - p (py >= 0) or 3 + p.  No trigonometric function: float32 numpy gives the device's bits."""
    d = np.ascontiguousarray(directions, np.float32).reshape(-1, 3)
    a, b = np.asarray(axis_a, np.float32).reshape(3), np.asarray(axis_b, np.float32).reshape(3)
    with np.errstate(all="ignore"):
        px = (d[:, 0] * a[0] + d[:, 1] * a[1]) + d[:, 2] * a[2]
        py = (d[:, 0] * b[0] + d[:, 1] * b[1]) + d[:, 2] * b[2]
        s = np.abs(px) + np.abs(py)
        ok = np.isfinite(s) & (s > 0)
        p = px / np.where(ok, s, np.float32(1))
        t = np.where(py >= 0, np.float32(1) - p, np.float32(3) + p)
    return np.where(ok, t, np.float32(0)).astype(np.float32)


def bake_lookup_reference(table, info, box, positions, directions) -> np.ndarray:
    """ct_debug_bake_lookup in numpy float32, the definition the device is held to (include/cloudtrace.h, "the network baked
    into a probe table").  table: float32 of info["entries"] values in the table's order; info: Bake.info (grid, azimuths, cosines,
    light, axis_a, axis_b); box: the box size (bx, by, bz) as float32; positions, directions: float32 [n, 3] -> float32 [n]."""
    f32 = np.float32
    nx, ny, nz = (int(v) for v in info["grid"])
    nphi, nc = int(info["azimuths"]), int(info["cosines"])
    T = np.ascontiguousarray(table, f32).reshape(nz, ny, nx, nphi, nc)
    w = np.ascontiguousarray(positions, f32).reshape(-1, 3)
    d = np.ascontiguousarray(directions, f32).reshape(-1, 3)
    box = np.asarray(box, f32).reshape(3)
    l = np.asarray(info["light"], f32).reshape(3)

    def cell(f, n):
        f = np.minimum(np.maximum(f, f32(0)), f32(n - 1)).astype(f32)
        i0 = np.minimum(f.astype(np.int64), n - 2)
        return i0, (f - i0.astype(f32)).astype(f32)

    def lerp(u, v, wt):
        return (u + ((v - u).astype(f32) * wt).astype(f32)).astype(f32)

    cells = []
    for axis, n in enumerate((nx, ny, nz)):
        scale = f32(f32(n - 1) / box[axis])
        cells.append(cell(((w[:, axis] + f32(0.5) * box[axis]).astype(f32) * scale).astype(f32), n))
    (x0, wx), (y0, wy), (z0, wz) = cells
    c = ((d[:, 0] * l[0] + d[:, 1] * l[1]).astype(f32) + d[:, 2] * l[2]).astype(f32)
    k0, wc = cell(((c + f32(1.0)).astype(f32) * f32(f32(0.5) * f32(nc - 1))).astype(f32), nc)
    ft = (bake_azimuth(d, info["axis_a"], info["axis_b"]) * f32(f32(nphi) * f32(0.25))).astype(f32)
    fl = np.floor(ft).astype(f32)
    wphi = (ft - fl).astype(f32)
    j0 = fl.astype(np.int64) % nphi
    j1 = (j0 + 1) % nphi

    def corner(z, y, x):
        at = [lerp(T[z, y, x, j, k0], T[z, y, x, j, k0 + 1], wc) for j in (j0, j1)]
        return lerp(at[0], at[1], wphi)

    c00 = lerp(corner(z0, y0, x0), corner(z0, y0, x0 + 1), wx)
    c10 = lerp(corner(z0, y0 + 1, x0), corner(z0, y0 + 1, x0 + 1), wx)
    c01 = lerp(corner(z0 + 1, y0, x0), corner(z0 + 1, y0, x0 + 1), wx)
    c11 = lerp(corner(z0 + 1, y0 + 1, x0), corner(z0 + 1, y0 + 1, x0 + 1), wx)
    return lerp(lerp(c00, c10, wy), lerp(c01, c11, wy), wz)


def bake_mask_reference(density, grid, sample_step):
    """The mask of ct_network_bake_sparse in numpy, the definition the device is held to (include/cloudtrace.h, "the sparse
    bake").  density: uint8 [Dz, Dy, Dx]; grid: (Nx, Ny, Nz); sample_step: the handle's (read as float32, like CtScene's).
    -> (cells uint8 [Nz-1, Ny-1, Nx-1], nodes uint8 [Nz, Ny, Nx], M): a cell is occupied when any texel in the box of its three
    per-axis ranges t_lo .. t_hi is non-zero, a node active when a cell it is a corner of is occupied."""
    occupied = np.ascontiguousarray(density) != 0
    if occupied.ndim != 3:
        raise ValueError("density must be [Dz, Dy, Dx]")
    dz, dy, dx = occupied.shape
    nx, ny, nz = (int(v) for v in grid)
    M = int(np.ceil(np.float64(np.float32(sample_step)) * np.float64(max(dx, dy, dz)))) + 3
    for axis, (n, d) in enumerate(((nz, dz), (ny, dy), (nx, dx))):          # the array's axes: z, y, x
        c = np.arange(n - 1, dtype=np.float64)
        lo = np.maximum(0.0, np.floor(c * np.float64(d) / np.float64(n - 1)) - M).astype(np.int64)
        hi = np.minimum(np.float64(d - 1), np.ceil((c + 1.0) * np.float64(d) / np.float64(n - 1)) + M).astype(np.int64)
        count = np.concatenate([np.zeros_like(np.take(occupied, [0], axis), np.int64), np.cumsum(occupied, axis, dtype=np.int64)], axis)
        occupied = (np.take(count, hi + 1, axis) - np.take(count, lo, axis)) > 0
    cells = occupied.astype(np.uint8)
    nodes = np.zeros((nz, ny, nx), np.uint8)
    for oz in (0, 1):
        for oy in (0, 1):
            for ox in (0, 1):
                nodes[oz:oz + nz - 1, oy:oy + ny - 1, ox:ox + nx - 1] |= cells
    return cells, nodes, M


def bake_slots_reference(nodes) -> np.ndarray:
    """The slot index of ct_network_bake_compact in numpy (include/cloudtrace.h, "the compact bake").  nodes: the mask's node
    bytes [Nz, Ny, Nx] -> uint32 of the same shape: 0 for an inactive node, 1 + r for the r-th active node in ascending node
    index (z Ny + y) Nx + x."""
    active = np.ascontiguousarray(nodes).reshape(-1) != 0
    slots = np.where(active, np.cumsum(active, dtype=np.uint64), 0).astype(np.uint32)
    return slots.reshape(np.shape(nodes))


def bake_directions_reference(info, probe_directions) -> np.ndarray:
    """The directions of a traced bake in numpy (include/cloudtrace.h, "the traced bake"): d(j, k) = c l + sqrt(1 - c^2) u_j with
    c = info["cosine"][k], in float64 from the float32 light info["light"] and the float32 probe directions u_j (the first
    `azimuths` rows of Bake.probes()[1]), rounded once to float32 -> [azimuths, cosines, 3]."""
    l = np.asarray(info["light"], np.float32).reshape(3).astype(np.float64)
    c = np.asarray(info["cosine"], np.float32).reshape(-1).astype(np.float64)
    u = np.ascontiguousarray(probe_directions, np.float32).reshape(-1, 3)[:int(info["azimuths"])].astype(np.float64)
    s = np.sqrt(1.0 - c * c)
    return (c[None, :, None] * l[None, None, :] + s[None, :, None] * u[:, None, :]).astype(np.float32)


def point_fold_reference(values_f32, mean=None, count: int = 0) -> np.ndarray:
    """The `radiance` of PointRadianceTask::addExperimentResult applied to values_f32[0], values_f32[1], ... (float32 [S, ...]) in
    order, every operation rounded to float32, newWeight = (float)(1.0 / (double)(float)N): what ct_point_radiance_launch and a
    traced bake store.  mean / count: the state to continue from (default: zeros, 0 experiments)."""
    f32 = np.float32
    v = np.ascontiguousarray(values_f32, f32)
    rad = np.zeros(v.shape[1:], f32) if mean is None else np.array(mean, f32)
    for k, x in enumerate(v):
        weight = f32(1.0 / np.float64(f32(count + k + 1)))
        rad = (rad + ((x - rad).astype(f32) * weight).astype(f32)).astype(f32)
    return rad


def point_fold_var_reference(values_f32, mean=None, m2=None, count=0):
    """PointRadianceTask::addExperimentResult applied to values_f32[0], values_f32[1], ... (float32 [S, ...]) in order, every
    operation rounded to float32: experimentCount++, N = (float)count, newWeight = (float)(1.0 / (double)N), newMean = mean +
    (x - mean) * newWeight, runningVariance += (x - mean) * (x - newMean) with the old mean in the first factor -- what
    ct_point_radiance_launch and an adaptive traced bake store.  mean / m2 / count: the state to continue from (default: zeros);
    count is one number or an integer array of the values' shape -> (mean, m2, count)."""
    f32 = np.float32
    v = np.ascontiguousarray(values_f32, f32)
    rad = np.zeros(v.shape[1:], f32) if mean is None else np.array(mean, f32)
    var = np.zeros(v.shape[1:], f32) if m2 is None else np.array(m2, f32)
    cnt = np.broadcast_to(np.asarray(count, np.int64), v.shape[1:]).copy()
    for x in v:
        cnt = cnt + 1
        weight = (1.0 / cnt.astype(f32).astype(np.float64)).astype(f32)
        previous = rad
        rad = (previous + ((x - previous).astype(f32) * weight).astype(f32)).astype(f32)
        var = (var + ((x - previous).astype(f32) * (x - rad).astype(f32)).astype(f32)).astype(f32)
    return rad, var, cnt


def point_converged_reference(mean, m2, count, rel_tol, abs_tol, zero_samples) -> np.ndarray:
    """The stopping rule of an adaptive traced bake (include/cloudtrace.h, "the adaptive traced bake"), which is
    RadianceCollector::update's test of a PointRadianceTask (PointRadianceTask.h:23-36, RadianceCollector.cpp:112-118) with its
    constants as parameters, in float32: absolute = (1.96f * sqrt(m2 / N)) / sqrt(N), relative = absolute / (mean + FLT_EPSILON),
    converged = relative < rel_tol or absolute < abs_tol, and where mean < FLT_EPSILON: converged = count > zero_samples.  A NaN
    compares false -> bool array."""
    f32 = np.float32
    eps = np.finfo(f32).eps
    rad, var = np.asarray(mean, f32), np.asarray(m2, f32)
    cnt = np.asarray(count, np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        N = cnt.astype(f32)
        absolute = (f32(1.96) * np.sqrt(var / N)) / np.sqrt(N)
        relative = absolute / (rad + eps)
        converged = (relative < f32(rel_tol)) | (absolute < f32(abs_tol))
        return np.where(rad < eps, cnt > int(zero_samples), converged)


# ---- bake files and half tables (include/cloudtrace.h, "bake files" and "half tables"), restated in numpy: no library call ----
BAKE_FILE_MAGIC = b"CTBAKE\r\n"
BAKE_FILE_VERSION = 1
BAKE_F32, BAKE_F16 = 0, 1

# The 256-byte header, little-endian, every field at the offset include/cloudtrace.h documents (CtBakeFileHeader).
bake_file_dtype = np.dtype({
    "names": ["magic", "version", "header_bytes", "kind", "format", "traced", "adaptive", "grid", "azimuths", "cosines", "margin_texels",
              "entries", "stored_entries", "active_nodes", "light", "axis_a", "axis_b", "dims", "sample_step_bits", "mean_free_path_bits",
              "cloud_size_bits", "estimator", "tex_fixed8", "light_color_bits", "light_intensity_bits", "samples", "volume_hash", "paths",
              "round_samples", "max_samples", "zero_samples", "rel_tol_bits", "abs_tol_bits", "rounds", "converged", "capped", "reserved"],
    "formats": ["S8", "<u4", "<u4", "<u4", "<u4", "<u4", "<u4", ("<u4", 3), "<u4", "<u4", "<u4",
                "<u8", "<u8", "<u8", ("<f4", 3), ("<f4", 3), ("<f4", 3), ("<u4", 3), "<u4", "<u4",
                "<u4", "<i4", "<u4", ("<u4", 3), "<u4", "<u4", "<u8", "<u8",
                "<u4", "<u4", "<u4", "<u4", "<u4", "<u4", "<u8", "<u8", ("u1", 32)],
    "offsets": [0, 8, 12, 16, 20, 24, 28, 32, 44, 48, 52,
                56, 64, 72, 80, 92, 104, 116, 128, 132,
                136, 140, 144, 148, 160, 164, 168, 176,
                184, 188, 192, 196, 200, 204, 208, 216, 224],
    "itemsize": 256,
})


def fnv1a64_reference(data: bytes) -> int:
    """FNV-1a 64 of `data`: the bake file's trailing checksum."""
    h = 0xCBF29CE484222325
    for byte in bytes(data):
        h = ((h ^ byte) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def volume_hash_reference(density) -> int:
    """The volume hash of a bake file: H = sum_i (t_i + 1) * ((i + 1) * 0x9E3779B97F4A7C15 mod 2^64) mod 2^64 over the level-0
    texels in linear order (x fastest), in uint64 arithmetic, which wraps."""
    t = np.ascontiguousarray(density, np.uint8).reshape(-1).astype(np.uint64)
    i = np.arange(1, t.size + 1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return int(np.sum((t + np.uint64(1)) * (i * np.uint64(0x9E3779B97F4A7C15)), dtype=np.uint64))


def half_round_reference(values_f32):
    """ct_bake_half's rounding: (bits, refused).  bits: uint16, numpy's float32 -> float16 conversion (nearest, ties to even,
    subnormals, the sign of zero); refused: bool, the values the call refuses -- NaN, infinite, or |v| >= 65520, which round to
    an infinity."""
    v = np.ascontiguousarray(values_f32, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        bits = v.astype(np.float16).view(np.uint16)
        refused = ~(np.abs(v) < np.float32(65520.0))
    return bits, refused


def _bake_file_sections(header):
    """-> {section: (offset, dtype, count)} and the checksum's offset, for a header record."""
    def pad(v, to=16):
        return (v + to - 1) // to * to
    at, out = 256, {}
    stored = int(header["stored_entries"])
    if int(header["kind"]) != 0:
        out["nodes"] = (at, np.dtype("u1"), int(np.prod(header["grid"].astype(np.uint64))))
        at += out["nodes"][2]
    at = pad(at)
    out["table"] = (at, np.dtype("<f2" if int(header["format"]) == BAKE_F16 else "<f4"), stored)
    at += stored * out["table"][1].itemsize
    if int(header["adaptive"]):
        at = pad(at)
        out["m2"] = (at, np.dtype("<f4"), stored)
        at = pad(at + 4 * stored)
        out["counts"] = (at, np.dtype("<u4"), stored)
        at += 4 * stored
    return out, pad(at, 8)


def write_bake_file_reference(header: dict, table, nodes=None, m2=None, counts=None) -> bytes:
    """The bytes of a bake file.  header: the fields of bake_file_dtype by name (missing ones are 0; magic, version and
    header_bytes are filled in); table: the stored table, float32, or uint16 binary16 bits for format 1; nodes: uint8 node bytes
    (sparse and compact kinds); m2 / counts: adaptive bakes."""
    h = np.zeros((), bake_file_dtype)
    h["magic"], h["version"], h["header_bytes"] = BAKE_FILE_MAGIC, BAKE_FILE_VERSION, 256
    for name, value in header.items():
        h[name] = value
    sections, end = _bake_file_sections(h)
    data = bytearray(end)
    data[:256] = h.tobytes()
    half = int(h["format"]) == BAKE_F16
    parts = {"nodes": (nodes, np.uint8), "table": (table, np.uint16 if half else np.float32), "m2": (m2, np.float32), "counts": (counts, np.uint32)}
    for name, (at, dtype, count) in sections.items():
        array, host = parts[name]
        raw = np.ascontiguousarray(array, host).reshape(-1)
        if raw.size != count:
            raise ValueError(f"write_bake_file_reference: {name} holds {raw.size} values, the header implies {count}")
        data[at:at + count * dtype.itemsize] = raw.astype(raw.dtype.newbyteorder("<")).tobytes()
    return bytes(data) + np.array(fnv1a64_reference(data), "<u8").tobytes()


def read_bake_file_reference(data: bytes) -> dict:
    """-> {"header": the bake_file_dtype record, "table" (float32, or uint16 bits for format 1), "nodes", "m2", "counts" (None where
    the file has no such section), "checksum"}.  ValueError for a wrong magic, version, length or checksum; the ranges are the
    library's to check (bake_file_info)."""
    data = bytes(data)
    if len(data) < 264:
        raise ValueError("shorter than a bake file's header and checksum")
    h = np.frombuffer(data, bake_file_dtype, 1)[0]
    if bytes(h["magic"]).ljust(8, b"\0") != BAKE_FILE_MAGIC or int(h["version"]) != BAKE_FILE_VERSION or int(h["header_bytes"]) != 256:
        raise ValueError("not a bake file of this version")
    sections, end = _bake_file_sections(h)
    if len(data) != end + 8:
        raise ValueError(f"{len(data)} bytes, the header implies {end + 8}")
    checksum = int(np.frombuffer(data, "<u8", 1, end)[0])
    if checksum != fnv1a64_reference(data[:end]):
        raise ValueError("wrong checksum")
    out = {"header": h, "nodes": None, "m2": None, "counts": None, "checksum": checksum}
    for name, (at, dtype, count) in sections.items():
        a = np.frombuffer(data, dtype, count, at)
        out[name] = a.view(np.uint16).copy() if dtype == np.dtype("<f2") else a.astype(dtype.newbyteorder("=")).copy()
    return out


def bake_file_info(path) -> dict:
    """ct_bake_file_info: a bake file read and checked without a device -> the header's fields by name (arrays as numpy arrays)
    and file_bytes, the sections' offsets and the checksum."""
    import os
    L = _lib.load()
    i = _lib.CtBakeFileInfo()
    check(L.ct_bake_file_info(os.fsencode(path), C.byref(i)), None)
    out = {}
    for name, ctype in i.header._fields_:
        v = getattr(i.header, name)
        out[name] = bytes(v) if name == "magic" else np.ctypeslib.as_array(v).copy() if hasattr(v, "__len__") else v
    for name, _ in i._fields_[1:]:
        out[name] = int(getattr(i, name))
    return out


@dataclass(frozen=True)
class AdaptiveParams:
    """CtBakeAdaptive: R experiments per live entry and round, the cap per entry (a multiple of R), and the stopping rule's
    tolerances; the defaults are the reference's (RadianceCollector.cpp:112-118)."""
    round_samples: int
    max_samples: int
    rel_tol: float = 2e-2
    abs_tol: float = 1e-4
    zero_samples: int = 100000


# The weight file: a 32-byte little-endian header -- magic "CTNW", u32 version, blocks, width, aux, head_layers, u64 weight
# count -- and then weight_count float32 values in the order of CtNetworkDesc.weights_host.
WEIGHT_MAGIC = b"CTNW"
WEIGHT_VERSION = 1
_WEIGHT_HEADER = "<4sIIIIIQ"


def save_weights(path, module_or_weights, shape: NetworkShape | None = None):
    """Writes a ScatterNet, or a flat weight array with its `shape`, as a weight file (read by load_weights and by
    `cloudtrace --network`)."""
    import struct
    if hasattr(module_or_weights, "blocks"):
        shape = module_or_weights.shape
        weights = pack_weights(module_or_weights)
    else:
        if shape is None:
            raise ValueError("save_weights: a flat weight array needs its NetworkShape")
        weights = np.ascontiguousarray(module_or_weights, np.float32).reshape(-1)
    if weights.size != shape.weight_count():
        raise ValueError(f"{weights.size} weights, the shapes imply {shape.weight_count()}")
    with open(path, "wb") as f:
        f.write(struct.pack(_WEIGHT_HEADER, WEIGHT_MAGIC, WEIGHT_VERSION, BLOCKS, shape.width, shape.aux, shape.head_layers, weights.size))
        f.write(weights.astype("<f4").tobytes())


def load_weights(path):
    """-> (flat float32 weights, NetworkShape).  ValueError for a file that is malformed: a wrong magic or version, a count
    that is not what the shapes imply, or fewer bytes than the header announces."""
    import struct
    with open(path, "rb") as f:
        data = f.read()
    n_head = struct.calcsize(_WEIGHT_HEADER)
    if len(data) < n_head:
        raise ValueError(f"{path}: shorter than the {n_head}-byte header of a weight file")
    magic, version, blocks, width, aux, head, count = struct.unpack(_WEIGHT_HEADER, data[:n_head])
    if magic != WEIGHT_MAGIC:
        raise ValueError(f"{path}: not a weight file (magic {magic!r})")
    if version != WEIGHT_VERSION:
        raise ValueError(f"{path}: weight file version {version}, this reader knows {WEIGHT_VERSION}")
    if blocks != BLOCKS or width < 16 or width > 256 or width % 8 or aux > 8 or not 1 <= head <= 4:
        raise ValueError(f"{path}: shapes out of range (blocks {blocks}, width {width}, aux {aux}, head layers {head})")
    shape = NetworkShape(width, aux, head)
    if count != shape.weight_count():
        raise ValueError(f"{path}: {count} weights, the shapes imply {shape.weight_count()}")
    if len(data) - n_head != 4 * count:
        raise ValueError(f"{path}: {len(data) - n_head} bytes of weights, {count} weights need {4 * count}")
    return np.frombuffer(data, "<f4", count, n_head).astype(np.float32), shape


class Network:
    """A CtNetwork on `tracer`'s device (ct_network_create).  `module_or_weights`: a ScatterNet, or the flat array with
    width / aux / head_layers given.  Close it before the tracer."""

    def __init__(self, tracer, module_or_weights, width: int | None = None, aux: int | None = None, head_layers: int | None = None):
        self.L = _lib.load()
        self.tracer = tracer
        if hasattr(module_or_weights, "blocks"):
            self.shape = module_or_weights.shape
            weights = pack_weights(module_or_weights)
        else:
            self.shape = NetworkShape(*(d if v is None else int(v) for v, d in zip((width, aux, head_layers), (200, 1, 3))))
            weights = np.ascontiguousarray(module_or_weights, np.float32).reshape(-1)
        d = _lib.CtNetworkDesc(_lib.CT_ABI_VERSION, BLOCKS, self.shape.width, self.shape.aux, self.shape.head_layers,
                               weights.ctypes.data_as(C.c_void_p), weights.size)
        n = C.c_void_p()
        check(self.L.ct_network_create(tracer.h, C.byref(d), C.byref(n)), tracer.h)
        self.n = n

    def close(self):
        if getattr(self, "n", None):
            self.L.ct_network_destroy(self.n)
            self.n = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def eval(self, descriptors_dev_ptr: int, aux_dev_ptr: int | None, count: int, out_dev_ptr: int):
        """ct_network_eval on raw device pointers: count records of 2250 bytes, count * A floats (None when A == 0), count floats out."""
        check(self.L.ct_network_eval(self.tracer.h, self.n, C.c_void_p(descriptors_dev_ptr), C.c_void_p(aux_dev_ptr) if aux_dev_ptr else None,
                                     count, C.c_void_p(out_dev_ptr)), self.tracer.h)

    def time_ms(self) -> float:
        """GPU milliseconds of the last eval (ct_debug_network_time)."""
        ms = C.c_double(0)
        rc = self.L.ct_debug_network_time(self.n, C.byref(ms))
        if rc != _lib.CT_OK:
            raise _lib.CloudTraceError(rc, "ct_debug_network_time")
        return float(ms.value)


class Bake:
    """A CtBake of `net` on its tracer (ct_network_bake): the network evaluated on a grid of grid[0] x grid[1] x grid[2] position
    nodes x `azimuths` view azimuths around the light x `cosines` polar nodes, which CloudTracer.baked_render_* interpolate in
    place of gather and network.  sparse: ct_network_bake_sparse, which bakes only the probes a flight can reach and leaves the
    rest of the table 0.  compact: ct_network_bake_compact, the sparse bake with only the active nodes stored, behind a slot index.
    Close it before the tracer; after tracer.set_light call update().
    net=None with samples=S: a traced bake (ct_bake_traced) of the same kind, whose entries are the means of S experiments of
    the path tracer's point estimator instead of a network's outputs; trace_more() refines it, retrace() follows a new light.
    net=None with adaptive=AdaptiveParams(...) (or a dict of its fields): an adaptive traced bake (ct_bake_traced_adaptive), traced
    in rounds until every entry passes the stopping rule or holds max_samples experiments; counts() and m2() are its per-entry
    experiment counts and sums of squared deviations, trace_adaptive_more() raises the cap, retrace_adaptive() follows a new light."""

    def __init__(self, tracer, net, grid, azimuths: int, cosines: int, sparse: bool = False, compact: bool = False, samples: int | None = None,
                 adaptive: "AdaptiveParams | dict | None" = None):
        if sparse and compact:
            raise ValueError("a bake is sparse or compact, not both")
        if net is not None and (samples is not None or adaptive is not None):
            raise ValueError("a bake holds a network's outputs (net) or traced radiance (net=None, samples=... or adaptive=...), not both")
        if samples is not None and adaptive is not None:
            raise ValueError("a traced bake takes samples=... (uniform) or adaptive=... (rounds under the stopping rule), not both")
        if net is None and samples is None and adaptive is None:
            raise ValueError("a bake needs a network, or net=None and samples=... or adaptive=... for a traced bake")
        if isinstance(adaptive, dict):
            adaptive = AdaptiveParams(**adaptive)
        self.L = _lib.load()
        self.tracer = tracer
        d = _lib.CtBakeDesc(_lib.CT_ABI_VERSION, (C.c_uint32 * 3)(*[int(v) for v in grid]), int(azimuths), int(cosines))
        b = C.c_void_p()
        kind = _lib.CT_BAKE_COMPACT if compact else _lib.CT_BAKE_SPARSE if sparse else _lib.CT_BAKE_DENSE
        if adaptive is not None:
            p = _lib.CtBakeAdaptive(_lib.CT_ABI_VERSION, int(adaptive.round_samples), int(adaptive.max_samples), int(adaptive.zero_samples),
                                    float(adaptive.rel_tol), float(adaptive.abs_tol))
            check(self.L.ct_bake_traced_adaptive(tracer.h, C.byref(d), kind, C.byref(p), C.byref(b)), tracer.h)
        elif net is None:
            check(self.L.ct_bake_traced(tracer.h, C.byref(d), kind, int(samples), C.byref(b)), tracer.h)
        else:
            entry = self.L.ct_network_bake_compact if compact else self.L.ct_network_bake_sparse if sparse else self.L.ct_network_bake
            check(entry(tracer.h, net.n, C.byref(d), C.byref(b)), tracer.h)
        self.b = b

    @classmethod
    def _adopt(cls, tracer, handle) -> "Bake":
        """A Bake around a CtBake the library has made another way (ct_bake_load, ct_bake_half)."""
        self = cls.__new__(cls)
        self.L = _lib.load()
        self.tracer = tracer
        self.b = handle
        return self

    @classmethod
    def load(cls, tracer, path) -> "Bake":
        """ct_bake_load: the bake a file holds, on `tracer`, which must hold the cloud and estimator the file was made on."""
        import os
        b = C.c_void_p()
        check(_lib.load().ct_bake_load(tracer.h, os.fsencode(path), C.byref(b)), tracer.h)
        return cls._adopt(tracer, b)

    @classmethod
    def traced_shard(cls, tracer, grid, azimuths: int, cosines: int, shard: int, shards: int, samples: int = 0,
                     adaptive: "AdaptiveParams | None" = None, sparse: bool = False, compact: bool = False) -> "Bake":
        """ct_debug_bake_shard: what shard `shard` of `shards` traces of a bake on a group, alone on `tracer` -- for timing it."""
        d = _lib.CtBakeDesc(_lib.CT_ABI_VERSION, (C.c_uint32 * 3)(*[int(v) for v in grid]), int(azimuths), int(cosines))
        kind = _lib.CT_BAKE_COMPACT if compact else _lib.CT_BAKE_SPARSE if sparse else _lib.CT_BAKE_DENSE
        p = None
        if adaptive is not None:
            p = C.byref(_lib.CtBakeAdaptive(_lib.CT_ABI_VERSION, int(adaptive.round_samples), int(adaptive.max_samples), int(adaptive.zero_samples),
                                            float(adaptive.rel_tol), float(adaptive.abs_tol)))
        b = C.c_void_p()
        check(_lib.load().ct_debug_bake_shard(tracer.h, C.byref(d), kind, int(samples), p, int(shard), int(shards), C.byref(b)), tracer.h)
        return cls._adopt(tracer, b)

    def save(self, path):
        """ct_bake_save: this bake, of any kind and format, as a bake file (written under a temporary name and renamed)."""
        import os
        check(self.L.ct_bake_save(self.b, os.fsencode(path)), self.tracer.h)

    def half(self) -> "Bake":
        """ct_bake_half: a NEW bake of the same kind, grid, frame and mask whose stored table is binary16 (each value rounded to
        nearest, ties to even).  CloudTraceError (CT_E_INVAL) when a value is not finite or rounds to an infinity.  A half bake
        is final: it renders and saves, and nothing bakes or traces into it."""
        b = C.c_void_p()
        check(self.L.ct_bake_half(self.tracer.h, self.b, C.byref(b)), self.tracer.h)
        return Bake._adopt(self.tracer, b)

    @property
    def format(self) -> int:
        """ct_bake_format: 0 (CT_BAKE_F32) or 1 (CT_BAKE_F16)."""
        f = C.c_uint32(0)
        check(self.L.ct_bake_format(self.b, C.byref(f)), self.tracer.h)
        return int(f.value)

    def half_table(self) -> np.ndarray:
        """ct_bake_download_half -> uint16, the stored binary16 bits of a half bake, shaped as counts() / stored_table()."""
        return self._stored_array(self.L.ct_bake_download_half, np.uint16)

    def close(self):
        if getattr(self, "b", None):
            self.L.ct_bake_destroy(self.b)
            self.b = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def update(self, net):
        """ct_bake_update: bake again in place, for the tracer's light as it is now and for `net`."""
        check(self.L.ct_bake_update(self.tracer.h, net.n, self.b), self.tracer.h)

    def trace_more(self, samples: int):
        """ct_bake_trace_more: `samples` more experiments per entry of a traced bake, folded behind those it holds."""
        check(self.L.ct_bake_trace_more(self.tracer.h, self.b, int(samples)), self.tracer.h)

    def retrace(self, samples: int):
        """ct_bake_retrace: a traced bake again from experiment 1, for the tracer's light as it is now."""
        check(self.L.ct_bake_retrace(self.tracer.h, self.b, int(samples)), self.tracer.h)

    def trace_info(self) -> dict:
        """ct_bake_trace_info: traced, samples, paths, trace_ms, fold_ms (a network's bake: all zero)."""
        i = _lib.CtBakeTraceInfo()
        check(self.L.ct_bake_trace_info(self.b, C.byref(i)), self.tracer.h)
        return {"traced": bool(i.traced), "samples": int(i.samples), "paths": int(i.paths), "trace_ms": float(i.trace_ms),
                "fold_ms": float(i.fold_ms)}

    def trace_adaptive_more(self, max_samples: int):
        """ct_bake_trace_adaptive_more: raise an adaptive bake's cap and go on with the entries that stopped at the old one."""
        check(self.L.ct_bake_trace_adaptive_more(self.tracer.h, self.b, int(max_samples)), self.tracer.h)

    def retrace_adaptive(self):
        """ct_bake_retrace_adaptive: an adaptive bake again from experiment 1, for the tracer's light as it is now."""
        check(self.L.ct_bake_retrace_adaptive(self.tracer.h, self.b), self.tracer.h)

    def adaptive_info(self) -> dict:
        """ct_bake_adaptive_info: adaptive, the parameters with the cap in force, rounds, entries_active, converged, capped, paths,
        trace_ms, fold_ms, test_ms (any other bake: all zero)."""
        i = _lib.CtBakeAdaptiveInfo()
        check(self.L.ct_bake_adaptive_info(self.b, C.byref(i)), self.tracer.h)
        out = {n: getattr(i, n) for n, _ in i._fields_ if n != "reserved"}
        out["adaptive"] = bool(i.adaptive)
        return out

    def counts(self) -> np.ndarray:
        """ct_bake_download_counts -> uint32, the experiments every entry holds, as stored: [Nz, Ny, Nx, azimuths, cosines], or
        (compact) [slots, azimuths, cosines] like stored_table()."""
        return self._stored_array(self.L.ct_bake_download_counts, np.uint32)

    def m2(self) -> np.ndarray:
        """ct_bake_download_m2 -> float32, every entry's sum of squared deviations (runningVariance), shaped as counts()."""
        return self._stored_array(self.L.ct_bake_download_m2, np.float32)

    def _stored_array(self, entry, dtype) -> np.ndarray:
        i, st = self.info, self.storage_info
        a = np.empty(st["stored_entries"], dtype)
        check(entry(self.b, a.ctypes.data_as(C.c_void_p), a.size), self.tracer.h)
        if st["compact"]:
            return a.reshape(-1, i["azimuths"], i["cosines"])
        nx, ny, nz = i["grid"]
        return a.reshape(nz, ny, nx, i["azimuths"], i["cosines"])

    def directions(self) -> np.ndarray:
        """ct_bake_directions -> float32 [azimuths, cosines, 3]: d(j, k), the direction a traced bake's entry (j, k) stands for."""
        i = self.info
        d = np.empty((i["azimuths"], i["cosines"], 3), np.float32)
        check(self.L.ct_bake_directions(self.b, d.ctypes.data_as(C.c_void_p), d.size), self.tracer.h)
        return d

    @property
    def info(self) -> dict:
        """ct_bake_info: grid, azimuths, cosines, entries, light, axis_a, axis_b (float32 [3]), cosine (float32 [cosines]),
        current, gather_ms, network_ms."""
        i = _lib.CtBakeInfo()
        check(self.L.ct_bake_info(self.b, C.byref(i)), self.tracer.h)
        return {"grid": tuple(int(v) for v in i.grid), "azimuths": int(i.azimuths), "cosines": int(i.cosines), "entries": int(i.entries),
                "light": np.array(i.light[:], np.float32), "axis_a": np.array(i.axis_a[:], np.float32),
                "axis_b": np.array(i.axis_b[:], np.float32), "cosine": np.array(i.cosine[:int(i.cosines)], np.float32),
                "current": bool(i.current), "gather_ms": float(i.gather_ms), "network_ms": float(i.network_ms)}

    @property
    def sparse_info(self) -> dict:
        """ct_bake_sparse_info: sparse, margin_texels (M), nodes, active_nodes, probes_baked, mask_ms."""
        i = _lib.CtBakeSparseInfo()
        check(self.L.ct_bake_sparse_info(self.b, C.byref(i)), self.tracer.h)
        return {"sparse": bool(i.sparse), "margin_texels": int(i.margin_texels), "nodes": int(i.nodes),
                "active_nodes": int(i.active_nodes), "probes_baked": int(i.probes_baked), "mask_ms": float(i.mask_ms)}

    def mask(self) -> np.ndarray:
        """ct_bake_mask -> uint8 [Nz, Ny, Nx]: 1 where the node's probes were baked (a dense bake: everywhere)."""
        nx, ny, nz = self.info["grid"]
        m = np.empty((nz, ny, nx), np.uint8)
        check(self.L.ct_bake_mask(self.b, m.ctypes.data_as(C.c_void_p), m.size), self.tracer.h)
        return m

    @property
    def storage_info(self) -> dict:
        """ct_bake_storage_info: compact, slots, stored_entries, table_bytes, index_bytes."""
        i = _lib.CtBakeStorageInfo()
        check(self.L.ct_bake_storage_info(self.b, C.byref(i)), self.tracer.h)
        return {"compact": bool(i.compact), "slots": int(i.slots), "stored_entries": int(i.stored_entries),
                "table_bytes": int(i.table_bytes), "index_bytes": int(i.index_bytes)}

    def slots(self) -> np.ndarray:
        """ct_bake_slots -> uint32 [Nz, Ny, Nx]: the node's block in stored_table(), 0 for an inactive node (compact bakes only)."""
        nx, ny, nz = self.info["grid"]
        s = np.empty((nz, ny, nx), np.uint32)
        check(self.L.ct_bake_slots(self.b, s.ctypes.data_as(C.c_void_p), s.size), self.tracer.h)
        return s

    def stored_table(self) -> np.ndarray:
        """ct_bake_download_stored -> float32 [slots, azimuths, cosines]: the zero block, then the blocks of the active nodes in
        ascending node index (compact bakes only)."""
        i, st = self.info, self.storage_info
        t = np.empty(st["stored_entries"], np.float32)
        check(self.L.ct_bake_download_stored(self.b, t.ctypes.data_as(C.c_void_p), t.size), self.tracer.h)
        return t.reshape(-1, i["azimuths"], i["cosines"])

    def probes(self, first: int = 0, count: int | None = None):
        """ct_bake_probes -> (positions, directions) float32 [count, 3], the records the bake used, in index order."""
        if count is None:
            i = self.info
            count = i["entries"] // i["cosines"] - first
        pos, d = np.empty((count, 3), np.float32), np.empty((count, 3), np.float32)
        check(self.L.ct_bake_probes(self.b, first, count, pos.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p)), self.tracer.h)
        return pos, d

    def table(self) -> np.ndarray:
        """ct_bake_download -> float32 [Nz, Ny, Nx, azimuths, cosines], the raw network outputs."""
        i = self.info
        t = np.empty(i["entries"], np.float32)
        check(self.L.ct_bake_download(self.b, t.ctypes.data_as(C.c_void_p), t.size), self.tracer.h)
        nx, ny, nz = i["grid"]
        return t.reshape(nz, ny, nx, i["azimuths"], i["cosines"])


def bake_spans_reference(active: int, shards: int) -> np.ndarray:
    """The split of a bake on a group (include/cloudtrace.h, "bakes on a group") in numpy: `active` = the nodes a build covers
    (every node of a dense bake, the active nodes in the list's order otherwise); shard i of `shards` owns the list positions
    [floor(i A / n), floor((i + 1) A / n)) -> uint64 [shards, 2]."""
    A, n = int(active), int(shards)
    if A < 0 or n < 1:
        raise ValueError("bake_spans_reference: active >= 0 and shards >= 1")
    return np.array([[i * A // n, (i + 1) * A // n] for i in range(n)], np.uint64).reshape(n, 2)


class _ShardTracer:
    """What a Bake needs of its tracer, for a shard's handle that a TracerGroup owns."""

    def __init__(self, h):
        self.h = h


class _BakeView(Bake):
    """A Bake around a CtBake that a GroupBake owns: every accessor and save() work, close() only lets go of it."""

    def close(self):
        self.b = None


class GroupBake:
    """A CtGroupBake on a TracerGroup (ct_group_bake_*): one CtBake per shard.  Every build cuts the bake's nodes into one span
    per shard (bake_spans_reference), every shard bakes or traces its span, and copies leave every shard with the whole bake,
    which is the single-GPU bake bit for bit.  Made by TracerGroup.network_bake / traced_bake / traced_bake_adaptive / load_bake;
    closed with, or before, its group.  shard(i) is shard i's bake as a network.Bake view: table(), counts(), info, save(), ..."""

    def __init__(self, group, gb):
        self.L, self.group, self.gb = group.L, group, gb
        group.__dict__.setdefault("_bakes", []).append(self)

    def close(self):
        if getattr(self, "gb", None):
            self.L.ct_group_bake_destroy(self.gb)
            self.gb = None
            if self in getattr(self.group, "_bakes", []):
                self.group._bakes.remove(self)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def shard(self, index: int) -> Bake:
        """ct_group_bake_shard -> a Bake view of shard `index`'s bake (owned by this GroupBake; do not change it through the view)."""
        b, h = C.c_void_p(), C.c_void_p()
        self.group._check(self.L.ct_group_bake_shard(self.gb, index, C.byref(b)))
        self.group._check(self.L.ct_group_handle(self.group.g, index, C.byref(h)))
        return _BakeView._adopt(_ShardTracer(h), b)

    def spans(self) -> np.ndarray:
        """ct_group_bake_spans -> uint64 [shards, 2]: lo and hi of every shard, node-list positions."""
        n = C.c_uint32(0)
        self.group._check(self.L.ct_group_size(self.group.g, C.byref(n)))
        out = np.zeros((int(n.value), 2), np.uint64)
        self.group._check(self.L.ct_group_bake_spans(self.gb, out.ctypes.data_as(C.c_void_p), out.size))
        return out

    def update(self, net):
        """ct_group_bake_update: bake again for the group's light as it is now (TracerGroup.set_light) and the GroupNetwork `net`."""
        self.group._check(self.L.ct_group_bake_update(self.gb, net.gn if net is not None else None))

    def trace_more(self, samples: int):
        """ct_group_bake_trace_more: Bake.trace_more on the group."""
        self.group._check(self.L.ct_group_bake_trace_more(self.gb, int(samples)))

    def retrace(self, samples: int):
        """ct_group_bake_retrace: Bake.retrace on the group."""
        self.group._check(self.L.ct_group_bake_retrace(self.gb, int(samples)))

    def trace_adaptive_more(self, max_samples: int):
        """ct_group_bake_trace_adaptive_more: Bake.trace_adaptive_more on the group."""
        self.group._check(self.L.ct_group_bake_trace_adaptive_more(self.gb, int(max_samples)))

    def retrace_adaptive(self):
        """ct_group_bake_retrace_adaptive: Bake.retrace_adaptive on the group."""
        self.group._check(self.L.ct_group_bake_retrace_adaptive(self.gb))

    def save(self, path, shard: int = 0):
        """ct_bake_save of shard `shard`'s bake: every shard holds the whole bake, so any shard's file is the bake's."""
        self.shard(shard).save(path)

    def exchange_info(self) -> dict:
        """ct_debug_group_bake_exchange: bytes copied between shards by the last exchange and its host milliseconds."""
        n, ms = C.c_uint64(0), C.c_double(0)
        self.group._check(self.L.ct_debug_group_bake_exchange(self.gb, C.byref(n), C.byref(ms)))
        return {"bytes": int(n.value), "ms": float(ms.value)}
