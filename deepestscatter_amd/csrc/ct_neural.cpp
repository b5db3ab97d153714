// ct_neural.cpp -- the first-scatter and network path of the C ABI: the density pyramid and the descriptor gather
// (ct_collect_descriptors, ct_descriptor_frame), the scattering network (ct_network_create, ct_network_eval) and the network as a
// renderer (ct_network_render_*, and ct_baked_render_* from a bake's probe table), on the handle of ct_handle.hpp.  The network
// itself is ct_network.hip.  The bakes -- what fills, refills, saves and loads a probe table -- are ct_bake.cpp; ct_bake.hpp
// declares the three things the renderer needs of a bake and the helpers of this file that a bake needs.
#include <cmath>

#include "ct_bake.hpp"
#include "ct_network.hpp"

DescriptorScale ct::descriptor_scale(CtHandle h)
{
    const float maxs = (float)std::max(h->scene.dims[0], std::max(h->scene.dims[1], h->scene.dims[2]));
    const float voxel_m = h->scene.cloud_size_m / maxs;
    const float voxel_fp = voxel_m / h->scene.mean_free_path_m;
    const float level0 = -ct_log2f(voxel_fp) - 1;
    return { level0, voxel_m };
}

// Resources::generateMipmaps (Resources.cpp:169-209) on the device: levels = floor(log2(maxDim)) + 1.
int ct::ensure_pyramid(CtHandle h)
{
    if (h->d_pyramid) {
        return CT_OK;
    }
    const uint32_t nx = h->scene.dims[0], ny = h->scene.dims[1], nz = h->scene.dims[2];
    uint32_t m = std::max(nx, std::max(ny, nz)), levels = 1;
    while (m /= 2) {
        levels++;
    }
    if (levels > (uint32_t)kMaxMipLevels) {
        return fail(h, CT_E_INVAL, "volume too large for the mip pyramid");
    }
    MipPyramid mp{};
    mp.levels = levels;
    size_t total = 0;
    for (uint32_t l = 0; l < levels; l++) {
        mp.nx[l] = (int32_t)std::max(1u, nx >> l);
        mp.ny[l] = (int32_t)std::max(1u, ny >> l);
        mp.nz[l] = (int32_t)std::max(1u, nz >> l);
        mp.offset[l] = (uint32_t)total;
        total += (size_t)mp.nx[l] * mp.ny[l] * mp.nz[l];
    }
    if (total >= (1ull << 32)) {
        return fail(h, CT_E_INVAL, "volume too large for the mip pyramid");
    }
    HIPCHK(h, h->d_pyramid.alloc(total));
    HIPCHK(h, hipMemcpyAsync(h->d_pyramid, h->d_density, (size_t)nx * ny * nz, hipMemcpyDeviceToDevice, h->stream));
    for (uint32_t l = 1; l < levels; l++) {
        HIPCHK(h, launch_mip_level(h->d_pyramid + mp.offset[l - 1], mp.nx[l - 1], mp.ny[l - 1], mp.nz[l - 1],
                                   h->d_pyramid + mp.offset[l], mp.nx[l], mp.ny[l], mp.nz[l], h->stream));
    }
    mp.base = h->d_pyramid;
    h->pyramid = mp;
    return CT_OK;
}

extern "C" int ct_collect_descriptors(CtHandle h, const float *positions_host, const float *directions_host,
                                      uint32_t count, uint8_t *descriptors_host_out)
{
    NEED(h);
    if (!positions_host || !directions_host || !descriptors_host_out || count == 0 || count > (1u << 20)) {
        return fail(h, CT_E_INVAL, "ct_collect_descriptors: need 1..2^20 samples, two input arrays and an output array");
    }
    const int prc = ensure_pyramid(h);
    if (prc != CT_OK) {
        return prc;
    }
    const DescriptorScale ds = descriptor_scale(h);
    DevBuf<float> d_pos, d_dir;
    DevBuf<uint8_t> d_out;
    return drained(h, [&]() -> int {
        HIPCHK(h, d_pos.alloc(3 * (size_t)count));
        HIPCHK(h, d_dir.alloc(3 * (size_t)count));
        HIPCHK(h, d_out.alloc((size_t)count * CT_DESCRIPTOR_BYTES));
        HIPCHK(h, hipMemcpyAsync(d_pos, positions_host, 3 * (size_t)count * sizeof(float), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(d_dir, directions_host, 3 * (size_t)count * sizeof(float), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, launch_descriptors(h->dev, h->pyramid, d_pos, d_dir, count, ds.level0, ds.voxel_m, h->scene.cloud_size_m,
                                     d_out, h->stream));
        HIPCHK(h, hipMemcpyAsync(descriptors_host_out, d_out, (size_t)count * CT_DESCRIPTOR_BYTES, hipMemcpyDeviceToHost,
                                 h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return CT_OK;
    });
}

// A band's first flights, the scan of their counts and the compacting write (at most `capacity` records), timed into *ms_sum,
// then the band's record count: one 4-byte read and the wait for it.  No band counts more records than it has pixels.
static int flights_counted(CtHandle h, const PixelBand &band, const FlightTemps &t, uint32_t subframe_id, uint32_t capacity, float *pos,
                           float *dir, uint32_t *pixels, double *ms_sum, uint32_t *count_out)
{
    const uint32_t n_pad = (band.n + 255u) / 256u * 256u;
    const int rc = timed(h, ms_sum, [&]() -> int {
        HIPCHK(h, launch_first_scatter_frame(h->dev, band, t, subframe_id, capacity, pos, dir, pixels, h->stream));
        return CT_OK;
    }, t.waves + n_pad / 64u, count_out);
    if (rc == CT_OK && *count_out > band.n) {
        return fail(h, CT_E_HIP, "internal: a band of %u pixels counted %u records", band.n, *count_out);
    }
    return rc;
}

extern "C" int ct_descriptor_frame(CtHandle h, uint32_t subframe_id, const uint32_t rect[4], uint32_t capacity,
                                   uint8_t *descriptors_dev, float *positions_dev, float *directions_dev, uint32_t *pixels_dev,
                                   uint32_t *count_out)
{
    NEED(h);
    if (!descriptors_dev || !count_out) {
        return fail(h, CT_E_INVAL, "ct_descriptor_frame: need a descriptor array and count_out");
    }
    *count_out = 0;
    if (!h->camera_set) {
        return fail(h, CT_E_STATE, "ct_set_camera has not been called");
    }
    const uint32_t W = h->scene.width, H = h->scene.height;
    const uint32_t x0 = rect ? rect[0] : 0u, y0 = rect ? rect[1] : 0u, x1 = rect ? rect[2] : W, y1 = rect ? rect[3] : H;
    if (x0 >= x1 || y0 >= y1 || x1 > W || y1 > H || (uint64_t)(x1 - x0) * (y1 - y0) > (1ull << 20)) {
        return fail(h, CT_E_INVAL, "ct_descriptor_frame: the rect must be non-empty, inside the %u x %u frame and of at most 2^20 pixels", W, H);
    }
    const uint32_t rw = x1 - x0, n = rw * (y1 - y0), n_pad = (n + 255u) / 256u * 256u;
    const DescriptorScale ds = descriptor_scale(h);
    DevBuf<float4> d_found;
    DevBuf<uint32_t> d_waves;
    DevBuf<float> d_pos, d_dir;
    h->dframe_scatter_ms = h->dframe_gather_ms = 0;
    return drained(h, [&]() -> int {
        // every temporary before any kernel
        const size_t held = std::max<size_t>(1, std::min<size_t>(capacity, n));   // records the compacting write can produce
        HIPCHK(h, d_found.alloc(n_pad));
        HIPCHK(h, d_waves.alloc(n_pad / 64u + 1u));
        if (!positions_dev) {
            HIPCHK(h, d_pos.alloc(3 * held));
        }
        if (!directions_dev) {
            HIPCHK(h, d_dir.alloc(3 * held));
        }
        const int prc = ensure_pyramid(h);
        if (prc != CT_OK) {
            return prc;
        }
        float *pos = positions_dev ? positions_dev : d_pos.get(), *dir = directions_dev ? directions_dev : d_dir.get();
        uint32_t count = 0;
        const int rc = flights_counted(h, rect_band(x0, y0, rw, y1 - y0), { d_found, d_waves, nullptr }, subframe_id, capacity, pos, dir,
                                       pixels_dev, &h->dframe_scatter_ms, &count);
        if (rc != CT_OK) {
            return rc;
        }
        *count_out = count;
        if (count > capacity) {
            return fail(h, CT_E_INVAL, "ct_descriptor_frame: %u valid pixels do not fit a capacity of %u", count, capacity);
        }
        if (count == 0) {
            return CT_OK;
        }
        return timed(h, &h->dframe_gather_ms, [&]() -> int {   // (the host's look at the count is no part of the gather)
            HIPCHK(h, launch_descriptors(h->dev, h->pyramid, pos, dir, count, ds.level0, ds.voxel_m, h->scene.cloud_size_m,
                                         descriptors_dev, h->stream));
            return CT_OK;
        });
    });
}

extern "C" int ct_debug_descriptor_frame_time(CtHandle h, double *first_scatter_ms_out, double *gather_ms_out)
{
    NEED_NOFLUSH(h);
    if (first_scatter_ms_out) {
        *first_scatter_ms_out = h->dframe_scatter_ms;
    }
    if (gather_ms_out) {
        *gather_ms_out = h->dframe_gather_ms;
    }
    return CT_OK;
}

// The scattering network (ct_network.hip): the handle's part is the device, the stream and the wait for batches in flight.
extern "C" int ct_network_create(CtHandle h, const CtNetworkDesc *d, CtNetwork *out)
{
    if (!h) {
        return fail(nullptr, CT_E_INVAL, "null handle");
    }
    char err[256] = "";
    int rc = ct::network_validate(d, out, err, sizeof err);   // (before the handle's device is touched)
    if (rc != CT_OK) {
        return fail(h, rc, "%s", err);
    }
    NEED(h);
    rc = ct::network_create(h->device, d, out, err, sizeof err);
    return rc == CT_OK ? CT_OK : fail(h, rc, "%s", err);
}

extern "C" int ct_network_eval(CtHandle h, CtNetwork n, const uint8_t *descriptors_dev, const float *aux_dev, uint32_t count,
                               float *out_dev)
{
    NEED(h);
    if (!n) {
        return fail(h, CT_E_INVAL, "ct_network_eval: null network");
    }
    if (ct::network_device(n) != h->device) {
        return fail(h, CT_E_INVAL, "ct_network_eval: the network lives on device %d, the handle on device %d", ct::network_device(n),
                    h->device);
    }
    char err[256] = "";
    const int rc = ct::network_eval(n, h->stream, descriptors_dev, aux_dev, count, out_dev, err, sizeof err);
    return rc == CT_OK ? CT_OK : fail(h, rc, "%s", err);
}

// ---- what the renderer (ct_network_render_*, ct_baked_render_*) and the bake share: checks and the handle's scratch ----------
// The checks touch nothing of the handle.
static int net_validate_params(CtHandle h, const CtNetworkRender *p, const char *who)
{
    if (p->abi_version != CT_ABI_VERSION) {
        return fail(h, CT_E_INVAL, "%s: abi_version %u, this library is %u", who, p->abi_version, CT_ABI_VERSION);
    }
    const int32_t out_transform = p->transform & ~CT_NET_ADD_SINGLE_SCATTER;
    if (out_transform != CT_NET_OUT_LINEAR && out_transform != CT_NET_OUT_EXPM1) {
        return fail(h, CT_E_INVAL, "%s: unknown output transform %d (CT_NET_OUT_LINEAR or CT_NET_OUT_EXPM1, with or without "
                                   "CT_NET_ADD_SINGLE_SCATTER)", who, p->transform);
    }
    if (!std::isfinite(p->rgb_scale[0]) || !std::isfinite(p->rgb_scale[1]) || !std::isfinite(p->rgb_scale[2])) {
        return fail(h, CT_E_INVAL, "%s: rgb_scale is not finite", who);
    }
    return CT_OK;
}

int ct::net_validate_network(CtHandle h, CtNetwork n, const char *who)
{
    if (ct::network_aux_inputs(n) != 1u) {
        return fail(h, CT_E_INVAL, "%s: the renderer feeds one aux input (the light angle); this network has %u", who,
                    ct::network_aux_inputs(n));
    }
    if (ct::network_device(n) != h->device) {
        return fail(h, CT_E_INVAL, "%s: the network lives on device %d, the handle on device %d", who, ct::network_device(n), h->device);
    }
    return CT_OK;
}

static int net_validate_shards(CtHandle h, const char *who, bool shards, const char *family)
{
    if (!shards && h->scene.shard_count > 1u) {
        return fail(h, CT_E_INVAL, "%s: this handle renders shard %u of %u; a shard's network frame is %s_shard_subframe / "
                                   "%s_shard_accumulate", who, h->scene.shard_index, h->scene.shard_count, family, family);
    }
    return CT_OK;
}

size_t ct::net_descriptor_limit(CtHandle h)
{
    return (size_t)knob_int(h->tune.NET_DESC_RECORDS, 1, 1 << 20, 1 << 20);
}

int ct::net_reserve(CtHandle h, size_t band_pixels, bool direct, bool hybrid)
{
    CtHandle_::NetScratch &s = h->net;
    const size_t n_pad = (band_pixels + 255u) / 256u * 256u;
    // (allocate, then swap, here and in net_grow_descriptors)
    if (hybrid && n_pad > s.omega.capacity()) {
        DevBuf<float4> omega;
        HIPCHK(h, omega.alloc(n_pad));
        s.omega = std::move(omega);
    }
    if (direct && n_pad > s.direct.capacity()) {
        DevBuf<float4> sun;
        HIPCHK(h, sun.alloc(n_pad));
        s.direct = std::move(sun);
    }
    if (n_pad > s.band_cap) {
        DevBuf<float4> found;
        DevBuf<uint32_t> waves;
        DevBuf<float> pos, dir, aux, out;
        HIPCHK(h, found.alloc(n_pad));
        HIPCHK(h, waves.alloc(n_pad / 64u + 1u));
        HIPCHK(h, pos.alloc(3 * n_pad));
        HIPCHK(h, dir.alloc(3 * n_pad));
        HIPCHK(h, aux.alloc(n_pad));
        HIPCHK(h, out.alloc(n_pad));
        s.found = std::move(found);
        s.waves = std::move(waves);
        s.pos = std::move(pos);
        s.dir = std::move(dir);
        s.aux = std::move(aux);
        s.out = std::move(out);
        s.band_cap = n_pad;
    }
    if (!s.desc) {
        // (CT_NET_DESC_RECORDS: the array never holds more records than this -- what a device without room for the growth leaves
        // a handle with, for the test that runs a band in pieces)
        const size_t first = std::min<size_t>(std::min<size_t>(n_pad, 4096), net_descriptor_limit(h));
        HIPCHK(h, s.desc.alloc(first * CT_DESCRIPTOR_BYTES));
    }
    return CT_OK;
}

void ct::net_grow_descriptors(CtHandle h, size_t count)
{
    CtHandle_::NetScratch &s = h->net;
    count = std::min(count, net_descriptor_limit(h));
    if (count <= s.desc_records()) {
        return;
    }
    DevBuf<uint8_t> bigger;
    if (bigger.alloc(count * CT_DESCRIPTOR_BYTES) != hipSuccess) {
        (void)hipGetLastError();
        return;
    }
    s.desc = std::move(bigger);
}

// The shard's tile list on the device, from ct_shard_tiles, once per handle.  The stream is idle.
static int net_ensure_tiles(CtHandle h)
{
    CtHandle_::NetScratch &s = h->net;
    if (s.tiles_built) {
        return CT_OK;
    }
    uint32_t count = 0;
    if (ct_shard_tiles(h->scene.width, h->scene.height, h->scene.shard_index, h->scene.shard_count, nullptr, 0, &count) != CT_OK) {
        return fail(h, CT_E_INVAL, "internal: ct_shard_tiles refused the handle's own frame");
    }
    std::vector<uint32_t> list(std::max(count, 1u), 0u);
    if (ct_shard_tiles(h->scene.width, h->scene.height, h->scene.shard_index, h->scene.shard_count, list.data(), count, &count) != CT_OK) {
        return fail(h, CT_E_INVAL, "internal: ct_shard_tiles refused the handle's own frame");
    }
    DevBuf<uint32_t> dev;
    HIPCHK(h, dev.alloc(list.size()));
    HIPCHK(h, hipMemcpy(dev, list.data(), list.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    s.tiles = std::move(dev);
    s.n_tiles = count;
    s.tiles_built = true;
    return CT_OK;
}

// ---- the renderer: the network evaluated band by band (ct_network_render_*) or looked up in its bake (ct_baked_render_*) -------
// A call of one of the twelve entry points.  Its bands are made of units: rows of the frame, or (tiles: the *_shard_* entry
// points) tiles of the shard's tile list.  The entry point fills the first part, net_begin the second.
struct NetCall {
    const char *who;
    CtNetwork n;       // the source of a record's output: the network ...
    CtBake b;          // ... or (baked) its bake; the other one is NULL
    const CtNetworkRender *p;
    bool baked, tiles;
    uint32_t depth;    // ct_baked_render_hybrid_*: the collisions the path is traced through before the bake is read; 0 otherwise
    bool hybrid;       // ... and that the call is one of them
    bool accumulate;   // into mean / M2 instead of the frame
    bool direct;       // the call carries CT_NET_ADD_SINGLE_SCATTER
    DescriptorScale ds;
};

// A hybrid call's depth: 1 .. 64, below the scene's max_depth (the path tracer itself stops there), and from 2 on only with the
// single-scatter term, without which the sum is no picture the library defines.
static int net_validate_depth(CtHandle h, const NetCall &c)
{
    if (c.depth == 0u || c.depth > 64u) {
        return fail(h, CT_E_INVAL, "%s: depth %u is outside 1 .. 64", c.who, c.depth);
    }
    if (c.depth >= h->scene.max_depth) {
        return fail(h, CT_E_INVAL, "%s: depth %u is not below the scene's max_depth %u", c.who, c.depth, h->scene.max_depth);
    }
    if (c.depth >= 2u && !(c.p->transform & CT_NET_ADD_SINGLE_SCATTER)) {
        return fail(h, CT_E_INVAL, "%s: depth %u needs CT_NET_ADD_SINGLE_SCATTER (only depth 1 is defined without the first collision's term)",
                    c.who, c.depth);
    }
    return CT_OK;
}

// What the entry points do before they run: the handle, every argument (first: a rejected call leaves the handle exactly as it
// was, batches in flight included), the camera, a bake's light, then the wait for the batches in flight.  bad_ids: NULL, or the
// message (a format of c.who) that refuses the call's subframe ids.
static int net_begin(CtHandle h, NetCall &c, bool accumulate, const char *bad_ids)
{
    if (!h) {
        return fail(nullptr, CT_E_INVAL, "null handle");
    }
    if (!c.p || (c.baked ? !c.b : !c.n)) {
        return fail(h, CT_E_INVAL, "%s: need a %s and its parameters", c.who, c.baked ? "bake" : "network");
    }
    NEED_NOFLUSH(h);
    int rc = net_validate_params(h, c.p, c.who);
    if (rc == CT_OK) {
        rc = c.baked ? bake_foreign(h, c.b, c.who) : net_validate_network(h, c.n, c.who);
    }
    if (rc == CT_OK) {
        rc = net_validate_shards(h, c.who, c.tiles, c.hybrid ? "ct_baked_render_hybrid" : c.baked ? "ct_baked_render" : "ct_network_render");
    }
    if (rc == CT_OK && c.hybrid) {
        rc = net_validate_depth(h, c);
    }
    if (rc != CT_OK) {
        return rc;
    }
    if (bad_ids) {
        return fail(h, CT_E_INVAL, bad_ids, c.who);
    }
    if (!h->camera_set) {
        return fail(h, CT_E_STATE, "ct_set_camera has not been called");
    }
    if (c.baked) {
        rc = bake_stale(h, c.b, c.who);
        if (rc != CT_OK) {
            return rc;
        }
    }
    c.accumulate = accumulate;
    c.direct = (c.p->transform & CT_NET_ADD_SINGLE_SCATTER) != 0;
    c.ds = descriptor_scale(h);
    return flush(h);
}

// Units of a band.  Rows: whole rows of at most band_pixels pixels, at least one (a row has at most 12288 pixels), at most 2^20
// pixels.  Tiles: at most band_pixels / 64, at least one, at most 2^14 (2^20 lanes).
static uint32_t net_band_units(CtHandle h, const NetCall &c)
{
    const uint32_t band_pixels = c.p->band_pixels;
    const uint32_t cap = (band_pixels == 0u || band_pixels > (1u << 20)) ? (1u << 20) : band_pixels;
    return c.tiles ? std::max(1u, cap / 64u) : std::min(h->scene.height, std::max(1u, cap / h->scene.width));
}

// One band of subframe `sid`, units [unit0, unit0 + units) of the call, into the frame or into mean / M2.
// Baked: the flights and one kernel that looks the table up and forms the pixels, enqueued only; hybrid: the same two steps with
// the flights followed through c.depth collisions and their directions in a third temporary.  Otherwise the flights with
// scan and compaction, the wait for the record count, gather and network in pieces of the descriptor array, and the compose
// kernel; every stage is waited for and booked into h->net.ms.
static int net_band(CtHandle h, const NetCall &c, uint32_t sid, uint32_t unit0, uint32_t units)
{
    CtHandle_::NetScratch &s = h->net;
    const uint32_t W = h->scene.width;
    const PixelBand band = c.tiles ? tile_band(h->dev, s.tiles + unit0, units) : rect_band(0u, unit0, W, units);
    const FlightTemps temps{ s.found, s.waves, c.direct ? s.direct : nullptr };
    const NetCompose compose{ c.p->transform & 0xff, c.p->rgb_scale[0], c.p->rgb_scale[1], c.p->rgb_scale[2] };
    const size_t first_pixel = c.tiles ? 0 : (size_t)unit0 * W;   // (the tile path writes at y * W + x of the whole frame)
    const ComposeTarget dst{ c.accumulate ? nullptr : h->d_frame + first_pixel, h->d_mean + first_pixel, h->d_m2 + first_pixel, sid };
    const uint32_t *const frozen = h->stop_cadence ? h->d_freeze : nullptr;
    if (c.hybrid) {
        HIPCHK(h, launch_hybrid_flights(h->dev, band, temps, s.omega, sid, c.depth, h->stream));
        HIPCHK(h, launch_hybrid_compose(h->dev, band, temps, s.omega, bake_table(c.b), compose, dst, frozen, h->stream));
        return CT_OK;
    }
    if (c.baked) {
        HIPCHK(h, launch_first_flights(h->dev, band, temps, sid, h->stream));
        HIPCHK(h, launch_baked_compose(h->dev, band, temps, bake_table(c.b), compose, dst, frozen, h->stream));
        return CT_OK;
    }
    uint32_t count = 0;
    int rc = flights_counted(h, band, temps, sid, band.n, s.pos, s.dir, nullptr, &s.ms[0], &count);
    if (rc != CT_OK) {
        return rc;
    }
    net_grow_descriptors(h, count);
    for (uint32_t at = 0; at < count;) {
        const uint32_t piece = (uint32_t)std::min<size_t>(count - at, s.desc_records());
        float ms = 0;
        HIPCHK(h, hipEventRecord(h->ev[0], h->stream));
        HIPCHK(h, launch_descriptors(h->dev, h->pyramid, s.pos + 3 * (size_t)at, s.dir + 3 * (size_t)at, piece, c.ds.level0, c.ds.voxel_m,
                                     h->scene.cloud_size_m, s.desc, h->stream));
        HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
        // l = the direction the light travels: the uniforms hold -l (Sun.cpp:13-18)
        HIPCHK(h, launch_network_aux(s.dir + 3 * (size_t)at, piece, -h->dev.nlx, -h->dev.nly, -h->dev.nlz, s.aux + at, h->stream));
        HIPCHK(h, hipEventRecord(h->ev[2], h->stream));
        char err[256] = "";
        rc = ct::network_eval(c.n, h->stream, s.desc, s.aux + at, piece, s.out + at, err, sizeof err);   // (waits)
        if (rc != CT_OK) {
            return fail(h, rc, "%s", err);
        }
        HIPCHK(h, hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
        s.ms[1] += ms;
        HIPCHK(h, hipEventElapsedTime(&ms, h->ev[1], h->ev[2]));
        s.ms[3] += ms;
        double net_ms = 0;
        ct_debug_network_time(c.n, &net_ms);
        s.ms[2] += net_ms;
        at += piece;
    }
    double compose_ms = 0;
    rc = timed(h, &compose_ms, [&]() -> int {
        HIPCHK(h, launch_network_compose(band, temps, compose, s.out, dst, frozen, h->stream));
        return CT_OK;
    });
    s.ms[3] += compose_ms;
    if (c.accumulate) {
        h->accum_ms += compose_ms;
    }
    return rc;
}

// Subframes [first, first + count) band by band.  The caller has validated and flushed.  A frame of the tile path is first
// filled with the shard's background.  A baked call only enqueues -- the convergence test keeps its own wait -- and is waited
// for once at its end: one event pair times it into h->baked_ms, and h->net.ms stays the last network call's.
static int net_run(CtHandle h, const NetCall &c, uint32_t first, uint32_t count)
{
    const uint32_t W = h->scene.width, H = h->scene.height, per_band = net_band_units(h, c);
    if (c.baked) {
        h->baked_ms = 0;
    } else {
        for (double &ms : h->net.ms) {
            ms = 0;
        }
    }
    return drained(h, [&]() -> int {
        int rc = c.tiles ? net_ensure_tiles(h) : CT_OK;
        if (rc != CT_OK) {
            return rc;
        }
        // (bands of the row path run bottom to top over H rows; those of the tile path over the list's n_tiles tiles)
        const uint32_t units = c.tiles ? h->net.n_tiles : H;
        const size_t band = c.tiles ? (size_t)64 * std::min(per_band, std::max(units, 1u)) : (size_t)W * per_band;
        rc = net_reserve(h, band, c.direct, c.hybrid);
        if (rc == CT_OK && !c.baked) {
            rc = ensure_pyramid(h);
        }
        if (rc != CT_OK) {
            return rc;
        }
        if (c.accumulate) {
            discard_ahead(h);   // like ct_accumulate: the running mean leaves the order the samples rendered ahead were made for
        }
        // the shard's background, as ct_render_subframe starts from it: the bands write the own pixels only
        const auto fill = [&]() -> int {
            HIPCHK(h, launch_fill_frame(h->d_frame, W, H, h->scene.shard_index, h->scene.shard_count, h->stream));
            return CT_OK;
        };
        if (c.baked) {
            HIPCHK(h, hipEventRecord(h->ev[0], h->stream));
        }
        for (uint32_t k = 0; k < count; k++) {
            const uint32_t sid = first + k;
            if (c.tiles && !c.accumulate) {
                rc = c.baked ? fill() : timed(h, &h->net.ms[3], fill);
                if (rc != CT_OK) {
                    return rc;
                }
            }
            for (uint32_t unit0 = 0; unit0 < units; unit0 += per_band) {
                rc = net_band(h, c, sid, unit0, std::min(per_band, units - unit0));
                if (rc != CT_OK) {
                    return rc;
                }
            }
            if (c.accumulate) {
                if (h->stop_cadence && sid % h->stop_cadence == 0u && sid >= h->stop_min) {   // as ct_accumulate
                    rc = enqueue_convergence_test(h, sid);
                    if (rc != CT_OK) {
                        return rc;
                    }
                    HIPCHK(h, hipStreamSynchronize(h->stream));
                }
                h->subframes = sid;
                discard_ahead(h);
            }
        }
        if (c.baked) {
            HIPCHK(h, hipEventRecord(h->ev[2], h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));
            float ms = 0;
            HIPCHK(h, hipEventElapsedTime(&ms, h->ev[0], h->ev[2]));
            h->baked_ms = ms;
        }
        return CT_OK;
    });
}

static int net_subframe(CtHandle h, NetCall c, uint32_t subframe_id, float *frame_rgba_dev)
{
    int rc = net_begin(h, c, false, subframe_id == 0 ? "%s: subframe ids are 1-based (Camera.cpp:191)" : nullptr);
    if (rc != CT_OK) {
        return rc;
    }
    rc = net_run(h, c, subframe_id, 1);
    if (rc != CT_OK) {
        return rc;
    }
    if (frame_rgba_dev) {
        HIPCHK(h, hipMemcpyAsync(frame_rgba_dev, h->d_frame, (size_t)h->scene.width * h->scene.height * sizeof(float4),
                                 hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return CT_OK;
}

static int net_accumulate(CtHandle h, NetCall c, uint32_t first_subframe_id, uint32_t count)
{
    const int rc = net_begin(h, c, true,
                             first_subframe_id == 0 || count == 0 ? "%s: subframe ids are 1-based and count must not be 0" : nullptr);
    if (rc != CT_OK) {
        return rc;
    }
    if (first_subframe_id != h->subframes + 1) {
        return fail(h, CT_E_STATE, "first_subframe_id %u but %u subframes are accumulated", first_subframe_id, h->subframes);
    }
    if (count > 0xffffffffu - first_subframe_id + 1u) {
        return fail(h, CT_E_INVAL, "%s: %u subframes from %u on exceed the 32-bit subframe id", c.who, count, first_subframe_id);
    }
    return net_run(h, c, first_subframe_id, count);
}

extern "C" int ct_network_render_subframe(CtHandle h, CtNetwork n, const CtNetworkRender *p, uint32_t subframe_id, float *frame_rgba_dev)
{
    return net_subframe(h, { "ct_network_render_subframe", n, nullptr, p, false, false }, subframe_id, frame_rgba_dev);
}

extern "C" int ct_network_render_shard_subframe(CtHandle h, CtNetwork n, const CtNetworkRender *p, uint32_t subframe_id,
                                                float *frame_rgba_dev)
{
    return net_subframe(h, { "ct_network_render_shard_subframe", n, nullptr, p, false, true }, subframe_id, frame_rgba_dev);
}

extern "C" int ct_network_render_accumulate(CtHandle h, CtNetwork n, const CtNetworkRender *p, uint32_t first_subframe_id, uint32_t count)
{
    return net_accumulate(h, { "ct_network_render_accumulate", n, nullptr, p, false, false }, first_subframe_id, count);
}

extern "C" int ct_network_render_shard_accumulate(CtHandle h, CtNetwork n, const CtNetworkRender *p, uint32_t first_subframe_id,
                                                  uint32_t count)
{
    return net_accumulate(h, { "ct_network_render_shard_accumulate", n, nullptr, p, false, true }, first_subframe_id, count);
}

extern "C" int ct_baked_render_subframe(CtHandle h, CtBake b, const CtNetworkRender *p, uint32_t subframe_id, float *frame_rgba_dev)
{
    return net_subframe(h, { "ct_baked_render_subframe", nullptr, b, p, true, false }, subframe_id, frame_rgba_dev);
}

extern "C" int ct_baked_render_shard_subframe(CtHandle h, CtBake b, const CtNetworkRender *p, uint32_t subframe_id, float *frame_rgba_dev)
{
    return net_subframe(h, { "ct_baked_render_shard_subframe", nullptr, b, p, true, true }, subframe_id, frame_rgba_dev);
}

extern "C" int ct_baked_render_accumulate(CtHandle h, CtBake b, const CtNetworkRender *p, uint32_t first_subframe_id, uint32_t count)
{
    return net_accumulate(h, { "ct_baked_render_accumulate", nullptr, b, p, true, false }, first_subframe_id, count);
}

extern "C" int ct_baked_render_shard_accumulate(CtHandle h, CtBake b, const CtNetworkRender *p, uint32_t first_subframe_id, uint32_t count)
{
    return net_accumulate(h, { "ct_baked_render_shard_accumulate", nullptr, b, p, true, true }, first_subframe_id, count);
}


extern "C" int ct_baked_render_hybrid_subframe(CtHandle h, CtBake b, const CtNetworkRender *p, uint32_t depth, uint32_t subframe_id,
                                               float *frame_rgba_dev)
{
    return net_subframe(h, { "ct_baked_render_hybrid_subframe", nullptr, b, p, true, false, depth, true }, subframe_id, frame_rgba_dev);
}

extern "C" int ct_baked_render_hybrid_shard_subframe(CtHandle h, CtBake b, const CtNetworkRender *p, uint32_t depth, uint32_t subframe_id,
                                                     float *frame_rgba_dev)
{
    return net_subframe(h, { "ct_baked_render_hybrid_shard_subframe", nullptr, b, p, true, true, depth, true }, subframe_id, frame_rgba_dev);
}

extern "C" int ct_baked_render_hybrid_accumulate(CtHandle h, CtBake b, const CtNetworkRender *p, uint32_t depth, uint32_t first_subframe_id,
                                                 uint32_t count)
{
    return net_accumulate(h, { "ct_baked_render_hybrid_accumulate", nullptr, b, p, true, false, depth, true }, first_subframe_id, count);
}

extern "C" int ct_baked_render_hybrid_shard_accumulate(CtHandle h, CtBake b, const CtNetworkRender *p, uint32_t depth,
                                                       uint32_t first_subframe_id, uint32_t count)
{
    return net_accumulate(h, { "ct_baked_render_hybrid_shard_accumulate", nullptr, b, p, true, true, depth, true }, first_subframe_id, count);
}

extern "C" int ct_debug_baked_render_time(CtHandle h, double *gpu_ms_out)
{
    NEED_NOFLUSH(h);
    if (!gpu_ms_out) {
        return fail(h, CT_E_INVAL, "ct_debug_baked_render_time: gpu_ms_out is NULL");
    }
    *gpu_ms_out = h->baked_ms;
    return CT_OK;
}

extern "C" int ct_debug_network_aux(CtHandle h, const float *directions_dev, uint32_t count, float *aux_dev_out)
{
    NEED(h);
    if (count == 0) {
        return CT_OK;
    }
    if (!directions_dev || !aux_dev_out) {
        return fail(h, CT_E_INVAL, "ct_debug_network_aux: need directions and an output array");
    }
    HIPCHK(h, launch_network_aux(directions_dev, count, -h->dev.nlx, -h->dev.nly, -h->dev.nlz, aux_dev_out, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return CT_OK;
}

extern "C" int ct_debug_network_render_time(CtHandle h, double ms_out[4])
{
    NEED_NOFLUSH(h);
    if (!ms_out) {
        return fail(h, CT_E_INVAL, "ct_debug_network_render_time: ms_out is NULL");
    }
    for (int i = 0; i < 4; i++) {
        ms_out[i] = h->net.ms[i];
    }
    return CT_OK;
}

extern "C" int ct_debug_network_scratch(CtHandle h, uint64_t out[12])
{
    NEED_NOFLUSH(h);
    if (!out) {
        return fail(h, CT_E_INVAL, "ct_debug_network_scratch: out is NULL");
    }
    const CtHandle_::NetScratch &s = h->net;
    const void *ptrs[9] = { s.found, s.waves, s.pos, s.dir, s.aux, s.out, s.desc, s.direct, s.tiles };
    for (int i = 0; i < 9; i++) {
        out[i] = (uint64_t)(uintptr_t)ptrs[i];
    }
    out[9] = s.band_cap;
    out[10] = s.desc_records();
    out[11] = s.direct.capacity();
    return CT_OK;
}
