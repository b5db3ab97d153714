// ct_bake.cpp -- the bakes of the C ABI, on the handle of ct_handle.hpp: the scattering network baked into a probe table
// (ct_network_bake, _sparse, _compact; ct_bake_update), which ct_neural.cpp's renderer looks up (ct_baked_render_*).  The traced
// bake (ct_bake_traced) fills the same table with the path tracer's point estimator instead: its two kernels are
// ct_bake_trace.hip, its launches ct_api.cpp's point_launch.  The adaptive traced bake (ct_bake_traced_adaptive) traces in
// rounds, keeps m2 and count per entry and stops entries by the reference's rule: its fold, scan and compaction kernels are in
// ct_bake_trace.hip too.  Half tables (ct_bake_half) and bake files (ct_bake_save, ct_bake_load) are at the end; the file's
// parser is the device-free ct_bakefile.hpp, their two kernels ct_bake_file.hip.  What crosses to ct_neural.cpp: ct_bake.hpp.
// A bake on a group (ct_group_bake_*, ct_group.hip) is a CtBake_ per shard that builds a span of the node list; the span, the
// checks a group call passes through and the exchange between the shards are here, behind ct_bake_group.hpp.
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>

#include <unistd.h>

#include "ct_bake.hpp"
#include "ct_bake_group.hpp"
#include "ct_bakefile.hpp"
#include "ct_network.hpp"

// ---- the network baked into a probe table (ct_network_bake, ct_baked_render_*) -----------------------------------------
// What a bake of the table writes besides the table: ct_bake_update and ct_bake_retrace fill a second table, and a failure puts
// this part back as it was.
struct BakeState {
    float l[3] = {}, a[3] = {}, b[3] = {};   // the light the table holds and the azimuth frame
    uint64_t epoch = 0;                      // the handle's light epoch at the bake
    uint32_t light_bits[4] = {};             // ... and the bits of its light colour and intensity then (the bake file's header)
    double gather_ms = 0, network_ms = 0, mask_ms = 0;
    uint32_t samples = 0;                    // a traced bake: experiments folded into every stored entry of an active node
    uint64_t paths = 0;
    double trace_ms = 0, fold_ms = 0;
    // an adaptive traced bake: `samples` is the count its last round reached
    uint32_t cap = 0, rounds = 0;            // max_samples as it is now; rounds traced
    uint64_t live = 0;                       // entries in d_live[live_cur]: those at the cap that fail the rule
    int live_cur = 0;
    double test_ms = 0;
};

// What a bake is besides that state and its buffers: whose it is, its grid and its kind.  Fixed once the bake is made (margin
// and active: once its mask is counted, bake_adopt_mask); ct_bake_half copies it whole.
struct BakeShape {
    CtHandle h = nullptr;
    int device = 0;
    uint32_t grid[3] = { 0, 0, 0 }, azimuths = 0, cosines = 0;
    uint64_t entries = 0;
    uint64_t stored = 0;                     // the floats the table holds: entries, or what a compact bake's mask leaves
    float cosine[64] = {};
    bool sparse = false;                     // ct_network_bake_sparse: only the probes of the active position nodes
    bool compact = false;                    // ct_network_bake_compact: ... and only their blocks are stored
    bool traced = false;                     // ct_bake_traced: means of the path tracer's point estimator, no network
    uint32_t margin = 0;                     // M
    uint64_t active = 0;                     // active nodes
};

struct CtBake_ : BakeState, BakeShape {
    DevBuf<float> d_table;
    // A sparse bake: the density of a live handle never changes, so the mask and the list are made once and ct_bake_update reuses them.
    DevBuf<uint8_t> d_nodes;                 // one byte per node
    DevBuf<uint32_t> d_list;                 // the active nodes, ascending
    DevBuf<float> d_probe;                   // the position nodes of x, y, z and the Nphi probe directions (bake_probe's floats)
    // A compact bake: a sparse bake whose table holds a zero block and then the blocks of the active nodes in the list's order;
    // d_slots finds a node's block.
    DevBuf<uint32_t> d_slots;                // one word per node: 1 + its place in the list, 0 for an inactive node
    // A traced bake of any kind has d_probe (its position nodes) and d_dirs, the Nphi x Nc x 3 direction table of its frame.
    DevBuf<float> d_dirs;
    // ct_bake_traced_adaptive: m2 and count beside every stored mean, the two live lists the rounds alternate
    // between (stored indices, counted through the blocks of the active nodes as the task kernel counts them) and the wave counts.
    bool adaptive = false;
    CtBakeAdaptive ap{};                     // (max_samples: as given; BakeState::cap is the one in force)
    DevBuf<float> d_m2;
    DevBuf<uint32_t> d_counts, d_live[2], d_waves;
    // ct_bake_half: the stored table as binary16 in d_half, no d_table.  Final: nothing bakes or traces into it.
    bool half = false;
    DevBuf<uint16_t> d_half;
    // A bake on a group (ct_group_bake_*): shard `shard` of `shards` builds and continues only the positions
    // [span_lo, span_hi) of the node list -- all nodes for a dense bake -- which are the floats [range_lo, range_hi) of the stored
    // arrays; the group's exchange brings the rest.  shards == 1: everything, and none of the four is read.
    uint32_t shard = 0, shards = 1;
    uint64_t span_lo = 0, span_hi = 0, range_lo = 0, range_hi = 0;
};

static uint64_t bake_nodes(const BakeShape &s)
{
    return (uint64_t)s.grid[0] * s.grid[1] * s.grid[2];
}

// The floats of d_probe -- the position nodes of x, y and z, then the Nphi probe directions -- and of d_dirs.
static size_t bake_axis_floats(const BakeShape &s)
{
    return (size_t)s.grid[0] + s.grid[1] + s.grid[2];
}
static size_t bake_probe_floats(const BakeShape &s)
{
    return bake_axis_floats(s) + 3 * (size_t)s.azimuths;
}
static size_t bake_dir_floats(const BakeShape &s)
{
    return 3 * (size_t)s.azimuths * s.cosines;
}

// The shape of a bake of `kind` (CT_BAKE_DENSE, _SPARSE or _COMPACT) on h, its description validated: the entries and the polar
// nodes cosine[k] = -1 + 2 k / (Nc - 1).  margin and active wait for the mask.
static BakeShape bake_shape(CtHandle h, const uint32_t grid[3], uint32_t azimuths, uint32_t cosines, uint32_t kind, bool traced)
{
    BakeShape s;
    s.h = h;
    s.device = h->device;
    std::copy_n(grid, 3, s.grid);
    s.azimuths = azimuths;
    s.cosines = cosines;
    s.entries = s.stored = bake_nodes(s) * azimuths * cosines;
    for (uint32_t k = 0; k < cosines; k++) {
        s.cosine[k] = (float)(-1.0 + 2.0 * (double)k / (double)(cosines - 1u));
    }
    s.sparse = kind != CT_BAKE_DENSE;
    s.compact = kind == CT_BAKE_COMPACT;
    s.traced = traced;
    return s;
}

static uint64_t bake_probes_total(const CtBake_ *b)
{
    return b->entries / b->cosines;
}

// The nodes a build covers: every node of a dense bake, the active ones in the list's order otherwise.  A bake on a group covers
// its span of them.
static uint64_t bake_cover(const CtBake_ *b)
{
    return b->sparse ? b->active : bake_nodes(*b);
}
static void bake_span(const CtBake_ *b, uint64_t *lo, uint64_t *hi)
{
    *lo = b->shards == 1u ? 0u : b->span_lo;
    *hi = b->shards == 1u ? bake_cover(b) : b->span_hi;
}

// Cuts b, whose mask is counted, for shard `shard` of `shards`: positions [shard A / shards, (shard + 1) A / shards) of the A nodes
// it covers (A <= 2^24, shards <= 64), and the floats of the stored arrays they are.  A sparse bake reads the two ends of its
// span from the list.
static int bake_cut(CtHandle h, CtBake_ *b, uint32_t shard, uint32_t shards)
{
    const uint64_t A = bake_cover(b), block = (uint64_t)b->azimuths * b->cosines;
    b->shard = shard;
    b->shards = shards;
    b->span_lo = (uint64_t)shard * A / shards;
    b->span_hi = ((uint64_t)shard + 1u) * A / shards;
    if (b->compact) {
        b->range_lo = block + b->span_lo * block;
        b->range_hi = block + b->span_hi * block;
    } else if (b->sparse && b->span_lo < b->span_hi && shards != 1u) {
        uint32_t first = 0, last = 0;
        HIPCHK(h, hipMemcpy(&first, b->d_list + b->span_lo, sizeof first, hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(&last, b->d_list + (b->span_hi - 1u), sizeof last, hipMemcpyDeviceToHost));
        b->range_lo = (uint64_t)first * block;
        b->range_hi = ((uint64_t)last + 1u) * block;
    } else if (b->sparse) {
        b->range_lo = b->range_hi = 0;
    } else {
        b->range_lo = b->span_lo * block;
        b->range_hi = b->span_hi * block;
    }
    return CT_OK;
}

// The record of probe `index` = ((z Ny + y) Nx + x) Nphi + j: its position node and u_j, made in double and rounded once.
static void bake_probe(const CtBake_ *b, uint64_t index, float pos[3], float dir[3])
{
    const uint32_t j = (uint32_t)(index % b->azimuths);
    uint64_t cell = index / b->azimuths;
    const float box[3] = { b->h->dev.bx, b->h->dev.by, b->h->dev.bz };
    for (int axis = 0; axis < 3; axis++) {
        const uint32_t i = (uint32_t)(cell % b->grid[axis]);
        cell /= b->grid[axis];
        pos[axis] = (float)(-0.5 * (double)box[axis] + (double)box[axis] * (double)i / (double)(b->grid[axis] - 1u));
    }
    const double t = (double)j / (double)(b->azimuths / 4u);
    const double p = t <= 2.0 ? 1.0 - t : t - 3.0, q = t <= 2.0 ? 1.0 - std::fabs(p) : -(1.0 - std::fabs(p));
    double u[3], len = 0;
    for (int axis = 0; axis < 3; axis++) {
        u[axis] = p * (double)b->a[axis] + q * (double)b->b[axis];
        len += u[axis] * u[axis];
    }
    len = std::sqrt(len);
    for (int axis = 0; axis < 3; axis++) {
        dir[axis] = (float)(u[axis] / len);
    }
}

// The light of the handle as it is now, and a frame (a, b) perpendicular to it: a = normalize(l x e) for the coordinate axis e
// on which l is shortest, b = l x a.
static void bake_frame(CtHandle h, BakeState *b)
{
    const double l[3] = { -(double)h->dev.nlx, -(double)h->dev.nly, -(double)h->dev.nlz };
    int e = 0;
    for (int axis = 1; axis < 3; axis++) {
        if (std::fabs(l[axis]) < std::fabs(l[e])) {
            e = axis;
        }
    }
    double ev[3] = { 0, 0, 0 };
    ev[e] = 1;
    double ll = std::sqrt(l[0] * l[0] + l[1] * l[1] + l[2] * l[2]);
    const double n[3] = { l[0] / ll, l[1] / ll, l[2] / ll };
    double a[3] = { n[1] * ev[2] - n[2] * ev[1], n[2] * ev[0] - n[0] * ev[2], n[0] * ev[1] - n[1] * ev[0] };
    const double al = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    for (double &v : a) {
        v /= al;
    }
    const double bb[3] = { n[1] * a[2] - n[2] * a[1], n[2] * a[0] - n[0] * a[2], n[0] * a[1] - n[1] * a[0] };
    for (int axis = 0; axis < 3; axis++) {
        b->l[axis] = (float)l[axis];
        b->a[axis] = (float)a[axis];
        b->b[axis] = (float)bb[axis];
    }
    b->epoch = h->light_epoch;
    for (int c = 0; c < 3; c++) {
        b->light_bits[c] = float_bits(h->scene.light_color[c]);
    }
    b->light_bits[3] = float_bits(h->scene.light_intensity);
}

BakeTable ct::bake_table(const CtBake_ *b)
{
    return { b->d_table, b->grid[0], b->grid[1], b->grid[2], b->azimuths, b->cosines, b->l[0], b->l[1], b->l[2],
             b->a[0], b->a[1], b->a[2], b->b[0], b->b[1], b->b[2], b->d_slots, b->d_half };
}

// The mask of a probe grid on h (include/cloudtrace.h, "the sparse bake"): its device memory, allocated by bake_mask_reserve
// before anything runs, and filled by bake_mask_run.
struct BakeMask {
    std::vector<uint32_t> host_ranges;   // lo | hi << 16 per cell of x, then y, then z
    uint32_t margin = 0, slab = 0;
    DevBuf<uint32_t> ranges, waves, list, slots;   // slots: only with bake_mask_reserve's `slots`
    DevBuf<uint8_t> tmp_x, tmp_xy, cells, nodes;
};

// The words a scan over n lanes needs (the mask's nodes, an adaptive bake's live entries): a count per wave of 64, in whole
// blocks of 256 lanes, and one for the total.
static size_t bake_wave_counts(uint64_t n)
{
    return (size_t)((n + 255u) / 256u * 4u + 1u);
}

static int bake_mask_reserve(CtHandle h, const uint32_t grid[3], BakeMask &m, bool slots = false)
{
    const uint32_t *dims = h->scene.dims;
    const uint32_t maxdim = std::max(dims[0], std::max(dims[1], dims[2]));
    const double S = (double)h->scene.sample_step * (double)maxdim;
    m.margin = (uint32_t)std::ceil(S) + 3u;
    m.host_ranges.clear();
    for (int axis = 0; axis < 3; axis++) {
        const double D = (double)dims[axis], last = (double)(grid[axis] - 1u), M = (double)m.margin;
        for (uint32_t c = 0; c + 1u < grid[axis]; c++) {
            const double lo = std::max(0.0, std::floor((double)c * D / last) - M);
            const double hi = std::min(D - 1.0, std::ceil((double)(c + 1u) * D / last) + M);
            m.host_ranges.push_back((uint32_t)lo | (uint32_t)hi << 16);   // (dims <= 2048)
        }
    }
    const size_t cx = grid[0] - 1u, cy = grid[1] - 1u, cz = grid[2] - 1u, nodes = (size_t)grid[0] * grid[1] * grid[2];
    // (CT_BAKE_MASK_BYTES: the most the first temporary may take; a volume whose planes need more goes through in slabs of z)
    const size_t cap = (size_t)knob_int(h->tune.BAKE_MASK_BYTES, 1, 1 << 30, 64 << 20), plane = (size_t)dims[1] * cx;
    m.slab = (uint32_t)std::min<size_t>(dims[2], std::max<size_t>(1, cap / plane));
    HIPCHK(h, m.ranges.alloc(m.host_ranges.size()));
    HIPCHK(h, m.tmp_x.alloc(m.slab * plane));
    HIPCHK(h, m.tmp_xy.alloc(m.slab * cy * cx));
    HIPCHK(h, m.cells.alloc(cz * cy * cx));
    HIPCHK(h, m.nodes.alloc(nodes));
    HIPCHK(h, m.waves.alloc(bake_wave_counts(nodes)));
    HIPCHK(h, m.list.alloc(nodes));
    if (slots) {
        HIPCHK(h, m.slots.alloc(nodes));
    }
    return CT_OK;
}

// The stream is idle.  *active_out = the number of active nodes (the one 4-byte read), *ms_out = the kernels' GPU time.
static int bake_mask_run(CtHandle h, const uint32_t grid[3], BakeMask &m, uint32_t *active_out, double *ms_out)
{
    const uint64_t nodes = (uint64_t)grid[0] * grid[1] * grid[2];
    return drained(h, [&]() -> int {
        HIPCHK(h, hipMemcpyAsync(m.ranges, m.host_ranges.data(), m.host_ranges.size() * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
        BakeMaskArgs a{};
        a.density = h->d_density;
        for (int axis = 0; axis < 3; axis++) {
            a.dims[axis] = h->scene.dims[axis];
            a.grid[axis] = grid[axis];
        }
        a.slab = m.slab;
        a.ranges = m.ranges;
        a.tmp_x = m.tmp_x;
        a.tmp_xy = m.tmp_xy;
        a.cells = m.cells;
        a.nodes = m.nodes;
        a.waves = m.waves;
        a.list = m.list;
        a.slots = m.slots;
        uint32_t count = 0;
        double ms = 0;
        const int rc = timed(h, &ms, [&]() -> int {
            HIPCHK(h, launch_bake_mask(a, h->stream));
            return CT_OK;
        }, m.waves + (bake_wave_counts(nodes) - 1u), &count);
        if (rc != CT_OK) {
            return rc;
        }
        if (count > nodes) {
            return fail(h, CT_E_HIP, "internal: a grid of %llu nodes counted %u active ones", (unsigned long long)nodes, count);
        }
        *active_out = count;
        *ms_out = ms;
        return CT_OK;
    });
}

// b takes over a mask that has run: its margin and count, the node bytes, the list and the slots (empty unless compact).
static void bake_adopt_mask(CtBake_ *b, BakeMask &m, uint32_t active)
{
    b->margin = m.margin;
    b->active = active;
    b->d_nodes = std::move(m.nodes);
    b->d_list = std::move(m.list);
    b->d_slots = std::move(m.slots);
}

// The tables of the sparse bake's record kernel in b->d_probe, by bake_probe (ct_bake_probes' floats): the position nodes of x,
// y and z, then the Nphi probe directions.
static int bake_upload_probe_tables(CtHandle h, const CtBake_ *b)
{
    const uint32_t nx = b->grid[0], ny = b->grid[1], nz = b->grid[2];
    std::vector<float> host(bake_probe_floats(*b));
    float p[3], d[3];
    for (uint32_t i = 0; i < nx; i++) {
        bake_probe(b, (uint64_t)i * b->azimuths, p, d);
        host[i] = p[0];
    }
    for (uint32_t i = 0; i < ny; i++) {
        bake_probe(b, (uint64_t)i * nx * b->azimuths, p, d);
        host[nx + i] = p[1];
    }
    for (uint32_t i = 0; i < nz; i++) {
        bake_probe(b, (uint64_t)i * nx * ny * b->azimuths, p, d);
        host[nx + ny + i] = p[2];
    }
    for (uint32_t j = 0; j < b->azimuths; j++) {
        bake_probe(b, j, p, &host[nx + ny + nz + 3 * (size_t)j]);
    }
    HIPCHK(h, hipMemcpy(b->d_probe, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
    return CT_OK;
}

// The records of probes [first, first + count) in the handle's scratch.  Dense: made on the host (pos / dir, which the stream
// has left) and copied.  Sparse: the compacted probes -- azimuth p % Nphi of node list[p / Nphi] -- from the record kernel,
// timed into *records_ms.
static int bake_chunk_records(CtHandle h, const CtBake_ *b, uint64_t first, uint32_t count, std::vector<float> &pos, std::vector<float> &dir,
                              double *records_ms)
{
    CtHandle_::NetScratch &s = h->net;
    if (b->sparse) {
        return timed(h, records_ms, [&]() -> int {
            HIPCHK(h, launch_bake_records(b->d_list, first, count, b->grid[0], b->grid[1], b->azimuths, b->d_probe,
                                          b->d_probe + bake_axis_floats(*b), s.pos, s.dir, h->stream));
            return CT_OK;
        });
    }
    for (uint32_t i = 0; i < count; i++) {
        bake_probe(b, first + i, &pos[3 * (size_t)i], &dir[3 * (size_t)i]);
    }
    HIPCHK(h, hipMemcpyAsync(s.pos, pos.data(), 3 * (size_t)count * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(s.dir, dir.data(), 3 * (size_t)count * sizeof(float), hipMemcpyHostToDevice, h->stream));
    return CT_OK;
}

// The network's outputs for polar node k of probes [first, first + piece) into the table: in place, or through the list.
// Compact: the table is contiguous in compacted-probe order behind its zero block, so in place again.
static int bake_store_piece(CtHandle h, const CtBake_ *b, float *table, uint64_t first, uint32_t piece, uint32_t k)
{
    if (b->compact) {
        HIPCHK(h, launch_bake_store(h->net.out, piece, table + (b->azimuths + first) * b->cosines, b->cosines, k, h->stream));
    } else if (b->sparse) {
        HIPCHK(h, launch_bake_store_list(h->net.out, b->d_list, first, piece, b->azimuths, table, b->cosines, k, h->stream));
    } else {
        HIPCHK(h, launch_bake_store(h->net.out, piece, table + first * b->cosines, b->cosines, k, h->stream));
    }
    return CT_OK;
}

// Fills `table` (b->stored floats, allocated) for the handle's light and network n: the probes of b's span in chunks through the handle's
// scratch, one gather per piece and one evaluation per polar node.  b's frame is the new light's already.
// A sparse bake zeroes the table first and runs only the probes of its list; a compact one zeroes only the zero block.
static int bake_run(CtHandle h, CtNetwork n, CtBake_ *b, float *table)
{
    CtHandle_::NetScratch &s = h->net;
    uint64_t lo, hi;
    bake_span(b, &lo, &hi);
    const uint64_t probes_lo = lo * b->azimuths, probes_hi = hi * b->azimuths, probes = probes_hi - probes_lo;
    const size_t chunk = (size_t)std::min<uint64_t>(probes, std::min<size_t>(net_descriptor_limit(h), (size_t)1 << 20));
    const DescriptorScale ds = descriptor_scale(h);
    std::vector<float> pos(b->sparse ? 0 : 3 * chunk), dir(b->sparse ? 0 : 3 * chunk);
    double gather_ms = 0, network_ms = 0, records_ms = 0;
    const int rc = drained(h, [&]() -> int {
        if (b->sparse) {
            const uint64_t zeroed = b->compact ? (uint64_t)b->azimuths * b->cosines : b->entries;
            HIPCHK(h, hipMemsetAsync(table, 0, (size_t)zeroed * sizeof(float), h->stream));
        }
        if (probes == 0u) {   // (a bake without active nodes, or a shard's empty span)
            HIPCHK(h, hipStreamSynchronize(h->stream));
            return CT_OK;
        }
        int rc = net_reserve(h, chunk, false);
        if (rc == CT_OK) {
            rc = ensure_pyramid(h);
        }
        if (rc != CT_OK) {
            return rc;
        }
        net_grow_descriptors(h, chunk);
        if (b->sparse) {
            rc = bake_upload_probe_tables(h, b);
            if (rc != CT_OK) {
                return rc;
            }
        }
        for (uint64_t first = probes_lo; first < probes_hi; first += chunk) {
            const uint32_t count = (uint32_t)std::min<uint64_t>(chunk, probes_hi - first);
            rc = bake_chunk_records(h, b, first, count, pos, dir, &records_ms);
            if (rc != CT_OK) {
                return rc;
            }
            for (uint32_t at = 0; at < count;) {
                const uint32_t piece = (uint32_t)std::min<size_t>(count - at, s.desc_records());
                float ms = 0;
                HIPCHK(h, hipEventRecord(h->ev[0], h->stream));
                HIPCHK(h, launch_descriptors(h->dev, h->pyramid, s.pos + 3 * (size_t)at, s.dir + 3 * (size_t)at, piece, ds.level0, ds.voxel_m,
                                             h->scene.cloud_size_m, s.desc, h->stream));
                HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
                for (uint32_t k = 0; k < b->cosines; k++) {
                    HIPCHK(h, launch_bake_fill(s.aux, piece, b->cosine[k], h->stream));
                    char err[256] = "";
                    rc = ct::network_eval(n, h->stream, s.desc, s.aux, piece, s.out, err, sizeof err);   // (waits)
                    if (rc != CT_OK) {
                        return fail(h, rc, "%s", err);
                    }
                    double net_ms = 0;
                    ct_debug_network_time(n, &net_ms);
                    network_ms += net_ms;
                    rc = bake_store_piece(h, b, table, first + at, piece, k);
                    if (rc != CT_OK) {
                        return rc;
                    }
                }
                HIPCHK(h, hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
                gather_ms += ms;
                at += piece;
            }
            HIPCHK(h, hipStreamSynchronize(h->stream));   // (before the host arrays are filled again)
        }
        return CT_OK;
    });
    if (rc != CT_OK) {
        return rc;
    }
    b->gather_ms = gather_ms;
    b->network_ms = network_ms;
    b->mask_ms = records_ms;
    return CT_OK;
}

// ---- the traced bake (ct_bake_traced): the table filled by the path tracer's point estimator ---------------------------------------
// d(j, k) = c l + sqrt(1 - c^2) u_j, c = cosine[k], in double from the frame's floats and rounded once: [j][k][xyz].
static void bake_directions(const CtBake_ *b, std::vector<float> &out)
{
    out.resize(bake_dir_floats(*b));
    float p[3], u[3];
    for (uint32_t j = 0; j < b->azimuths; j++) {
        bake_probe(b, j, p, u);
        for (uint32_t k = 0; k < b->cosines; k++) {
            const double c = (double)b->cosine[k], s = std::sqrt(1.0 - c * c);
            for (int axis = 0; axis < 3; axis++) {
                out[3 * ((size_t)j * b->cosines + k) + axis] = (float)(c * (double)b->l[axis] + s * (double)u[axis]);
            }
        }
    }
}

// The tables the task kernel reads, for b's frame as it is: the position nodes and u_j in d_probe, d(j, k) in d_dirs.
static int bake_upload_trace_tables(CtHandle h, const CtBake_ *b)
{
    std::vector<float> dirs;
    bake_directions(b, dirs);
    HIPCHK(h, hipMemcpy(b->d_dirs, dirs.data(), dirs.size() * sizeof(float), hipMemcpyHostToDevice));
    return bake_upload_probe_tables(h, b);
}

// The stored entries of active nodes: what a trace covers.
static uint64_t bake_trace_total(const CtBake_ *b)
{
    const uint64_t block = (uint64_t)b->azimuths * b->cosines;
    return b->sparse ? b->active * block : b->entries;
}

// What the trace kernels are told of b whatever the chunk: first, n, n_pad and live are the caller's.
static BakeTraceArgs bake_trace_args(const CtBake_ *b)
{
    BakeTraceArgs a{};
    a.list = b->sparse ? b->d_list.get() : nullptr;
    a.axes = b->d_probe;
    a.directions = b->d_dirs;
    a.nx = b->grid[0];
    a.ny = b->grid[1];
    a.nphi = b->azimuths;
    a.nc = b->cosines;
    a.compact = b->compact ? 1u : 0u;
    return a;
}

// Results one pass of the traced bake may keep in the point buffers' `frames`: 2^24 (256 MiB), or CT_BAKE_TRACE_RESULTS.
static uint32_t bake_trace_budget(CtHandle h)
{
    return (uint32_t)knob_int(h->tune.BAKE_TRACE_RESULTS, 64, 1 << 26, 1 << 24);
}

// Experiments b->samples + 1 .. b->samples + samples of every stored entry of an active node, folded into `table` (b->stored
// floats, which hold the means of b->samples experiments).  The stream is idle and the tables of b's frame are uploaded.  The
// entries go through in chunks of at most 2^20, a chunk's samples in passes that keep at most the budget of results; the
// estimator runs on a copy of the handle's scene in CT_MODE_SUN_MULTIPLE_SCATTER.  Books b's counts and times.
static int bake_trace(CtHandle h, CtBake_ *b, float *table, uint32_t samples)
{
    const uint64_t block = (uint64_t)b->azimuths * b->cosines;
    uint64_t lo, hi;
    bake_span(b, &lo, &hi);
    const uint64_t begin = lo * block, end = hi * block, total = end - begin;   // (a bake on a group: its span's entries)
    b->trace_ms = b->fold_ms = 0;
    if (samples == 0u || total == 0u) {
        b->samples += samples;
        return CT_OK;
    }
    const uint32_t budget = bake_trace_budget(h);
    const uint32_t chunk = (uint32_t)std::min<uint64_t>(total, std::min<uint32_t>(budget, 1u << 20));
    DevScene sc = h->dev;
    sc.mode = CT_MODE_SUN_MULTIPLE_SCATTER;
    Event ev[4];
    for (Event &e : ev) {
        HIPCHK(h, e.create());
    }
    CtHandle_::PointBuffers &pt = h->pt;
    const double render_before = h->render_ms;
    double fold_ms = 0;
    for (uint64_t first = begin; first < end; first += chunk) {
        BakeTraceArgs a = bake_trace_args(b);
        a.first = first;
        a.n = (uint32_t)std::min<uint64_t>(chunk, end - first);
        a.n_pad = (a.n + 63u) & ~63u;
        const uint32_t per_pass = std::min(0xffffu, std::max(1u, budget / a.n_pad));
        for (uint32_t at = 0; at < samples; at += per_pass) {
            const uint32_t passes = std::min(per_pass, samples - at), done = b->samples + at;
            const int rc = point_launch(
                h, sc, a.n, done + 1u, passes,
                [&]() -> int {
                    HIPCHK(h, hipEventRecord(ev[0], h->stream));
                    HIPCHK(h, launch_bake_trace_tasks(sc, a, pt.primary, pt.pixels, h->stream));
                    HIPCHK(h, hipEventRecord(ev[1], h->stream));
                    return CT_OK;
                },
                [&]() -> int {
                    HIPCHK(h, hipEventRecord(ev[2], h->stream));
                    HIPCHK(h, launch_bake_trace_fold(a, pt.frames, a.n_pad, passes, done, table, h->stream));
                    HIPCHK(h, hipEventRecord(ev[3], h->stream));
                    return CT_OK;
                });
            if (rc != CT_OK) {
                return rc;
            }
            float ms0 = 0, ms1 = 0;
            HIPCHK(h, hipEventElapsedTime(&ms0, ev[0], ev[1]));
            HIPCHK(h, hipEventElapsedTime(&ms1, ev[2], ev[3]));
            fold_ms += (double)ms0 + (double)ms1;
        }
    }
    b->samples += samples;
    b->paths += total * samples;
    b->trace_ms = h->render_ms - render_before;
    b->fold_ms = fold_ms;
    return CT_OK;
}

// A trace from nothing into `table` (b->stored floats): zeroed, the tables of b's frame as it is uploaded, `samples` experiments.
static int bake_trace_fresh(CtHandle h, CtBake_ *b, float *table, uint32_t samples)
{
    return drained(h, [&]() -> int {
        HIPCHK(h, hipMemsetAsync(table, 0, (size_t)b->stored * sizeof(float), h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        const int up = bake_upload_trace_tables(h, b);
        return up != CT_OK ? up : bake_trace(h, b, table, samples);
    });
}

// ---- the adaptive traced bake (ct_bake_traced_adaptive): rounds of experiments for the entries that have not converged ----------
// What an adaptive trace writes: the bake's own arrays, or ct_bake_retrace_adaptive's second set.
struct BakeAdaptiveSet {
    DevBuf<float> table, m2;
    DevBuf<uint32_t> counts, live[2], waves;
};
struct BakeAdaptiveTarget {
    float *table, *m2;
    uint32_t *counts, *live[2], *waves;
};
static BakeAdaptiveTarget bake_adaptive_target(float *table, const BakeAdaptiveSet &s)
{
    return { table, s.m2, s.counts, { s.live[0], s.live[1] }, s.waves };
}
static BakeAdaptiveTarget bake_adaptive_target(const CtBake_ *b)
{
    return { b->d_table, b->d_m2, b->d_counts, { b->d_live[0], b->d_live[1] }, b->d_waves };
}

// m2, counts, the live lists and the wave counts of b (and the table, with_table), whose kind and active count are known.
static int bake_adaptive_reserve(CtHandle h, const CtBake_ *b, BakeAdaptiveSet &s, bool with_table, const char *who)
{
    const size_t total = (size_t)std::max<uint64_t>(1, bake_trace_total(b)), stored = (size_t)b->stored;
    if ((with_table && s.table.alloc(stored) != hipSuccess) || s.m2.alloc(stored) != hipSuccess || s.counts.alloc(stored) != hipSuccess ||
        s.live[0].alloc(total) != hipSuccess || s.live[1].alloc(total) != hipSuccess || s.waves.alloc(bake_wave_counts(total)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(h, CT_E_NOMEM, "%s: no device memory for the variances, counts and live lists of %llu stored entries", who,
                    (unsigned long long)b->stored);
    }
    return CT_OK;
}

// The parameters of an adaptive bake; nothing of the handle is touched.
static int bake_adaptive_validate(CtHandle h, const CtBakeAdaptive *p, const char *who)
{
    if (p->abi_version != CT_ABI_VERSION) {
        return fail(h, CT_E_INVAL, "%s: parameters of abi_version %u, this library is %u", who, p->abi_version, CT_ABI_VERSION);
    }
    if (p->round_samples == 0u || p->round_samples > 0xffffu) {
        return fail(h, CT_E_INVAL, "%s: round_samples %u, a round traces 1 .. 65535 experiments per entry", who, p->round_samples);
    }
    if (p->max_samples == 0u || p->max_samples % p->round_samples != 0u || p->max_samples > (1u << 24)) {
        return fail(h, CT_E_INVAL, "%s: max_samples %u; a multiple of round_samples (%u), at most 2^24", who, p->max_samples, p->round_samples);
    }
    if (!std::isfinite(p->rel_tol) || !std::isfinite(p->abs_tol) || p->rel_tol < 0.f || p->abs_tol < 0.f) {
        return fail(h, CT_E_INVAL, "%s: rel_tol and abs_tol must be finite and not negative", who);
    }
    return CT_OK;
}

// b takes over what a trace has filled (the table, when the set has one).
static void bake_adaptive_adopt(CtBake_ *b, BakeAdaptiveSet &s)
{
    if (s.table) {
        b->d_table = std::move(s.table);
    }
    b->d_m2 = std::move(s.m2);
    b->d_counts = std::move(s.counts);
    b->d_live[0] = std::move(s.live[0]);
    b->d_live[1] = std::move(s.live[1]);
    b->d_waves = std::move(s.waves);
}

// Rounds of b->ap.round_samples experiments until no entry is live or the live ones hold b->cap.  On entry the `n_live` live
// entries all hold b->samples experiments; listed: they are t.live[b->live_cur], otherwise (the first round) every stored entry
// of an active node.  The stream is idle, the tables of b's frame are uploaded, t's table, m2 and counts hold the state.  A
// round's live entries go through bake_trace's chunks (whole groups of 64: a chunk's waves are the live list's) and passes;
// behind the last fold of the round follow the scan, the compacting write into the other list and the read of the survivors'
// number, which point_launch's wait covers.  Books b's counts and times; b->live entries are left at the cap, unconverged.
// live_at: where in t.live[b->live_cur] the n_live entries begin -- a shard's sub-range of a merged list; the wave counts and the
// list a round writes start at 0 whatever it is.
static int bake_trace_adaptive(CtHandle h, CtBake_ *b, const BakeAdaptiveTarget &t, uint64_t n_live, bool listed, uint64_t live_at = 0)
{
    b->trace_ms = b->fold_ms = b->test_ms = 0;
    const uint32_t R = b->ap.round_samples, budget = bake_trace_budget(h);
    DevScene sc = h->dev;
    sc.mode = CT_MODE_SUN_MULTIPLE_SCATTER;
    Event ev[6];
    for (Event &e : ev) {
        HIPCHK(h, e.create());
    }
    CtHandle_::PointBuffers &pt = h->pt;
    const BakeAdaptiveState st{ t.table, t.m2, t.counts, b->ap.rel_tol, b->ap.abs_tol, b->ap.zero_samples };
    const double render_before = h->render_ms;
    double fold_ms = 0, test_ms = 0;
    while (n_live != 0u && b->samples < b->cap) {
        const uint32_t c = b->samples, L = (uint32_t)n_live;
        uint32_t chunk = std::min(L, std::min<uint32_t>(budget, 1u << 20));
        if (chunk >= 64u) {
            chunk &= ~63u;
        }
        const uint32_t *live_in = listed ? t.live[b->live_cur] + live_at : nullptr;
        uint32_t *live_out = t.live[listed ? b->live_cur ^ 1 : 0];
        uint32_t survivors = 0;
        for (uint32_t first = 0; first < L; first += chunk) {
            BakeTraceArgs a = bake_trace_args(b);
            a.first = first;
            a.n = std::min(chunk, L - first);
            a.n_pad = (a.n + 63u) & ~63u;
            a.live = live_in;
            const uint32_t per_pass = std::min(0xffffu, std::max(1u, budget / a.n_pad));
            for (uint32_t at = 0; at < R; at += per_pass) {
                const uint32_t passes = std::min(per_pass, R - at), done = c + at;
                const bool last_pass = at + passes == R, last = last_pass && first + a.n == L;
                const int rc = point_launch(
                    h, sc, a.n, done + 1u, passes,
                    [&]() -> int {
                        HIPCHK(h, hipEventRecord(ev[0], h->stream));
                        HIPCHK(h, launch_bake_trace_tasks(sc, a, pt.primary, pt.pixels, h->stream));
                        HIPCHK(h, hipEventRecord(ev[1], h->stream));
                        return CT_OK;
                    },
                    [&]() -> int {
                        HIPCHK(h, hipEventRecord(ev[2], h->stream));
                        HIPCHK(h, launch_bake_adaptive_fold(a, pt.frames, a.n_pad, passes, done, st, last_pass ? t.waves : nullptr, h->stream));
                        HIPCHK(h, hipEventRecord(ev[3], h->stream));
                        if (last) {
                            HIPCHK(h, hipEventRecord(ev[4], h->stream));
                            HIPCHK(h, launch_bake_adaptive_scan(t.waves, L, h->stream));
                            HIPCHK(h, launch_bake_adaptive_compact(a, st, live_in, L, t.waves, live_out, h->stream));
                            HIPCHK(h, hipEventRecord(ev[5], h->stream));
                            HIPCHK(h, hipMemcpyAsync(&survivors, t.waves + (L + 63u) / 64u, sizeof survivors, hipMemcpyDeviceToHost, h->stream));
                        }
                        return CT_OK;
                    });
                if (rc != CT_OK) {
                    return rc;
                }
                float ms0 = 0, ms1 = 0, ms2 = 0;
                HIPCHK(h, hipEventElapsedTime(&ms0, ev[0], ev[1]));
                HIPCHK(h, hipEventElapsedTime(&ms1, ev[2], ev[3]));
                if (last) {
                    HIPCHK(h, hipEventElapsedTime(&ms2, ev[4], ev[5]));
                }
                fold_ms += (double)ms0 + (double)ms1;
                test_ms += (double)ms2;
            }
        }
        if (survivors > L) {
            return fail(h, CT_E_HIP, "internal: a round of %u live entries counted %u survivors", L, survivors);
        }
        b->samples = c + R;
        b->rounds += 1u;
        b->paths += (uint64_t)L * R;
        b->live_cur = listed ? b->live_cur ^ 1 : 0;
        listed = true;
        live_at = 0;
        n_live = survivors;
        b->live = n_live;   // (with every round: a call that fails later leaves whole rounds)
    }
    b->live = n_live;
    b->trace_ms = h->render_ms - render_before;
    b->fold_ms = fold_ms;
    b->test_ms = test_ms;
    return CT_OK;
}

// An adaptive trace from nothing into t (the table, m2 and counts: b->stored values each): zeroed, the tables of b's frame as
// it is uploaded, then the rounds over every stored entry of an active node.
static int bake_trace_adaptive_fresh(CtHandle h, CtBake_ *b, const BakeAdaptiveTarget &t)
{
    return drained(h, [&]() -> int {
        HIPCHK(h, hipMemsetAsync(t.table, 0, (size_t)b->stored * sizeof(float), h->stream));
        HIPCHK(h, hipMemsetAsync(t.m2, 0, (size_t)b->stored * sizeof(float), h->stream));
        HIPCHK(h, hipMemsetAsync(t.counts, 0, (size_t)b->stored * sizeof(uint32_t), h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        const int up = bake_upload_trace_tables(h, b);
        if (up != CT_OK || b->shards == 1u) {
            return up != CT_OK ? up : bake_trace_adaptive(h, b, t, bake_trace_total(b), false);
        }
        // a bake on a group: the first round's list is the span's stored indices, written out
        const uint64_t block = (uint64_t)b->azimuths * b->cosines, n = (b->span_hi - b->span_lo) * block;
        HIPCHK(h, launch_bake_live_iota(t.live[0], (uint32_t)(b->span_lo * block), (uint32_t)n, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        b->live_cur = 0;
        return bake_trace_adaptive(h, b, t, n, true);
    });
}

// ct_network_bake, ct_network_bake_sparse and ct_network_bake_compact: one validation, one order of errors.  kind: CT_BAKE_DENSE,
// _SPARSE or _COMPACT.  trace_samples: ct_bake_traced, which takes no network (n is NULL) and fills the table with that many
// experiments per entry.  adaptive: ct_bake_traced_adaptive, traced likewise, in rounds under the stopping rule of *adaptive.
// shard of shards: ct_group_bake_*, which builds that span of the bake on this handle and exchanges the rest.
static int bake_create(CtHandle h, CtNetwork n, const CtBakeDesc *d, CtBake *out, uint32_t kind, const uint32_t *trace_samples = nullptr,
                       const CtBakeAdaptive *adaptive = nullptr, uint32_t shard = 0, uint32_t shards = 1)
{
    const bool sparse = kind != CT_BAKE_DENSE, compact = kind == CT_BAKE_COMPACT, traced = trace_samples != nullptr || adaptive != nullptr;
    const char *const who = adaptive ? "ct_bake_traced_adaptive" : traced ? "ct_bake_traced" : compact ? "ct_network_bake_compact" : sparse ? "ct_network_bake_sparse" : "ct_network_bake";
    if (!h) {
        return fail(nullptr, CT_E_INVAL, "null handle");
    }
    if ((!traced && !n) || !d || !out) {
        return fail(h, CT_E_INVAL, traced ? "%s: need a description and out" : "%s: need a network, a description and out", who);
    }
    *out = nullptr;
    if (kind != CT_BAKE_DENSE && kind != CT_BAKE_SPARSE && kind != CT_BAKE_COMPACT) {   // (the traced entry points pass theirs on)
        return fail(h, CT_E_INVAL, "%s: unknown kind %u (CT_BAKE_DENSE, CT_BAKE_SPARSE or CT_BAKE_COMPACT)", who, kind);
    }
    if (d->abi_version != CT_ABI_VERSION) {
        return fail(h, CT_E_INVAL, "%s: abi_version %u, this library is %u", who, d->abi_version, CT_ABI_VERSION);
    }
    uint64_t entries = 1;
    for (int axis = 0; axis < 3; axis++) {
        if (d->grid[axis] < 2u || d->grid[axis] > 256u) {
            return fail(h, CT_E_INVAL, "%s: grid[%d] = %u, a grid has 2 .. 256 nodes per axis", who, axis, d->grid[axis]);
        }
        entries *= d->grid[axis];
    }
    if (d->azimuths < 4u || d->azimuths > 64u || d->azimuths % 4u != 0u) {
        return fail(h, CT_E_INVAL, "%s: %u azimuths; a multiple of 4 in 4 .. 64", who, d->azimuths);
    }
    if (d->cosines < 2u || d->cosines > 64u) {
        return fail(h, CT_E_INVAL, "%s: %u cosines; 2 .. 64", who, d->cosines);
    }
    entries *= (uint64_t)d->azimuths * d->cosines;   // (<= 2^36)
    if (!compact && entries > (1ull << 26)) {        // (a compact bake bounds what it stores, once the mask has been counted)
        return fail(h, CT_E_INVAL, "%s: %llu entries, a table holds at most 2^26", who, (unsigned long long)entries);
    }
    if (trace_samples && *trace_samples > 0xffffu) {
        return fail(h, CT_E_INVAL, "%s: %u samples, one call traces at most 65535", who, *trace_samples);
    }
    if (adaptive) {
        const int rc = bake_adaptive_validate(h, adaptive, who);
        if (rc != CT_OK) {
            return rc;
        }
    }
    if (traced && (h->scene.flags & CT_FLAG_SIMPLE_KERNEL)) {
        return fail(h, CT_E_INVAL, "%s: point radiance tasks need the persistent kernel", who);
    }
    NEED_NOFLUSH(h);
    int rc = traced ? CT_OK : net_validate_network(h, n, who);
    if (rc != CT_OK) {
        return rc;
    }
    rc = flush(h);
    if (rc != CT_OK) {
        return rc;
    }
    std::unique_ptr<CtBake_> made(new CtBake_());   // (every return but the last deletes it)
    CtBake_ *const b = made.get();
    static_cast<BakeShape &>(*b) = bake_shape(h, d->grid, d->azimuths, d->cosines, kind, traced);
    if (!compact && b->d_table.alloc((size_t)entries) != hipSuccess) {   // (before the first kernel)
        (void)hipGetLastError();
        return fail(h, CT_E_NOMEM, "%s: no device memory for a table of %llu entries", who, (unsigned long long)entries);
    }
    if (traced && (b->d_dirs.alloc(bake_dir_floats(*b)) != hipSuccess || (!sparse && b->d_probe.alloc(bake_probe_floats(*b)) != hipSuccess))) {
        (void)hipGetLastError();
        return fail(h, CT_E_NOMEM, "%s: no device memory for the direction and probe tables", who);
    }
    double mask_ms = 0;
    if (sparse) {   // the mask's temporaries, the node bytes, the list, the slots and the record tables: all before the first kernel, too
        BakeMask m;
        rc = bake_mask_reserve(h, b->grid, m, compact);
        if (rc == CT_OK && b->d_probe.alloc(bake_probe_floats(*b)) != hipSuccess) {
            (void)hipGetLastError();
            rc = fail(h, CT_E_NOMEM, "%s: no device memory for the probe tables", who);
        }
        uint32_t active = 0;
        if (rc == CT_OK) {
            rc = bake_mask_run(h, b->grid, m, &active, &mask_ms);
        }
        if (rc == CT_OK && compact) {
            // The one allocation behind a kernel: the stored table has the size the mask has counted.  Still before any gather or
            // network kernel, and nothing of the handle has changed.
            b->stored = ((uint64_t)active + 1u) * b->azimuths * b->cosines;
            if (b->stored > (1ull << 26)) {
                rc = fail(h, CT_E_INVAL, "%s: %u active nodes of %llu store %llu entries, a table holds at most 2^26 (%llu)", who, active,
                          (unsigned long long)(entries / b->azimuths / b->cosines), (unsigned long long)b->stored, 1ull << 26);
            } else if (b->d_table.alloc((size_t)b->stored) != hipSuccess) {
                (void)hipGetLastError();
                rc = fail(h, CT_E_NOMEM, "%s: no device memory for a table of %llu stored entries", who, (unsigned long long)b->stored);
            }
        }
        if (rc != CT_OK) {
            return rc;
        }
        bake_adopt_mask(b, m, active);
    }
    if (shards != 1u) {   // (a bake on a group: the nodes it covers are counted now)
        rc = bake_cut(h, b, shard, shards);
        if (rc != CT_OK) {
            return rc;
        }
    }
    BakeAdaptiveSet set;
    if (adaptive) {   // (a dense bake: no kernel has run yet; the others: behind the mask's count, like the compact table)
        b->adaptive = true;
        b->ap = *adaptive;
        b->cap = adaptive->max_samples;
        rc = bake_adaptive_reserve(h, b, set, false, who);
        if (rc != CT_OK) {
            return rc;
        }
    }
    bake_frame(h, b);
    if (adaptive) {
        rc = bake_trace_adaptive_fresh(h, b, bake_adaptive_target(b->d_table, set));
        bake_adaptive_adopt(b, set);
    } else if (traced) {
        rc = bake_trace_fresh(h, b, b->d_table, *trace_samples);
    } else {
        rc = bake_run(h, n, b, b->d_table);
    }
    b->mask_ms += mask_ms;   // (bake_run has set it to its record kernel's time)
    if (rc != CT_OK) {
        return rc;
    }
    *out = made.release();
    return CT_OK;
}

extern "C" int ct_network_bake(CtHandle h, CtNetwork n, const CtBakeDesc *d, CtBake *out)
{
    return bake_create(h, n, d, out, CT_BAKE_DENSE);
}

extern "C" int ct_network_bake_sparse(CtHandle h, CtNetwork n, const CtBakeDesc *d, CtBake *out)
{
    return bake_create(h, n, d, out, CT_BAKE_SPARSE);
}

extern "C" int ct_network_bake_compact(CtHandle h, CtNetwork n, const CtBakeDesc *d, CtBake *out)
{
    return bake_create(h, n, d, out, CT_BAKE_COMPACT);
}

extern "C" int ct_bake_traced(CtHandle h, const CtBakeDesc *d, uint32_t kind, uint32_t samples, CtBake *out)
{
    return bake_create(h, nullptr, d, out, kind, &samples);
}

extern "C" int ct_bake_storage_info(CtBake b, CtBakeStorageInfo *out)
{
    if (!b || !out) {
        return fail(b ? b->h : nullptr, CT_E_INVAL, "ct_bake_storage_info: need a bake and out");
    }
    *out = CtBakeStorageInfo{};
    const uint64_t nodes = bake_nodes(*b);
    out->compact = b->compact ? 1u : 0u;
    out->slots = b->compact ? b->active + 1u : nodes;
    out->stored_entries = b->stored;
    out->table_bytes = (b->half ? 2u : 4u) * b->stored;
    out->index_bytes = b->compact ? 4u * nodes : 0u;
    return CT_OK;
}

// The stored table as b->stored floats on the host: a half bake's values widened, which is exact.
static int bake_stored_floats(CtHandle h, const CtBake_ *b, float *out)
{
    if (!b->half) {
        HIPCHK(h, hipMemcpy(out, b->d_table, (size_t)b->stored * sizeof(float), hipMemcpyDeviceToHost));
        return CT_OK;
    }
    std::vector<uint16_t> bits((size_t)b->stored);
    HIPCHK(h, hipMemcpy(bits.data(), b->d_half, bits.size() * sizeof(uint16_t), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < bits.size(); i++) {
        out[i] = half_widen(bits[i]);
    }
    return CT_OK;
}

// A half bake is final (include/cloudtrace.h, "half tables").
static int bake_half_final(CtHandle h, CtBake b, const char *who)
{
    return b->half ? fail(h, CT_E_INVAL, "%s: a half bake is final; bake again from float32 and take ct_bake_half of that", who) : CT_OK;
}

extern "C" int ct_bake_slots(CtBake b, uint32_t *slots_host_out, size_t count)
{
    if (!b) {
        return fail(nullptr, CT_E_INVAL, "ct_bake_slots: null bake");
    }
    CtHandle h = b->h;
    if (!b->compact) {
        return fail(h, CT_E_INVAL, "ct_bake_slots: only a bake of ct_network_bake_compact has slots");
    }
    const size_t nodes = (size_t)bake_nodes(*b);
    if (!slots_host_out || count != nodes) {
        return fail(h, CT_E_INVAL, "ct_bake_slots: need an array of exactly %llu words", (unsigned long long)nodes);
    }
    NEED(h);
    HIPCHK(h, hipMemcpy(slots_host_out, b->d_slots, nodes * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return CT_OK;
}

extern "C" int ct_bake_download_stored(CtBake b, float *table_host_out, size_t count)
{
    if (!b) {
        return fail(nullptr, CT_E_INVAL, "ct_bake_download_stored: null bake");
    }
    CtHandle h = b->h;
    if (!b->compact) {
        return fail(h, CT_E_INVAL, "ct_bake_download_stored: only a bake of ct_network_bake_compact has a stored table; ct_bake_download");
    }
    if (!table_host_out || count != b->stored) {
        return fail(h, CT_E_INVAL, "ct_bake_download_stored: need an array of exactly %llu floats", (unsigned long long)b->stored);
    }
    NEED(h);
    return bake_stored_floats(h, b, table_host_out);
}

extern "C" int ct_bake_sparse_info(CtBake b, CtBakeSparseInfo *out)
{
    if (!b || !out) {
        return fail(b ? b->h : nullptr, CT_E_INVAL, "ct_bake_sparse_info: need a bake and out");
    }
    *out = CtBakeSparseInfo{};
    out->sparse = b->sparse ? 1u : 0u;
    out->margin_texels = b->margin;
    out->nodes = bake_nodes(*b);
    out->active_nodes = b->sparse ? b->active : out->nodes;
    out->probes_baked = out->active_nodes * b->azimuths;
    out->mask_ms = b->mask_ms;
    return CT_OK;
}

extern "C" int ct_bake_mask(CtBake b, uint8_t *nodes_host_out, size_t count)
{
    if (!b) {
        return fail(nullptr, CT_E_INVAL, "ct_bake_mask: null bake");
    }
    CtHandle h = b->h;
    const size_t nodes = (size_t)bake_nodes(*b);
    if (!nodes_host_out || count != nodes) {
        return fail(h, CT_E_INVAL, "ct_bake_mask: need an array of exactly %llu bytes", (unsigned long long)nodes);
    }
    if (!b->sparse) {
        std::fill(nodes_host_out, nodes_host_out + nodes, (uint8_t)1);
        return CT_OK;
    }
    NEED(h);
    HIPCHK(h, hipMemcpy(nodes_host_out, b->d_nodes, nodes, hipMemcpyDeviceToHost));
    return CT_OK;
}

extern "C" int ct_debug_bake_mask(CtHandle h, const uint32_t grid[3], uint8_t *cells_host_out, uint8_t *nodes_host_out,
                                  uint32_t *active_host_out, uint32_t capacity, uint32_t *count_out)
{
    const char *const who = "ct_debug_bake_mask";
    if (!h) {
        return fail(nullptr, CT_E_INVAL, "null handle");
    }
    if (!grid || !count_out) {
        return fail(h, CT_E_INVAL, "%s: need a grid and count_out", who);
    }
    *count_out = 0;
    for (int axis = 0; axis < 3; axis++) {
        if (grid[axis] < 2u || grid[axis] > 256u) {
            return fail(h, CT_E_INVAL, "%s: grid[%d] = %u, a grid has 2 .. 256 nodes per axis", who, axis, grid[axis]);
        }
    }
    NEED(h);
    BakeMask m;
    int rc = bake_mask_reserve(h, grid, m);
    uint32_t active = 0;
    double ms = 0;
    if (rc == CT_OK) {
        rc = bake_mask_run(h, grid, m, &active, &ms);
    }
    if (rc != CT_OK) {
        return rc;
    }
    *count_out = active;
    if (active_host_out && capacity < active) {
        return fail(h, CT_E_INVAL, "%s: %u active nodes do not fit a capacity of %u", who, active, capacity);
    }
    const size_t cells = (size_t)(grid[0] - 1u) * (grid[1] - 1u) * (grid[2] - 1u), nodes = (size_t)grid[0] * grid[1] * grid[2];
    if (cells_host_out) {
        HIPCHK(h, hipMemcpy(cells_host_out, m.cells, cells, hipMemcpyDeviceToHost));
    }
    if (nodes_host_out) {
        HIPCHK(h, hipMemcpy(nodes_host_out, m.nodes, nodes, hipMemcpyDeviceToHost));
    }
    if (active_host_out && active != 0u) {
        HIPCHK(h, hipMemcpy(active_host_out, m.list, (size_t)active * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    return CT_OK;
}

// The transaction of ct_bake_update, ct_bake_retrace and ct_bake_retrace_adaptive: `fill` writes a second set of arrays, which
// the caller allocated and adopts on success, under b's frame for the handle's light as it is now.  A failure leaves the old
// arrays and puts the state back as it was; a traced bake's device tables are the old frame's again, and the text of the first
// error stays unless that upload fails too.
template <typename F>
static int bake_refill(CtHandle h, CtBake_ *b, F &&fill)
{
    const BakeState before = *b;
    bake_frame(h, b);
    const int rc = fill();
    if (rc != CT_OK) {
        const std::string text = h->error;
        static_cast<BakeState &>(*b) = before;
        if (!b->traced || bake_upload_trace_tables(h, b) == CT_OK) {
            h->error = text;
        }
    }
    return rc;
}

// What ct_bake_update checks before it flushes, in this order.
static int bake_update_checks(CtHandle h, CtNetwork n, CtBake b, const char *who)
{
    if (!h) {
        return fail(nullptr, CT_E_INVAL, "null handle");
    }
    if (!n || !b) {
        return fail(h, CT_E_INVAL, "%s: need a network and a bake", who);
    }
    NEED_NOFLUSH(h);
    int rc = net_validate_network(h, n, who);
    if (rc != CT_OK) {
        return rc;
    }
    if (b->h != h) {
        return fail(h, CT_E_INVAL, "%s: the bake was made on another handle", who);
    }
    rc = bake_half_final(h, b, who);
    if (rc != CT_OK) {
        return rc;
    }
    if (b->traced) {
        return fail(h, CT_E_INVAL, "%s: a traced bake holds no network's outputs; %s traces it again", who,
                    b->adaptive ? "ct_bake_retrace_adaptive" : "ct_bake_retrace");
    }
    return CT_OK;
}

extern "C" int ct_bake_update(CtHandle h, CtNetwork n, CtBake b)
{
    const char *const who = "ct_bake_update";
    int rc = bake_update_checks(h, n, b, who);
    if (rc == CT_OK) {
        rc = flush(h);
    }
    if (rc != CT_OK) {
        return rc;
    }
    // into a second table: a failure leaves the old table, its light and its frame as they were
    DevBuf<float> fresh;
    if (fresh.alloc((size_t)b->stored) != hipSuccess) {   // (a compact bake: its stored table; list and slots are reused)
        (void)hipGetLastError();
        return fail(h, CT_E_NOMEM, "%s: no device memory for a table of %llu entries", who, (unsigned long long)b->stored);
    }
    rc = bake_refill(h, b, [&]() -> int { return bake_run(h, n, b, fresh); });
    if (rc == CT_OK) {
        b->d_table = std::move(fresh);
    }
    return rc;
}

// How the four calls that trace a bake further or again open, in this order; the device is set, nothing is flushed.
static int bake_own_checks(CtHandle h, CtBake b, const char *who)
{
    if (!h) {
        return fail(nullptr, CT_E_INVAL, "null handle");
    }
    if (!b) {
        return fail(h, CT_E_INVAL, "%s: need a bake", who);
    }
    NEED_NOFLUSH(h);
    const int rc = bake_foreign(h, b, who);
    return rc != CT_OK ? rc : bake_half_final(h, b, who);
}

// What ct_bake_trace_more and ct_bake_retrace check alike, in this order.
static int bake_trace_checks(CtHandle h, CtBake b, uint32_t samples, const char *who)
{
    const int rc = bake_own_checks(h, b, who);
    if (rc != CT_OK) {
        return rc;
    }
    if (!b->traced) {
        return fail(h, CT_E_INVAL, "%s: the bake holds a network's outputs; ct_bake_update bakes it again", who);
    }
    if (b->adaptive) {
        return fail(h, CT_E_INVAL, "%s: the entries of an adaptive bake hold different counts; ct_bake_trace_adaptive_more raises its cap, "
                                   "ct_bake_retrace_adaptive traces it again", who);
    }
    if (samples == 0u || samples > 0xffffu) {
        return fail(h, CT_E_INVAL, "%s: %u samples, a call traces 1 .. 65535", who, samples);
    }
    return CT_OK;
}

static int bake_trace_more_checks(CtHandle h, CtBake b, uint32_t samples, const char *who)
{
    const int rc = bake_trace_checks(h, b, samples, who);
    if (rc != CT_OK) {
        return rc;
    }
    if ((uint64_t)b->samples + samples > (1ull << 24)) {
        return fail(h, CT_E_INVAL, "%s: %u samples behind %u, an entry holds at most 2^24 experiments", who, samples, b->samples);
    }
    if (b->epoch != h->light_epoch) {
        return fail(h, CT_E_STATE, "%s: the handle's light has changed since the bake; ct_bake_retrace traces it again", who);
    }
    return CT_OK;
}

extern "C" int ct_bake_trace_more(CtHandle h, CtBake b, uint32_t samples)
{
    int rc = bake_trace_more_checks(h, b, samples, "ct_bake_trace_more");
    if (rc == CT_OK) {
        rc = flush(h);
    }
    if (rc != CT_OK) {
        return rc;
    }
    return drained(h, [&]() -> int {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return bake_trace(h, b, b->d_table, samples);
    });
}

extern "C" int ct_bake_retrace(CtHandle h, CtBake b, uint32_t samples)
{
    const char *const who = "ct_bake_retrace";
    int rc = bake_trace_checks(h, b, samples, who);
    if (rc == CT_OK) {
        rc = flush(h);
    }
    if (rc != CT_OK) {
        return rc;
    }
    // into a second table, as ct_bake_update: a failure leaves the old table, its frame and its sample count as they were
    DevBuf<float> fresh;
    if (fresh.alloc((size_t)b->stored) != hipSuccess) {
        (void)hipGetLastError();
        return fail(h, CT_E_NOMEM, "%s: no device memory for a table of %llu entries", who, (unsigned long long)b->stored);
    }
    rc = bake_refill(h, b, [&]() -> int {
        b->samples = 0;
        b->paths = 0;
        return bake_trace_fresh(h, b, fresh, samples);
    });
    if (rc == CT_OK) {
        b->d_table = std::move(fresh);
    }
    return rc;
}

extern "C" int ct_bake_trace_info(CtBake b, CtBakeTraceInfo *out)
{
    if (!b || !out) {
        return fail(b ? b->h : nullptr, CT_E_INVAL, "ct_bake_trace_info: need a bake and out");
    }
    *out = CtBakeTraceInfo{};
    if (b->traced) {
        out->traced = 1u;
        out->samples = b->samples;
        out->paths = b->paths;
        out->trace_ms = b->trace_ms;
        out->fold_ms = b->fold_ms;
    }
    return CT_OK;
}

extern "C" int ct_bake_traced_adaptive(CtHandle h, const CtBakeDesc *d, uint32_t kind, const CtBakeAdaptive *p, CtBake *out)
{
    const char *const who = "ct_bake_traced_adaptive";
    if (!h) {
        return fail(nullptr, CT_E_INVAL, "null handle");
    }
    if (!d || !p || !out) {   // (bake_create tells an adaptive bake by p)
        return fail(h, CT_E_INVAL, "%s: need a description, parameters and out", who);
    }
    return bake_create(h, nullptr, d, out, kind, nullptr, p);
}

// What ct_bake_trace_adaptive_more and ct_bake_retrace_adaptive check alike, in this order.
static int bake_adaptive_checks(CtHandle h, CtBake b, const char *who)
{
    const int rc = bake_own_checks(h, b, who);
    if (rc != CT_OK) {
        return rc;
    }
    if (!b->adaptive) {
        return fail(h, CT_E_INVAL, "%s: the bake was not made by ct_bake_traced_adaptive; %s", who,
                    b->traced ? "ct_bake_trace_more / ct_bake_retrace trace it" : "ct_bake_update bakes it again");
    }
    return CT_OK;
}

static int bake_adaptive_more_checks(CtHandle h, CtBake b, uint32_t max_samples, const char *who)
{
    const int rc = bake_adaptive_checks(h, b, who);
    if (rc != CT_OK) {
        return rc;
    }
    if (max_samples <= b->cap || max_samples % b->ap.round_samples != 0u || max_samples > (1u << 24)) {
        return fail(h, CT_E_INVAL, "%s: max_samples %u; a multiple of round_samples (%u) above the cap in force (%u), at most 2^24", who,
                    max_samples, b->ap.round_samples, b->cap);
    }
    if (b->epoch != h->light_epoch) {
        return fail(h, CT_E_STATE, "%s: the handle's light has changed since the bake; ct_bake_retrace_adaptive traces it again", who);
    }
    return CT_OK;
}

extern "C" int ct_bake_trace_adaptive_more(CtHandle h, CtBake b, uint32_t max_samples)
{
    int rc = bake_adaptive_more_checks(h, b, max_samples, "ct_bake_trace_adaptive_more");
    if (rc == CT_OK) {
        rc = flush(h);
    }
    if (rc != CT_OK) {
        return rc;
    }
    // (in place, like ct_bake_trace_more: a failure between two rounds leaves the rounds that were completed)
    return drained(h, [&]() -> int {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        uint64_t at = 0, n_live = b->live;
        if (b->shards != 1u && n_live != 0u) {   // a bake on a group: the span's sub-range of the merged or loaded list
            const uint64_t block = (uint64_t)b->azimuths * b->cosines;
            uint32_t bounds[2] = { 0, 0 };
            HIPCHK(h, launch_bake_live_bounds(b->d_live[b->live_cur], (uint32_t)n_live, (uint32_t)(b->span_lo * block),
                                              (uint32_t)(b->span_hi * block), b->d_waves, h->stream));
            HIPCHK(h, hipMemcpyAsync(bounds, b->d_waves, sizeof bounds, hipMemcpyDeviceToHost, h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));
            if (bounds[0] > bounds[1] || bounds[1] > n_live) {
                return fail(h, CT_E_HIP, "internal: a live list of %llu entries gave the span %u .. %u", (unsigned long long)n_live, bounds[0], bounds[1]);
            }
            at = bounds[0];
            n_live = bounds[1] - bounds[0];
        }
        b->cap = max_samples;
        return bake_trace_adaptive(h, b, bake_adaptive_target(b), n_live, true, at);
    });
}

extern "C" int ct_bake_retrace_adaptive(CtHandle h, CtBake b)
{
    const char *const who = "ct_bake_retrace_adaptive";
    int rc = bake_adaptive_checks(h, b, who);
    if (rc == CT_OK) {
        rc = flush(h);
    }
    if (rc != CT_OK) {
        return rc;
    }
    // into a second table, m2, counts and pair of live lists: a failure leaves the bake as it was
    BakeAdaptiveSet fresh;
    rc = bake_adaptive_reserve(h, b, fresh, true, who);
    if (rc != CT_OK) {
        return rc;
    }
    rc = bake_refill(h, b, [&]() -> int {
        b->samples = b->rounds = 0;
        b->paths = b->live = 0;
        return bake_trace_adaptive_fresh(h, b, bake_adaptive_target(fresh.table, fresh));
    });
    if (rc == CT_OK) {
        bake_adaptive_adopt(b, fresh);
    }
    return rc;
}

extern "C" int ct_bake_adaptive_info(CtBake b, CtBakeAdaptiveInfo *out)
{
    if (!b || !out) {
        return fail(b ? b->h : nullptr, CT_E_INVAL, "ct_bake_adaptive_info: need a bake and out");
    }
    *out = CtBakeAdaptiveInfo{};
    if (b->adaptive) {
        out->adaptive = 1u;
        out->round_samples = b->ap.round_samples;
        out->max_samples = b->cap;
        out->zero_samples = b->ap.zero_samples;
        out->rel_tol = b->ap.rel_tol;
        out->abs_tol = b->ap.abs_tol;
        out->rounds = b->rounds;
        out->entries_active = bake_trace_total(b);
        out->capped = b->live;
        out->converged = b->rounds != 0u ? out->entries_active - b->live : 0u;
        out->paths = b->paths;
        out->trace_ms = b->trace_ms;
        out->fold_ms = b->fold_ms;
        out->test_ms = b->test_ms;
    }
    return CT_OK;
}

// ct_bake_download_counts and ct_bake_download_m2: `count` words of an adaptive bake's array, as stored.
static int bake_adaptive_download(CtBake b, const void *dev, void *host_out, size_t count, const char *who)
{
    if (!b) {
        return fail(nullptr, CT_E_INVAL, "%s: null bake", who);
    }
    CtHandle h = b->h;
    if (!b->adaptive) {
        return fail(h, CT_E_INVAL, "%s: only a bake of ct_bake_traced_adaptive keeps counts and variances", who);
    }
    if (!host_out || count != b->stored) {
        return fail(h, CT_E_INVAL, "%s: need an array of exactly %llu values", who, (unsigned long long)b->stored);
    }
    NEED(h);
    HIPCHK(h, hipMemcpy(host_out, dev, count * 4u, hipMemcpyDeviceToHost));
    return CT_OK;
}

extern "C" int ct_bake_download_counts(CtBake b, uint32_t *counts_host_out, size_t count)
{
    return bake_adaptive_download(b, b ? b->d_counts.get() : nullptr, counts_host_out, count, "ct_bake_download_counts");
}

extern "C" int ct_bake_download_m2(CtBake b, float *m2_host_out, size_t count)
{
    return bake_adaptive_download(b, b ? b->d_m2.get() : nullptr, m2_host_out, count, "ct_bake_download_m2");
}

extern "C" int ct_bake_directions(CtBake b, float *directions_host_out, size_t count)
{
    if (!b) {
        return fail(nullptr, CT_E_INVAL, "ct_bake_directions: null bake");
    }
    const size_t floats = bake_dir_floats(*b);
    if (!directions_host_out || count != floats) {
        return fail(b->h, CT_E_INVAL, "ct_bake_directions: need an array of exactly %llu floats", (unsigned long long)floats);
    }
    std::vector<float> dirs;
    bake_directions(b, dirs);
    std::copy(dirs.begin(), dirs.end(), directions_host_out);
    return CT_OK;
}

extern "C" int ct_bake_destroy(CtBake b)
{
    if (!b) {
        return CT_OK;
    }
    hipSetDevice(b->device);
    delete b;
    return CT_OK;
}

extern "C" int ct_bake_info(CtBake b, CtBakeInfo *out)
{
    if (!b || !out) {
        return fail(b ? b->h : nullptr, CT_E_INVAL, "ct_bake_info: need a bake and out");
    }
    *out = CtBakeInfo{};
    for (int axis = 0; axis < 3; axis++) {
        out->grid[axis] = b->grid[axis];
        out->light[axis] = b->l[axis];
        out->axis_a[axis] = b->a[axis];
        out->axis_b[axis] = b->b[axis];
    }
    out->azimuths = b->azimuths;
    out->cosines = b->cosines;
    out->entries = b->entries;
    for (uint32_t k = 0; k < b->cosines; k++) {
        out->cosine[k] = b->cosine[k];
    }
    out->current = b->epoch == b->h->light_epoch ? 1u : 0u;
    out->gather_ms = b->gather_ms;
    out->network_ms = b->network_ms;
    return CT_OK;
}

extern "C" int ct_bake_probes(CtBake b, uint64_t first, uint32_t count, float *positions_host_out, float *directions_host_out)
{
    if (!b) {
        return fail(nullptr, CT_E_INVAL, "ct_bake_probes: null bake");
    }
    if (!positions_host_out || !directions_host_out) {
        return fail(b->h, CT_E_INVAL, "ct_bake_probes: need two output arrays");
    }
    const uint64_t probes = bake_probes_total(b);
    if (first > probes || count > probes - first) {
        return fail(b->h, CT_E_INVAL, "ct_bake_probes: probes %llu .. +%u of %llu", (unsigned long long)first, count,
                    (unsigned long long)probes);
    }
    for (uint32_t i = 0; i < count; i++) {
        bake_probe(b, first + i, positions_host_out + 3 * (size_t)i, directions_host_out + 3 * (size_t)i);
    }
    return CT_OK;
}

extern "C" int ct_bake_download(CtBake b, float *table_host_out, size_t count)
{
    if (!b) {
        return fail(nullptr, CT_E_INVAL, "ct_bake_download: null bake");
    }
    CtHandle h = b->h;
    if (!table_host_out || count != b->entries) {
        return fail(h, CT_E_INVAL, "ct_bake_download: need an array of exactly %llu floats", (unsigned long long)b->entries);
    }
    NEED(h);
    if (b->compact) {   // expanded on the host: zeros off the mask, the stored blocks on it -- the sparse bake's table
        const size_t block = (size_t)b->azimuths * b->cosines, nodes = (size_t)bake_nodes(*b);
        std::vector<float> stored((size_t)b->stored);
        std::vector<uint32_t> slots(nodes);
        const int rc = bake_stored_floats(h, b, stored.data());
        if (rc != CT_OK) {
            return rc;
        }
        HIPCHK(h, hipMemcpy(slots.data(), b->d_slots, nodes * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (size_t node = 0; node < nodes; node++) {
            if (slots[node] > b->active) {
                return fail(h, CT_E_HIP, "internal: node %llu has slot %u of %llu", (unsigned long long)node, slots[node],
                            (unsigned long long)b->active + 1u);
            }
            std::copy_n(stored.data() + slots[node] * block, block, table_host_out + node * block);
        }
        return CT_OK;
    }
    return bake_stored_floats(h, b, table_host_out);
}

// A bake that belongs to h and holds h's light: CT_E_INVAL / CT_E_STATE otherwise.
int ct::bake_foreign(CtHandle h, CtBake b, const char *who)
{
    return b->h == h ? CT_OK : fail(h, CT_E_INVAL, "%s: the bake was made on another handle", who);
}
int ct::bake_stale(CtHandle h, CtBake b, const char *who)
{
    if (b->epoch != h->light_epoch) {
        return fail(h, CT_E_STATE, "%s: the handle's light has changed since the bake; %s", who,
                    b->half ? "a half bake is final: bake again from float32" : b->adaptive ? "ct_bake_retrace_adaptive traces it again" : b->traced ? "ct_bake_retrace traces it again"
                                                                                           : "ct_bake_update bakes it again");
    }
    return CT_OK;
}

extern "C" int ct_debug_bake_lookup(CtHandle h, CtBake b, const float *positions_dev, const float *directions_dev, uint32_t count,
                                    float *out_dev)
{
    const char *const who = "ct_debug_bake_lookup";
    if (!h) {
        return fail(nullptr, CT_E_INVAL, "null handle");
    }
    if (!b || (count != 0u && (!positions_dev || !directions_dev || !out_dev))) {
        return fail(h, CT_E_INVAL, "%s: need a bake, positions, directions and an output array", who);
    }
    NEED_NOFLUSH(h);
    int rc = bake_foreign(h, b, who);
    if (rc == CT_OK) {
        rc = bake_stale(h, b, who);
    }
    if (rc == CT_OK) {
        rc = flush(h);
    }
    if (rc != CT_OK || count == 0u) {
        return rc;
    }
    HIPCHK(h, launch_bake_lookup(h->dev, bake_table(b), positions_dev, directions_dev, count, out_dev, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return CT_OK;
}

// ---- half tables (ct_bake_half) and bake files (ct_bake_save, ct_bake_file_info, ct_bake_load): DESIGN 8 f-18 ----------------------
extern "C" uint16_t ct_debug_half_round(float x)
{
    return half_round_bits(float_bits(x));
}

extern "C" int ct_bake_format(CtBake b, uint32_t *format_out)
{
    if (!b || !format_out) {
        return fail(b ? b->h : nullptr, CT_E_INVAL, "ct_bake_format: need a bake and format_out");
    }
    *format_out = b->half ? CT_BAKE_F16 : CT_BAKE_F32;
    return CT_OK;
}

extern "C" int ct_bake_download_half(CtBake b, uint16_t *table_host_out, size_t count)
{
    if (!b) {
        return fail(nullptr, CT_E_INVAL, "ct_bake_download_half: null bake");
    }
    CtHandle h = b->h;
    if (!b->half) {
        return fail(h, CT_E_INVAL, "ct_bake_download_half: a float32 bake holds no binary16 table; ct_bake_half makes one");
    }
    if (!table_host_out || count != b->stored) {
        return fail(h, CT_E_INVAL, "ct_bake_download_half: need an array of exactly %llu values", (unsigned long long)b->stored);
    }
    NEED(h);
    HIPCHK(h, hipMemcpy(table_host_out, b->d_half, count * sizeof(uint16_t), hipMemcpyDeviceToHost));
    return CT_OK;
}

// What a bake is apart from its table, m2, counts and live lists: the scalars, and copies of the node bytes, the list, the
// slots and the probe and direction tables.  Everything is allocated before the first copy; the copies are enqueued on h's stream.
template <typename T>
static bool bake_dup_alloc(DevBuf<T> &dst, const DevBuf<T> &src)
{
    return src.capacity() == 0u || dst.alloc(src.capacity()) == hipSuccess;
}
template <typename T>
static hipError_t bake_dup_copy(CtHandle h, DevBuf<T> &dst, const DevBuf<T> &src)
{
    return src.capacity() == 0u ? hipSuccess : hipMemcpyAsync(dst, src, src.capacity() * sizeof(T), hipMemcpyDeviceToDevice, h->stream);
}

extern "C" int ct_bake_half(CtHandle h, CtBake src, CtBake *out)
{
    const char *const who = "ct_bake_half";
    if (!h) {
        return fail(nullptr, CT_E_INVAL, "null handle");
    }
    if (!src || !out) {
        return fail(h, CT_E_INVAL, "%s: need a bake and out", who);
    }
    *out = nullptr;
    NEED_NOFLUSH(h);
    int rc = bake_foreign(h, src, who);
    if (rc == CT_OK) {
        rc = bake_half_final(h, src, who);
    }
    if (rc == CT_OK) {
        rc = flush(h);
    }
    if (rc != CT_OK) {
        return rc;
    }
    std::unique_ptr<CtBake_> made(new CtBake_());   // (every return but the last deletes it)
    CtBake_ *const b = made.get();
    static_cast<BakeShape &>(*b) = *src;   // (src->h is h)
    static_cast<BakeState &>(*b) = *src;   // the frame, its epoch, samples and paths; the times and the adaptive state are not carried
    b->gather_ms = b->network_ms = b->mask_ms = b->trace_ms = b->fold_ms = b->test_ms = 0;
    b->cap = b->rounds = 0;
    b->live = 0;
    b->live_cur = 0;
    b->half = true;
    DevBuf<uint32_t> refused;   // [0] the values refused, [1] the first of them
    if (b->d_half.alloc((size_t)b->stored) != hipSuccess || refused.alloc(2) != hipSuccess || !bake_dup_alloc(b->d_nodes, src->d_nodes) ||
        !bake_dup_alloc(b->d_list, src->d_list) || !bake_dup_alloc(b->d_slots, src->d_slots) || !bake_dup_alloc(b->d_probe, src->d_probe) ||
        !bake_dup_alloc(b->d_dirs, src->d_dirs)) {
        (void)hipGetLastError();
        return fail(h, CT_E_NOMEM, "%s: no device memory for a half table of %llu stored entries", who, (unsigned long long)src->stored);
    }
    uint32_t count = 0, first = 0;
    rc = drained(h, [&]() -> int {
        HIPCHK(h, bake_dup_copy(h, b->d_nodes, src->d_nodes));
        HIPCHK(h, bake_dup_copy(h, b->d_list, src->d_list));
        HIPCHK(h, bake_dup_copy(h, b->d_slots, src->d_slots));
        HIPCHK(h, bake_dup_copy(h, b->d_probe, src->d_probe));
        HIPCHK(h, bake_dup_copy(h, b->d_dirs, src->d_dirs));
        HIPCHK(h, hipMemsetAsync(refused, 0, sizeof(uint32_t), h->stream));
        HIPCHK(h, hipMemsetAsync(refused + 1, 0xff, sizeof(uint32_t), h->stream));
        HIPCHK(h, launch_bake_half_convert(src->d_table, (uint32_t)b->stored, b->d_half, refused, h->stream));   // (stored <= 2^26)
        HIPCHK(h, hipMemcpyAsync(&count, refused, sizeof count, hipMemcpyDeviceToHost, h->stream));             // the one 4-byte read
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (count != 0u) {   // (only the refusal reads a second word)
            HIPCHK(h, hipMemcpy(&first, refused + 1, sizeof first, hipMemcpyDeviceToHost));
        }
        return CT_OK;
    });
    if (rc == CT_OK && count != 0u) {
        rc = fail(h, CT_E_INVAL, "%s: %u stored values are NaN, infinite or round to an infinity (|v| >= 65520), the first at stored index %u", who,
                  count, first);
    }
    if (rc != CT_OK) {
        return rc;
    }
    *out = made.release();
    return CT_OK;
}

// The handle's volume hash, reduced on the device in whatever order the waves run (the sum is exact).  Nothing is in flight.
static int bake_volume_hash(CtHandle h, uint64_t *hash_out)
{
    DevBuf<unsigned long long> sum;
    HIPCHK(h, sum.alloc(1));
    unsigned long long host = 0;
    const uint64_t texels = (uint64_t)h->scene.dims[0] * h->scene.dims[1] * h->scene.dims[2];
    return drained(h, [&]() -> int {
        HIPCHK(h, hipMemsetAsync(sum, 0, sizeof host, h->stream));
        HIPCHK(h, launch_volume_hash(h->d_density, texels, sum, h->stream));
        HIPCHK(h, hipMemcpyAsync(&host, sum, sizeof host, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        *hash_out = host;
        return CT_OK;
    });
}

extern "C" int ct_debug_volume_hash(CtHandle h, uint64_t *hash_out)
{
    if (!h) {
        return fail(nullptr, CT_E_INVAL, "null handle");
    }
    if (!hash_out) {
        return fail(h, CT_E_INVAL, "ct_debug_volume_hash: need hash_out");
    }
    NEED(h);
    return bake_volume_hash(h, hash_out);
}

// The header of b's file, the volume hash apart (a zeroed header is the caller's), and its mirror: the shape and the state of a
// bake on h from a header the parser has passed.  A header field is written here and read there.
static void bake_to_header(const CtBake_ *b, CtBakeFileHeader &hd)
{
    CtHandle h = b->h;
    std::memcpy(hd.magic, CT_BAKE_FILE_MAGIC, 8);
    hd.version = CT_BAKE_FILE_VERSION;
    hd.header_bytes = sizeof hd;
    hd.kind = b->compact ? CT_BAKE_COMPACT : b->sparse ? CT_BAKE_SPARSE : CT_BAKE_DENSE;   // (bake_shape reads it back)
    hd.format = b->half ? CT_BAKE_F16 : CT_BAKE_F32;
    hd.traced = b->traced ? 1u : 0u;
    hd.adaptive = b->adaptive ? 1u : 0u;
    for (int axis = 0; axis < 3; axis++) {
        hd.grid[axis] = b->grid[axis];
        hd.light[axis] = b->l[axis];
        hd.axis_a[axis] = b->a[axis];
        hd.axis_b[axis] = b->b[axis];
        hd.dims[axis] = h->scene.dims[axis];
        hd.light_color_bits[axis] = b->light_bits[axis];
    }
    hd.light_intensity_bits = b->light_bits[3];
    hd.azimuths = b->azimuths;
    hd.cosines = b->cosines;
    hd.margin_texels = b->margin;
    hd.entries = b->entries;
    hd.stored_entries = b->stored;
    hd.active_nodes = b->sparse ? b->active : bake_nodes(*b);
    hd.sample_step_bits = float_bits(h->scene.sample_step);
    hd.mean_free_path_bits = float_bits(h->scene.mean_free_path_m);
    hd.cloud_size_bits = float_bits(h->scene.cloud_size_m);
    hd.estimator = h->scene.estimator;
    hd.tex_fixed8 = (h->scene.flags & CT_FLAG_TEX_FIXED8) ? 1u : 0u;
    if (b->traced) {
        hd.samples = b->samples;
        hd.paths = b->paths;
    }
    if (b->adaptive) {
        hd.round_samples = b->ap.round_samples;
        hd.max_samples = b->cap;
        hd.zero_samples = b->ap.zero_samples;
        hd.rel_tol_bits = float_bits(b->ap.rel_tol);
        hd.abs_tol_bits = float_bits(b->ap.abs_tol);
        hd.rounds = b->rounds;
        hd.capped = b->live;
        hd.converged = b->rounds != 0u ? bake_trace_total(b) - b->live : 0u;
    }
}

static void bake_from_header(CtHandle h, const CtBakeFileHeader &hd, CtBake_ *b)
{
    static_cast<BakeShape &>(*b) = bake_shape(h, hd.grid, hd.azimuths, hd.cosines, hd.kind, hd.traced != 0u);
    b->stored = hd.stored_entries;   // (margin and active: the mask's, once it has been verified)
    b->half = hd.format == (uint32_t)CT_BAKE_F16;
    b->adaptive = hd.adaptive != 0u;
    for (int axis = 0; axis < 3; axis++) {
        b->l[axis] = hd.light[axis];
        b->a[axis] = hd.axis_a[axis];
        b->b[axis] = hd.axis_b[axis];
        b->light_bits[axis] = hd.light_color_bits[axis];
    }
    b->light_bits[3] = hd.light_intensity_bits;
    b->samples = hd.samples;
    b->paths = hd.paths;
    if (b->adaptive) {
        b->ap = CtBakeAdaptive{ CT_ABI_VERSION, hd.round_samples, hd.max_samples, hd.zero_samples, bits_float(hd.rel_tol_bits), bits_float(hd.abs_tol_bits) };
        b->cap = hd.max_samples;
        b->rounds = hd.rounds;
    }
    // current: the file's light, colour and intensity are the handle's, bit for bit
    BakeState now;
    bake_frame(h, &now);
    bool same = std::memcmp(now.light_bits, b->light_bits, sizeof now.light_bits) == 0;
    for (int axis = 0; axis < 3; axis++) {
        same = same && float_bits(now.l[axis]) == float_bits(b->l[axis]);
    }
    b->epoch = same ? h->light_epoch : h->light_epoch - 1u;
}

extern "C" int ct_bake_save(CtBake b, const char *path)
{
    const char *const who = "ct_bake_save";
    if (!b || !path) {
        return fail(b ? b->h : nullptr, CT_E_INVAL, "%s: need a bake and a path", who);
    }
    CtHandle h = b->h;
    NEED(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    CtBakeFileInfo fi{};
    CtBakeFileHeader &hd = fi.header;
    bake_to_header(b, hd);
    int rc = bake_volume_hash(h, &hd.volume_hash);
    if (rc != CT_OK) {
        return rc;
    }
    bakefile_layout(&fi);
    std::vector<uint8_t> bytes;
    try {
        bytes.assign((size_t)fi.file_bytes, 0);
    } catch (const std::bad_alloc &) {
        return fail(h, CT_E_NOMEM, "%s: no host memory for a file of %llu bytes", who, (unsigned long long)fi.file_bytes);
    }
    std::memcpy(bytes.data(), &hd, sizeof hd);
    if (b->sparse) {
        HIPCHK(h, hipMemcpy(bytes.data() + fi.nodes_offset, b->d_nodes, (size_t)bake_nodes(*b), hipMemcpyDeviceToHost));
    }
    if (b->half) {
        HIPCHK(h, hipMemcpy(bytes.data() + fi.table_offset, b->d_half, (size_t)b->stored * 2u, hipMemcpyDeviceToHost));
    } else {
        HIPCHK(h, hipMemcpy(bytes.data() + fi.table_offset, b->d_table, (size_t)b->stored * 4u, hipMemcpyDeviceToHost));
    }
    if (b->adaptive) {
        HIPCHK(h, hipMemcpy(bytes.data() + fi.m2_offset, b->d_m2, (size_t)b->stored * 4u, hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(bytes.data() + fi.counts_offset, b->d_counts, (size_t)b->stored * 4u, hipMemcpyDeviceToHost));
    }
    const uint64_t sum = fnv1a64(bytes.data(), (size_t)fi.checksum_offset);
    std::memcpy(bytes.data() + fi.checksum_offset, &sum, 8);
    // through a temporary name in the same directory, then renamed: no partial file ever stands under `path`
    const std::string tmp = std::string(path) + ".tmp" + std::to_string((long long)getpid());
    FILE *f = std::fopen(tmp.c_str(), "wb");
    if (!f) {
        return fail(h, CT_E_INVAL, "%s: cannot create %s: %s", who, tmp.c_str(), std::strerror(errno));
    }
    const bool written = std::fwrite(bytes.data(), 1, bytes.size(), f) == bytes.size();
    const bool closed = std::fclose(f) == 0;
    if (!written || !closed || std::rename(tmp.c_str(), path) != 0) {
        const int err = errno;
        std::remove(tmp.c_str());
        return fail(h, CT_E_INVAL, "%s: cannot write %s: %s", who, path, std::strerror(err));
    }
    return CT_OK;
}

// A whole file read and checked by the device-free parser.  h: whose error text a failure sets (NULL: the thread's).
static int bake_file_read(CtHandle h, const char *path, const char *who, std::vector<uint8_t> &data, CtBakeFileInfo *fi)
{
    FILE *f = std::fopen(path, "rb");
    if (!f) {
        return fail(h, CT_E_INVAL, "%s: cannot open %s: %s", who, path, std::strerror(errno));
    }
    // (the largest valid file: header, 2^24 node bytes, three sections of 2^26 words)
    const size_t limit = sizeof(CtBakeFileHeader) + (1u << 24) + 3u * ((size_t)4 << 26) + 64u;
    bool ok = true;
    try {
        uint8_t chunk[65536];
        size_t got;
        while ((got = std::fread(chunk, 1, sizeof chunk, f)) != 0u) {
            if (data.size() + got > limit) {
                ok = false;
                break;
            }
            data.insert(data.end(), chunk, chunk + got);
        }
    } catch (const std::bad_alloc &) {
        std::fclose(f);
        return fail(h, CT_E_NOMEM, "%s: no host memory for %s", who, path);
    }
    const bool read_error = std::ferror(f) != 0;
    std::fclose(f);
    if (read_error) {
        return fail(h, CT_E_INVAL, "%s: cannot read %s", who, path);
    }
    if (!ok) {
        return fail(h, CT_E_INVAL, "%s: %s is longer than any bake file", who, path);
    }
    BakeFileError err;
    if (bakefile_parse(data.data(), data.size(), fi, err) != CT_OK) {
        return fail(h, CT_E_INVAL, "%s: %s: %s", who, path, err.text);
    }
    return CT_OK;
}

extern "C" int ct_bake_file_info(const char *path, CtBakeFileInfo *out)
{
    if (!path || !out) {
        return fail(nullptr, CT_E_INVAL, "ct_bake_file_info: need a path and out");
    }
    std::vector<uint8_t> data;
    return bake_file_read(nullptr, path, "ct_bake_file_info", data, out);
}

// ---- ct_bake_load in stages: the file read and parsed (bake_file_read), its cloud compared with the handle's, then the bake
// under construction from the header (bake_from_header), its mask, its memory, its contents and its live list ---------------------
struct BakeFile {
    const char *who;
    const std::vector<uint8_t> &data;
    const CtBakeFileInfo &fi;
};
static const char *const kBakeOther = "a bake of another cloud / estimator";

// The cloud and the estimator the table was made on, as far as the host knows them: nothing of the handle is touched.
static int bake_load_same_scene(CtHandle h, const CtBakeFileHeader &hd, const char *who)
{
    for (int axis = 0; axis < 3; axis++) {
        if (hd.dims[axis] != h->scene.dims[axis]) {
            return fail(h, CT_E_INVAL, "%s: %s: dims[%d] is %u in the file, %u on the handle", who, kBakeOther, axis, hd.dims[axis], h->scene.dims[axis]);
        }
    }
    const struct {
        const char *name;
        uint32_t file, handle;
    } fields[] = {
        { "sample_step", hd.sample_step_bits, float_bits(h->scene.sample_step) },
        { "mean_free_path_m", hd.mean_free_path_bits, float_bits(h->scene.mean_free_path_m) },
        { "cloud_size_m", hd.cloud_size_bits, float_bits(h->scene.cloud_size_m) },
        { "estimator", (uint32_t)hd.estimator, (uint32_t)h->scene.estimator },
        { "CT_FLAG_TEX_FIXED8", hd.tex_fixed8, (h->scene.flags & CT_FLAG_TEX_FIXED8) ? 1u : 0u },
    };
    for (const auto &fd : fields) {
        if (fd.file != fd.handle) {
            return fail(h, CT_E_INVAL, "%s: %s: %s is 0x%08x in the file, 0x%08x on the handle", who, kBakeOther, fd.name, fd.file, fd.handle);
        }
    }
    if (hd.traced && (h->scene.flags & CT_FLAG_SIMPLE_KERNEL)) {
        return fail(h, CT_E_INVAL, "%s: a traced bake's point radiance tasks need the persistent kernel", who);
    }
    return CT_OK;
}

// ... and its texels.  Nothing is in flight.
static int bake_load_same_volume(CtHandle h, const CtBakeFileHeader &hd, const char *who)
{
    uint64_t hash = 0;
    const int rc = bake_volume_hash(h, &hash);
    if (rc != CT_OK) {
        return rc;
    }
    if (hash != hd.volume_hash) {
        return fail(h, CT_E_INVAL, "%s: %s: the volume hash is %016llx in the file, %016llx on the handle", who, kBakeOther,
                    (unsigned long long)hd.volume_hash, (unsigned long long)hash);
    }
    return CT_OK;
}

// The mask again, on this handle: the file's node bytes must be it; list and slots are the recomputation's.
static int bake_load_mask(CtHandle h, CtBake_ *b, const BakeFile &f)
{
    if (!b->sparse) {
        return CT_OK;
    }
    const CtBakeFileHeader &hd = f.fi.header;
    BakeMask m;
    int rc = bake_mask_reserve(h, b->grid, m, b->compact);
    uint32_t active = 0;
    double ms = 0;
    if (rc == CT_OK) {
        rc = bake_mask_run(h, b->grid, m, &active, &ms);
    }
    if (rc != CT_OK) {
        return rc;
    }
    const size_t nodes = (size_t)bake_nodes(*b);
    std::vector<uint8_t> mask(nodes);
    HIPCHK(h, hipMemcpy(mask.data(), m.nodes, nodes, hipMemcpyDeviceToHost));
    if (m.margin != hd.margin_texels || active != hd.active_nodes || std::memcmp(mask.data(), f.data.data() + f.fi.nodes_offset, nodes) != 0) {
        return fail(h, CT_E_INVAL, "%s: the file's node bytes are not this handle's mask of the grid (%llu active nodes, margin %u in the file; "
                                   "%u, margin %u here)", f.who, (unsigned long long)hd.active_nodes, hd.margin_texels, active, m.margin);
    }
    bake_adopt_mask(b, m, active);
    return CT_OK;
}

// Everything else, allocated before the first copy.
static int bake_load_reserve(CtHandle h, CtBake_ *b, const BakeFile &f)
{
    const size_t stored = (size_t)b->stored;
    bool got = b->half ? b->d_half.alloc(stored) == hipSuccess : b->d_table.alloc(stored) == hipSuccess;
    got = got && ((!b->sparse && !b->traced) || b->d_probe.alloc(bake_probe_floats(*b)) == hipSuccess);
    got = got && (!b->traced || b->d_dirs.alloc(bake_dir_floats(*b)) == hipSuccess);
    if (!got) {
        (void)hipGetLastError();
        return fail(h, CT_E_NOMEM, "%s: no device memory for a bake of %llu stored entries", f.who, (unsigned long long)b->stored);
    }
    if (b->adaptive) {
        BakeAdaptiveSet set;
        const int rc = bake_adaptive_reserve(h, b, set, false, f.who);
        if (rc != CT_OK) {
            return rc;
        }
        bake_adaptive_adopt(b, set);
    }
    return CT_OK;
}

// The file's table (and m2 and counts), and a traced bake's tables of its frame.
static int bake_load_upload(CtHandle h, CtBake_ *b, const BakeFile &f)
{
    const size_t stored = (size_t)b->stored;
    const uint8_t *const data = f.data.data();
    return drained(h, [&]() -> int {
        if (b->half) {
            HIPCHK(h, hipMemcpyAsync(b->d_half, data + f.fi.table_offset, stored * 2u, hipMemcpyHostToDevice, h->stream));
        } else {
            HIPCHK(h, hipMemcpyAsync(b->d_table, data + f.fi.table_offset, stored * 4u, hipMemcpyHostToDevice, h->stream));
        }
        if (b->adaptive) {
            HIPCHK(h, hipMemcpyAsync(b->d_m2, data + f.fi.m2_offset, stored * 4u, hipMemcpyHostToDevice, h->stream));
            HIPCHK(h, hipMemcpyAsync(b->d_counts, data + f.fi.counts_offset, stored * 4u, hipMemcpyHostToDevice, h->stream));
        }
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return b->traced ? bake_upload_trace_tables(h, b) : CT_OK;
    });
}

// The live list the bake was left with: the stored entries of active nodes that fail the rule, ascending.  (An entry that
// stopped by the rule passes it; one that fails holds `samples` experiments, or it would have gone on.)  The header's `capped`
// is their number.  The count and compaction kernels read the list and the grid of bake_trace_args, not its two tables.
static int bake_load_live(CtHandle h, CtBake_ *b, const BakeFile &f)
{
    if (!b->adaptive) {
        return CT_OK;
    }
    const uint32_t n = (uint32_t)bake_trace_total(b);   // (<= stored <= 2^26)
    if (b->rounds != 0u && n != 0u) {
        const int rc = drained(h, [&]() -> int {
            const BakeTraceArgs a = bake_trace_args(b);
            const BakeAdaptiveState st{ b->d_table, b->d_m2, b->d_counts, b->ap.rel_tol, b->ap.abs_tol, b->ap.zero_samples };
            uint32_t survivors = 0;
            HIPCHK(h, launch_bake_adaptive_count(a, st, n, b->d_waves, h->stream));
            HIPCHK(h, launch_bake_adaptive_scan(b->d_waves, n, h->stream));
            HIPCHK(h, launch_bake_adaptive_compact(a, st, nullptr, n, b->d_waves, b->d_live[0], h->stream));
            HIPCHK(h, hipMemcpyAsync(&survivors, b->d_waves + (n + 63u) / 64u, sizeof survivors, hipMemcpyDeviceToHost, h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));
            b->live = survivors;
            b->live_cur = 0;
            return CT_OK;
        });
        if (rc != CT_OK) {
            return rc;
        }
    }
    if (b->live != f.fi.header.capped) {
        return fail(h, CT_E_INVAL, "%s: the header counts %llu capped entries, the stored means, m2 and counts leave %llu", f.who,
                    (unsigned long long)f.fi.header.capped, (unsigned long long)b->live);
    }
    return CT_OK;
}

extern "C" int ct_bake_load(CtHandle h, const char *path, CtBake *out)
{
    const char *const who = "ct_bake_load";
    if (!h) {
        return fail(nullptr, CT_E_INVAL, "null handle");
    }
    if (!path || !out) {
        return fail(h, CT_E_INVAL, "%s: need a path and out", who);
    }
    *out = nullptr;
    std::vector<uint8_t> data;
    CtBakeFileInfo fi{};
    int rc = bake_file_read(h, path, who, data, &fi);
    if (rc == CT_OK) {
        rc = bake_load_same_scene(h, fi.header, who);
    }
    if (rc != CT_OK) {
        return rc;
    }
    NEED_NOFLUSH(h);
    rc = flush(h);
    if (rc == CT_OK) {
        rc = bake_load_same_volume(h, fi.header, who);
    }
    if (rc != CT_OK) {
        return rc;
    }
    std::unique_ptr<CtBake_> made(new CtBake_());   // (every return but the last deletes it)
    CtBake_ *const b = made.get();
    bake_from_header(h, fi.header, b);
    const BakeFile file{ who, data, fi };
    for (const auto stage : { bake_load_mask, bake_load_reserve, bake_load_upload, bake_load_live }) {
        rc = stage(h, b, file);
        if (rc != CT_OK) {
            return rc;
        }
    }
    *out = made.release();
    return CT_OK;
}

// ---- a bake on a group (ct_group_bake_*, ct_group.hip): one shard's span, the checks passed through, the exchange: DESIGN 8 f-19 ----
int ct::bake_create_shard(CtHandle h, CtNetwork n, const CtBakeDesc *d, uint32_t kind, const uint32_t *samples, const CtBakeAdaptive *p,
                          uint32_t shard, uint32_t shards, CtBake *out)
{
    return bake_create(h, n, d, out, kind, samples, p, shard, shards);
}

extern "C" int ct_debug_bake_shard(CtHandle h, const CtBakeDesc *d, uint32_t kind, uint32_t samples, const CtBakeAdaptive *p, uint32_t shard,
                                   uint32_t shards, CtBake *out)
{
    if (!h) {
        return fail(nullptr, CT_E_INVAL, "null handle");
    }
    if (!d || !out || shards == 0u || shards > 64u || shard >= shards) {
        return fail(h, CT_E_INVAL, "ct_debug_bake_shard: need a description, out and shard < shards <= 64");
    }
    return bake_create(h, nullptr, d, out, kind, p ? nullptr : &samples, p, shard, shards);
}

int ct::bake_cut_shard(CtBake b, uint32_t shard, uint32_t shards)
{
    CtHandle h = b->h;
    NEED(h);
    return bake_cut(h, b, shard, shards);
}

void ct::bake_shard_span(CtBake b, uint64_t lo_hi_out[2])
{
    bake_span(b, &lo_hi_out[0], &lo_hi_out[1]);
}

int ct::bake_op_checks(CtHandle h, CtNetwork n, CtBake b, BakeOp op, uint32_t arg)
{
    switch (op) {
    case BAKE_OP_UPDATE:
        return bake_update_checks(h, n, b, "ct_bake_update");
    case BAKE_OP_TRACE_MORE:
        return bake_trace_more_checks(h, b, arg, "ct_bake_trace_more");
    case BAKE_OP_RETRACE:
        return bake_trace_checks(h, b, arg, "ct_bake_retrace");
    case BAKE_OP_ADAPTIVE_MORE:
        return bake_adaptive_more_checks(h, b, arg, "ct_bake_trace_adaptive_more");
    default:
        return bake_adaptive_checks(h, b, "ct_bake_retrace_adaptive");
    }
}

// `count` words from src on s's device into dst on d's: on d's stream, which the caller waits for.
static hipError_t bake_exchange_copy(const CtBake_ *d, void *dst, const CtBake_ *s, const void *src, size_t count)
{
    if (count == 0u) {
        return hipSuccess;
    }
    return d->device == s->device ? hipMemcpyAsync(dst, src, count * 4u, hipMemcpyDeviceToDevice, d->h->stream)
                                  : hipMemcpyPeerAsync(dst, d->device, src, s->device, count * 4u, d->h->stream);
}

int ct::bake_exchange(CtBake const *bakes, uint32_t count, uint64_t paths_before, uint64_t *bytes_out, char *error, size_t error_bytes)
{
    auto failed = [&](const char *what, hipError_t e) {
        std::snprintf(error, error_bytes, "the exchange of a group bake: %s failed: %s", what, hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? CT_E_NOMEM : CT_E_HIP;
    };
    const CtBake_ *const b0 = bakes[0];
    BakeState whole = *b0;
    whole.paths = paths_before;
    whole.live = 0;
    for (uint32_t i = 0; i < count; i++) {
        const CtBake_ *s = bakes[i];
        whole.samples = std::max(whole.samples, s->samples);
        whole.rounds = std::max(whole.rounds, s->rounds);
        whole.paths += s->paths - paths_before;
        whole.live += s->live;
        whole.gather_ms = std::max(whole.gather_ms, s->gather_ms);
        whole.network_ms = std::max(whole.network_ms, s->network_ms);
        whole.mask_ms = std::max(whole.mask_ms, s->mask_ms);
        whole.trace_ms = std::max(whole.trace_ms, s->trace_ms);
        whole.fold_ms = std::max(whole.fold_ms, s->fold_ms);
        whole.test_ms = std::max(whole.test_ms, s->test_ms);
    }
    if (whole.live > bake_trace_total(b0)) {   // (what a live list holds)
        std::snprintf(error, error_bytes, "internal: the shards of a group bake leave %llu live entries of %llu",
                      (unsigned long long)whole.live, (unsigned long long)bake_trace_total(b0));
        return CT_E_HIP;
    }
    uint64_t moved = 0;
    for (uint32_t i = 0; i < count; i++) {
        CtBake_ *d = bakes[i];
        hipError_t e = hipSetDevice(d->device);
        if (e != hipSuccess) {
            return failed("hipSetDevice", e);
        }
        (void)hipGetLastError();
        uint64_t at = 0;
        for (uint32_t j = 0; j < count; j++) {
            const CtBake_ *s = bakes[j];
            const size_t first = (size_t)s->range_lo, n = (size_t)(s->range_hi - s->range_lo);
            if (j != i) {
                e = bake_exchange_copy(d, d->d_table + first, s, s->d_table + first, n);
                if (e == hipSuccess && d->adaptive) {
                    e = bake_exchange_copy(d, d->d_m2 + first, s, s->d_m2 + first, n);
                }
                if (e == hipSuccess && d->adaptive) {
                    e = bake_exchange_copy(d, d->d_counts + first, s, s->d_counts + first, n);
                }
                moved += (d->adaptive ? 12u : 4u) * (uint64_t)n + (d->adaptive ? 4u * s->live : 0u);
            }
            if (e == hipSuccess && d->adaptive) {   // (its own survivors too: from the front of one of its lists into the other)
                e = bake_exchange_copy(d, d->d_live[d->live_cur ^ 1] + at, s, s->d_live[s->live_cur], (size_t)s->live);
                at += s->live;
            }
            if (e != hipSuccess) {
                return failed("a copy between shards", e);
            }
        }
    }
    for (uint32_t i = 0; i < count; i++) {   // (no list changes its role before every copy that reads it has landed)
        hipError_t e = hipSetDevice(bakes[i]->device);
        if (e == hipSuccess) {
            e = hipStreamSynchronize(bakes[i]->h->stream);
        }
        if (e != hipSuccess) {
            return failed("hipStreamSynchronize", e);
        }
    }
    for (uint32_t i = 0; i < count; i++) {
        CtBake_ *d = bakes[i];
        BakeState next = whole;   // the frame, its epoch, its light's bits and the cap are the shard's own: the same values
        std::copy_n(d->l, 3, next.l);
        std::copy_n(d->a, 3, next.a);
        std::copy_n(d->b, 3, next.b);
        std::copy_n(d->light_bits, 4, next.light_bits);
        next.epoch = d->epoch;
        next.cap = d->cap;
        next.live_cur = d->adaptive ? d->live_cur ^ 1 : d->live_cur;
        static_cast<BakeState &>(*d) = next;
    }
    *bytes_out = moved;
    return CT_OK;
}
