// ct_internal.hpp -- launcher declarations shared by ct_kernels.hip and the host files (ct_api.cpp, ct_neural.cpp, ct_bake.cpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ct_device.hpp"

namespace ct {

constexpr int kTile = 8;            // pixel tile edge: 8x8 = one wave of primary rays
constexpr int kCounterCount = 9;    // paths, box_hits, density, inscatter, scatter, capped (the algorithm's, = the oracle's);
                                    // then what the kernels ISSUED: density fetches, shadow-volume fetches (ct_fetch_counters),
                                    // and the samples the accumulate kernels found without alpha == 1 (ct_debug_invariants)
constexpr int kStatCount = 82;      // scheduler diagnostics (ct_debug_stats): [0,64) as before, [64,68) path conservation
                                    // (samples dealt, paths resumed, results written, paths suspended; STATS kernels only),
                                    // [73,75) MARCH free-space skips and the burst steps their replays took, per lane,
                                    // [75,82) MARCH schedule mix: scheduler visits, idle lanes summed over them, bursts, and the
                                    // bursts ended by: the step count, too few marching lanes, burst_scatter, the tail rule
constexpr int kContWords = 16;      // words of a suspended path (render_persistent_kernel)
constexpr int kContWordsDelta = 32; // the same for render_delta_kernel (its DDA state rides along)
constexpr int kLeftWords = 8;        // words of a job handed to the next launch (BatchArgs::left_out)
constexpr int kQueueFlag = 32;       // word of the queue array (its own 128-B line) that says "job list empty"
constexpr int kQueueDone = 16;       // ... and the word that counts the queues whose last job has been taken
constexpr int kQueueWords = 64;      // size of a queue array
constexpr int kQueues = 8;          // one job queue per XCD (MI355X: 8 XCDs, each with its own L2)

// One progressive batch: subframes first .. first+S-1 of the handle's own tiles.
struct BatchArgs {
    // per-sample results (frameResultBuffer x S).  Compact form: frames[s * frame_stride + e] for
    // entry e of the pixel list (only this shard's box-hitting pixels exist); dense form
    // (frame_stride == 0): frames[pixel], one full W x H frame, used by ct_render_subframe.
    float4 *frames;
    uint32_t frame_stride;
    const float4 *primary;     // 2 float4 per pixel: cached primary ray (primary_rays_kernel)
    const float4 *advance;     // per pixel: state after the pre-walked prefix of the primary flight: 1 float4
                               // (MARCH, primary_advance_kernel) or 4 (DELTA, primary_advance_delta_kernel);
                               // NULL = start at the entry point
    const uint32_t *pixels;    // this shard's box-hitting pixels, 64 per group, 0xffffffff padded
    const float4 *start;       // image launches of the MARCH kernel: per slot of `pixels` what its samples start from, 2 float4
                               // (start_records_kernel): the regenerate phase then reads neither pixels, primary nor advance.
                               // NULL (point tasks, dense frames, the other kernels): it reads those three
    // A launch may cover only a CHUNK of the pixel groups (all S subframes of each): the scratch then has a column of 64
    // entries per group of the chunk, group g's at (group_rank[g] - rank_base) * 64 -- group_rank = the group's place in the
    // cost-sorted order the job list is built in, of which a chunk is a contiguous piece.  NULL: column g * 64 (every group).
    const uint32_t *group_rank;
    uint32_t rank_base;
    // job list: job j renders subframes [begin, begin+count) of pixel group job_group[j];
    // job_sub[j] = begin | count << 16.  Sorted most expensive group first, and expensive groups
    // are cut into short jobs, so the long paths start early and spread over all waves while
    // every wave still stays on one 64-pixel group at a time (cache locality).
    const uint32_t *job_group;
    const uint32_t *job_sub;
    uint2 *cost;               // the cost-measuring launch of a pose (NULL once the job order is tuned): what every path has
                               // cost (MARCH: fetches + 4 per bounce; DELTA: bounces) and how deep it went, stored where its
                               // result goes -- cost[out_idx - out_offset] -- and summed per pixel group by
                               // launch_cost_reduce.  (Until round 3 two atomics per path on per-group words: 17.6 M
                               // device-scope atomics were 5.7 of the 21 ms of a pose's first 10 subframes.)
    uint32_t n_jobs;
    // Queue x < kQueues holds jobs [q_begin[x], q_begin[x+1]): the pixel groups of one compact image
    // region, so that the waves of one XCD share that region's bricks in their L2.  Queue kQueues
    // is shared: the jobs of the deepest groups, which every wave of the chip must start on at
    // once (a launch cannot be shorter than its deepest path).  A wave drains the shared queue,
    // then the queue of the XCD it runs on, then the following ones (work stealing).
    uint32_t q_begin[kQueues + 2];
    uint32_t reverse;          // 1 = every queue is walked from its end (short launches alternate: the sweep over the image
                               // turns round where the previous launch stopped, whose paths this one resumes)
    uint32_t first_subframe;   // 1-based subframeId of slice 0
    uint32_t S;
    uint32_t *queue;           // kQueueWords words, zero before launch: kQueues + 1 work counters, the flag
    // Path continuation (MARCH estimator, batches enqueued with ct_render_accumulate_async): when the job
    // queue is empty a wave does not run its surviving paths to their end -- a launch would end with a
    // tail of waves that carry a few long paths each, 19 ms of 107 at 256 subframes -- it writes their
    // state (kContWords words each) to cont_out and exits; the next launch resumes them from cont_in
    // before it takes jobs.  A resumed path is never suspended again and writes its result where it
    // always would: out_offset selects the half of the scratch that belongs to its batch.
    const uint32_t *cont_in;        // NULL: nothing to resume
    const uint32_t *cont_in_count;  // entries in cont_in (device memory: written by the previous launch)
    uint32_t *cont_cursor;          // zero before launch
    uint32_t *cont_out;             // NULL: run every path to its end
    uint32_t *cont_out_count;       // zero before launch
    uint32_t cont_capacity;         // entries cont_out can hold
    uint32_t max_age;               // a path that has been suspended this often is run to its end (>= 1 when cont_out is set):
                                    // the host accumulates a batch once max_age further launches have run
    unsigned long long *cont_total; // running total of suspended paths (diagnostic), or NULL
    // Jobs handed on like paths: a wave that learns that the job list is empty while it still has samples of its own job
    // to start (its lanes are busy with long paths) does not hold the launch up until lanes come free -- it writes the
    // rest of the job to left_out (kLeftWords words: group, first subframe of the job, next and end sample, the batch's
    // scratch offset and first subframe id, the age its samples start with) and the next launch's waves take those
    // before the job list.  Same samples, same seeds, same result indices: only the launch that runs them changes.
    const uint32_t *left_in;        // NULL: none
    const uint32_t *left_in_count;
    uint32_t *left_cursor;          // zero before launch
    uint32_t *left_out;             // NULL: every wave finishes its job
    uint32_t *left_out_count;       // zero before launch
    uint32_t left_capacity;
    uint32_t out_offset;            // added to a compact result index (frame_stride != 0)
    unsigned long long *counters; // kCounterCount
    unsigned long long *stats;    // kStatCount
    unsigned long long *timeline; // diagnostics (CT_TIMELINE=1), else NULL: per wave [start, end] on the 100 MHz wall clock
    // diagnostics (ct_debug_track_lines; STATS kernels only), else NULL: one bit per 128-B line of the density array the
    // estimator reads (march bricks / apron bricks / twin bricks) and of the shadow volume's apron bricks, set when a launch
    // fetches from the line -- the kernel's working set, to be held against the 256 MiB of the Infinity Cache
    uint32_t *touched_density, *touched_shadow;
};

struct LaunchShape {
    int blocks;
    int threads;
    bool stats;   // launch the diagnostics build of the kernel (CT_STATS / CT_DEBUG_INVARIANTS at ct_create)
    uint32_t pool_slots = 0;   // exchange kernels (ct_exchange.hpp): slots of the block's path pool in LDS
    uint32_t scatter_waves = 0; // ... and how many of a block's 16 waves only run scatter batches
    bool wide = false;          // MARCH: a brick array of more than 4 GiB (or CT_WIDE_OFFSETS=1): launch the kernels that address
                                // footprints with 64-bit offsets
};

// Evenly split job list (no locality information): point tasks, first launches.
inline void split_queues_evenly(BatchArgs &ba)
{
    for (int x = 0; x <= kQueues; x++) {
        ba.q_begin[x] = (uint32_t)(((uint64_t)ba.n_jobs * (uint32_t)x) / kQueues);
    }
    ba.q_begin[kQueues + 1] = ba.n_jobs; // empty shared queue
}

// Tile -> shard map (also exported as ct_tile_owner).
#ifndef CT_SHARD_SHIFT
#define CT_SHARD_SHIFT 0   // experiment: interleave blocks of 2^k x 2^k tiles instead of single tiles
#endif
__host__ __device__ inline uint32_t tile_owner(uint32_t tx, uint32_t ty, uint32_t shard_count)
{
    return shard_count <= 1 ? 0u : ((tx >> CT_SHARD_SHIFT) + 3u * (ty >> CT_SHARD_SHIFT)) % shard_count;
}

hipError_t launch_build_bricks(const uint8_t *texels, int nx, int ny, int nz, int bias, int gx, int gy, int gz,
                               uint8_t *bricks, hipStream_t stream);
hipError_t launch_build_twin_bricks(const uint8_t *density, const uint8_t *shadow, int nx, int ny, int nz, int bias, int gx, int gy, int gz,
                                    uint8_t *bricks, hipStream_t stream);
hipError_t launch_build_dist(const uint8_t *texels, int nx, int ny, int nz, int bias, int gx, int gy, int gz,
                             uint8_t *dist, uint8_t *scratch, uint8_t *majorant, hipStream_t stream);
hipError_t launch_majorant_cells(const uint8_t *texels, int nx, int ny, int nz, int bias, int cell, const int origin[3], int gx, int gy, int gz,
                                 uint8_t *out, uint8_t *out_codes, hipStream_t stream);
hipError_t launch_brick_meta(const uint8_t *dist, const uint8_t *majorant, int nx, int ny, int nz, int bias, int gx,
                             int gy, int gz, uint8_t *bricks, hipStream_t stream);
hipError_t launch_build_mbricks(const uint8_t *texels, int nx, int ny, int nz, int bias_x, int bias, int gx, int gy,
                                int gz, uint8_t *tmp_a, uint8_t *tmp_b, uint8_t *bricks, hipStream_t stream);
#ifdef CT_EXPERIMENTS
hipError_t launch_mbrick_chunk_class(const uint8_t *bricks, int64_t total_bytes, int64_t chunk_bytes, uint4 *out, hipStream_t stream);
hipError_t launch_mbrick_chunk_quantize(uint8_t *chunk, int64_t chunk_bytes, hipStream_t stream);
#endif
hipError_t launch_mbrick_extent(const uint8_t *bricks, int gx, int gy, int gz, uint32_t *row_x0, uint32_t *row_x1, hipStream_t stream);
hipError_t launch_mbrick_compact(const uint8_t *dense, int gx, int gy, int gz, const uint2 *rows, uint8_t *compact, hipStream_t stream);
hipError_t launch_nee_skip_flags(const uint8_t *shadow, int nx, int ny, int nz, int r, int bias_x, int bias, int gx, int gy,
                                 int gz, uint8_t *tmp_a, uint8_t *tmp_c, uint8_t *bricks, hipStream_t stream);
hipError_t launch_shadow_zero_rows(const uint8_t *shadow, int nx, int ny, int nz, int r, int bias_x, int bias, int gx, int gy, int gz,
                                   uint8_t *tmp_a, uint8_t *tmp_c, uint8_t *bricks, const uint2 *rows, hipStream_t stream);
hipError_t launch_twin_shadow_half(const uint8_t *shadow, int nx, int ny, int nz, int bias, int gx, int gy, int gz, uint8_t *bricks,
                                   hipStream_t stream);
hipError_t launch_coarse_clearance(const uint8_t *dist, int nx, int ny, int nz, int bias, int cshift, int cgx, int cgy, int cgz,
                                   uint8_t *out, hipStream_t stream);
hipError_t launch_render_delta(const DevScene &sc, const BatchArgs &ba, LaunchShape shape, hipStream_t stream);
hipError_t launch_inscatter(const DevScene &sc, uint8_t *out, uint32_t zero_faces, hipStream_t stream);
hipError_t launch_primary_rays(const DevScene &sc, float4 *primary, hipStream_t stream);
hipError_t launch_cost_reduce(const uint2 *cost_plane, uint32_t frame_stride, uint32_t S, uint32_t n_groups_in_chunk,
                              const uint32_t *group_order, uint32_t rank_base, uint32_t *cost_sum, uint32_t *cost_deepest,
                              hipStream_t stream);
hipError_t launch_hit_flags(const float4 *primary, const float4 *advance, uint8_t *flags, uint32_t pixels, uint32_t width,
                            uint32_t shard_index, uint32_t shard_count, unsigned long long *through_steps, hipStream_t stream);
hipError_t launch_primary_advance(const DevScene &sc, const float4 *primary, float4 *advance, bool classify, hipStream_t stream);
hipError_t launch_start_records(const DevScene &sc, const uint32_t *pixels, uint32_t slots, const float4 *primary,
                                const float4 *advance, float4 *start, hipStream_t stream);
hipError_t launch_primary_advance_delta(const DevScene &sc, const float4 *primary, float4 *advance, hipStream_t stream);
// Zeroes up to six short word arrays in ONE dispatch (the counters a launch of the estimator starts from: five memsets
// of a few words each were five dispatches of 5 us in front of every 10-subframe launch).
struct ZeroList {
    uint32_t *ptr[6];
    uint32_t words[6];
    int n = 0;
    void add(uint32_t *p, uint32_t w) { ptr[n] = p; words[n] = w; n += 1; }
};
hipError_t launch_zero_words(const ZeroList &z, hipStream_t stream);
hipError_t launch_fill_frame(float4 *frame, uint32_t width, uint32_t height, uint32_t shard_index,
                             uint32_t shard_count, hipStream_t stream);
hipError_t launch_render_persistent(const DevScene &sc, const BatchArgs &ba, LaunchShape shape, hipStream_t stream);
hipError_t launch_render_simple(const DevScene &sc, const BatchArgs &ba, uint32_t shard_index,
                                uint32_t shard_count, hipStream_t stream);
hipError_t launch_accumulate_batch(const float4 *frames, float4 *mean, float4 *m2, uint32_t first_subframe,
                                   uint32_t S, uint32_t width, uint32_t height, uint32_t shard_index,
                                   uint32_t shard_count, unsigned long long *bad_samples, const uint32_t *frozen,
                                   hipStream_t stream);
hipError_t launch_accumulate_list(const float4 *frames, uint32_t frame_stride, const uint32_t *pixels,
                                  uint32_t n_entries, const uint32_t *group_order, uint32_t rank_base, bool with_misses,
                                  const uint8_t *pixel_class, float4 *mean, float4 *m2,
                                  uint32_t first_subframe, uint32_t S, uint32_t width, uint32_t height,
                                  uint32_t shard_index, uint32_t shard_count, unsigned long long *bad_samples,
                                  const uint32_t *frozen, hipStream_t stream);
hipError_t launch_reinhard(const float4 *mean, uint32_t width, uint32_t height, float exposure,
                           float *column_sums, float *avg, uchar4 *screen, uint32_t *generation, int device, hipStream_t stream);
hipError_t launch_converged(const float4 *mean, const float4 *m2, uint32_t subframe_id, uint64_t pixels,
                            unsigned long long *unconverged, hipStream_t stream);
hipError_t launch_converged_freeze(const float4 *mean, const float4 *m2, uint32_t subframe_id, uint64_t pixels,
                                   uint32_t limit, uint32_t *state, hipStream_t stream);
hipError_t launch_cdf_selftest(const float *cdf, const uint16_t *guide, uint32_t first_u24, uint32_t count,
                               uint32_t *k_out, hipStream_t stream);
hipError_t launch_math_selftest(int which, uint32_t lo_bits, uint32_t hi_bits, unsigned long long *out, hipStream_t stream);
hipError_t launch_math_eval(int fn, const uint32_t *in, uint32_t n, uint32_t *out, hipStream_t stream);
hipError_t launch_fetch_probe(const uint8_t *buf, uint32_t log2_lines, uint32_t second_offset,
                              unsigned long long *sum, hipStream_t stream);
hipError_t launch_fetch_probe_ws(const uint8_t *buf, uint32_t log2_threads, uint32_t ws_lines, uint32_t salt, unsigned long long *sum,
                                 hipStream_t stream);
hipError_t launch_point_rays(const DevScene &sc, const void *tasks, uint32_t n, uint32_t n_pad, float4 *primary,
                             uint32_t *pixels, hipStream_t stream);
hipError_t launch_point_accumulate(const float4 *frames, uint32_t stride, void *tasks, uint32_t n, uint32_t launches,
                                   hipStream_t stream);
hipError_t launch_scatter_samples(const DevScene &sc, uint32_t count, uint32_t batch_seed, float *positions,
                                  float *directions, hipStream_t stream);
// The pixels a pass of the first-scatter / network path works on, one per lane: a rect of the frame in row-major order, or a run
// of 8x8 tiles of a shard's tile list, one wave per tile, lane l of a tile its pixel (l & 7, l >> 3).  A lane of a tile that the
// frame clips has no pixel.
struct PixelBand {
    uint32_t x0, y0, w;      // rect: origin and row length
    uint32_t n;              // lanes: the rect's pixels, or 64 per tile
    const uint32_t *tiles;   // tile run (device, n / 64 entries, ty * tiles_x + tx each); NULL: a rect
    uint32_t tiles_x, width, height;   // tile run: the frame's
};
inline PixelBand rect_band(uint32_t x0, uint32_t y0, uint32_t w, uint32_t rows)
{
    return { x0, y0, w, w * rows, nullptr, 0u, 0u, 0u };
}
inline PixelBand tile_band(const DevScene &sc, const uint32_t *tiles, uint32_t count)
{
    return { 0u, 0u, 0u, 64u * count, tiles, sc.tiles_x, sc.width, sc.height };
}
// The flight's temporaries, indexed by lane: found and direct hold (n rounded up to 256) float4, waves (n rounded up to 256) / 64 + 1
// words -- the waves' record counts, after the scan their offsets and, in the last word, the number of records.
struct FlightTemps {
    float4 *found;
    uint32_t *waves;
    float4 *direct;   // the single-scatter term of a lane's collision (CT_NET_ADD_SINGLE_SCATTER), zeros without a record; NULL: not made
};
// ct_descriptor_frame: the band's first flights, a scan of the per-wave counts and the compacting write, three dispatches.
// positions / directions hold `capacity` records, pixels may be NULL.
hipError_t launch_first_scatter_frame(const DevScene &sc, const PixelBand &band, const FlightTemps &t, uint32_t subframe_id,
                                      uint32_t capacity, float *positions, float *directions, uint32_t *pixels, hipStream_t stream);
// ... and its first dispatch alone (ct_baked_render_*): found, direct and the waves' counts, neither scanned nor compacted.
hipError_t launch_first_flights(const DevScene &sc, const PixelBand &band, const FlightTemps &t, uint32_t subframe_id, hipStream_t stream);
// ct_network_render_*: aux[i] = dot(directions[i], l), left to right; and the band's pixels from the flight's temporaries and the
// network's outputs of the band's records.
struct NetCompose {
    int32_t transform;   // CT_NET_OUT_* (the low byte of CtNetworkRender::transform)
    float sr, sg, sb;    // rgb_scale
};
struct ComposeTarget {       // a rect: at the band's first pixel; a tile run: the whole frame's
    float4 *frame;           // the pixels are stored here; NULL: they go into the Welford update of
    float4 *mean, *m2;       // ... these, with n = subframe_id, unless *frozen
    uint32_t subframe_id;
};
hipError_t launch_network_aux(const float *directions, uint32_t count, float lx, float ly, float lz, float *aux, hipStream_t stream);
hipError_t launch_network_compose(const PixelBand &band, const FlightTemps &t, const NetCompose &c, const float *out,
                                  const ComposeTarget &dst, const uint32_t *frozen, hipStream_t stream);
// ct_network_bake: the probe table as the lookup sees it (include/cloudtrace.h, "the network baked into a probe table").
struct BakeTable {
    const float *table;              // [z][y][x][azimuth][cosine]
    uint32_t nx, ny, nz, nphi, nc;
    float lx, ly, lz;                // the light travel direction the table was baked for
    float ax, ay, az, bx, by, bz;    // the azimuth frame
    const uint32_t *slots;           // ct_network_bake_compact: the block of node (z Ny + y) Nx + x in the table; nullptr: dense addressing
    const uint16_t *half;            // ct_bake_half: the table as binary16 in the same order (`table` is nullptr then); nullptr: float32
};
// The bake's own kernels: aux[i] = value; table[i * stride + k] = out[i]; and (ct_debug_bake_lookup) the lookup of caller-supplied
// records.  launch_baked_compose forms a band's pixels as launch_network_compose does (the kernels share everything behind a
// record's output), with the output looked up in the table.
hipError_t launch_bake_fill(float *aux, uint32_t count, float value, hipStream_t stream);
hipError_t launch_bake_store(const float *out, uint32_t count, float *table, uint32_t stride, uint32_t k, hipStream_t stream);
hipError_t launch_bake_lookup(const DevScene &sc, const BakeTable &t, const float *positions, const float *directions, uint32_t count,
                              float *out, hipStream_t stream);
// ct_network_bake_sparse: the mask of a probe grid (include/cloudtrace.h, "the sparse bake").  Everything is the caller's,
// allocated: ranges = the texel range lo | hi << 16 of every cell of x, then y, then z; tmp_x = slab * dims[1] * (grid[0] - 1)
// bytes and tmp_xy = slab * (grid[1] - 1) * (grid[0] - 1), the z planes the reduction takes at a time; cells, x fastest; nodes;
// waves = (nodes rounded up to 256) / 64 + 1 counts, the last of which becomes the number of active nodes; list = room for every
// node, filled with the active ones in ascending order; slots (ct_network_bake_compact) = nullptr, or one word per node: 1 + the
// node's place in the list, 0 for an inactive node.
struct BakeMaskArgs {
    const uint8_t *density;
    uint32_t dims[3], grid[3], slab;
    const uint32_t *ranges;
    uint8_t *tmp_x, *tmp_xy, *cells, *nodes;
    uint32_t *waves, *list, *slots;
};
hipError_t launch_bake_mask(const BakeMaskArgs &a, hipStream_t stream);
// The bake's chunk from the list: records [first, first + count) of the compacted probes (node list[p / nphi], azimuth p % nphi)
// from the host's tables (axes: the position nodes of x, y, z; directions: nphi x 3), and launch_bake_store through the list
// into the whole table.
hipError_t launch_bake_records(const uint32_t *list, uint64_t first, uint32_t count, uint32_t nx, uint32_t ny, uint32_t nphi,
                               const float *axes, const float *directions, float *pos, float *dir, hipStream_t stream);
hipError_t launch_bake_store_list(const float *out, const uint32_t *list, uint64_t first, uint32_t count, uint32_t nphi, float *table,
                                  uint32_t stride, uint32_t k, hipStream_t stream);
hipError_t launch_baked_compose(const DevScene &sc, const PixelBand &band, const FlightTemps &t, const BakeTable &table, const NetCompose &c,
                                const ComposeTarget &dst, const uint32_t *frozen, hipStream_t stream);
// ct_baked_render_hybrid_*: launch_first_flights followed through the path tracer's first `depth` collisions -- found[i].w = 0
// none, 1 alive at collision `depth`, 2 ended before it; t.direct = the NEE sum so far (NULL: depth 1 without the single-scatter
// term); omega (as large as found) = the direction the path reached its collision along; t.waves is not used -- and
// launch_baked_compose with that direction and the ended state.
hipError_t launch_hybrid_flights(const DevScene &sc, const PixelBand &band, const FlightTemps &t, float4 *omega, uint32_t subframe_id,
                                 uint32_t depth, hipStream_t stream);
hipError_t launch_hybrid_compose(const DevScene &sc, const PixelBand &band, const FlightTemps &t, const float4 *omega, const BakeTable &table,
                                 const NetCompose &c, const ComposeTarget &dst, const uint32_t *frozen, hipStream_t stream);
// Bake files and half tables (ct_bake_file.hip).  launch_volume_hash: *hash (zeroed by the caller) += the volume hash of
// include/cloudtrace.h, "bake files", over `count` texels, in whatever order the waves run.  launch_bake_half_convert: half[i] =
// half_round_bits(table[i]) for i < count, one lane per value; refused[0] (zeroed) counts the values ct_bake_half refuses and
// refused[1] (0xffffffff) becomes the smallest index of one.
hipError_t launch_volume_hash(const uint8_t *texels, uint64_t count, unsigned long long *hash, hipStream_t stream);
hipError_t launch_bake_half_convert(const float *table, uint32_t count, uint16_t *half, uint32_t *refused, hipStream_t stream);
// ct_bake_traced (ct_bake_trace.hip): the stored entries [first, first + n) of a bake as point tasks and their fold.  list:
// nullptr for a dense bake (stored entry = virtual entry), otherwise the active nodes, whose blocks the stored entries count
// through.  axes: the position nodes of x, y, z; directions: nphi x nc x 3.  launch_bake_trace_tasks writes primary[2 i],
// primary[2 i + 1] and pixels[i] for i < n_pad (a multiple of 64, >= n) as launch_point_rays does, with the seed base of the
// entry's virtual index; launch_bake_trace_fold folds frames[f * stride + i].x, f < passes, into the entry's float of `table`
// (the stored table: compact = behind its zero block), which holds the mean of `done` experiments.
struct BakeTraceArgs {
    const uint32_t *list;
    const float *axes, *directions;
    uint32_t nx, ny, nphi, nc;
    uint64_t first;
    uint32_t n, n_pad, compact;
    const uint32_t *live;   // ct_bake_traced_adaptive: lane i is stored entry live[first + i]; nullptr: first + i
};
hipError_t launch_bake_trace_tasks(const DevScene &sc, const BakeTraceArgs &a, float4 *primary, uint32_t *pixels, hipStream_t stream);
hipError_t launch_bake_trace_fold(const BakeTraceArgs &a, const float4 *frames, uint32_t stride, uint32_t passes, uint32_t done,
                                  float *table, hipStream_t stream);
// ct_bake_traced_adaptive: the state of an entry -- mean (the table), m2 and count at the entry's stored address -- and the
// stopping rule of include/cloudtrace.h, "the adaptive traced bake".  launch_bake_adaptive_fold folds a pass as
// point_accumulate_kernel does, mean and m2, and stores count = done + passes; with `waves` (the round's last pass; a.first is a
// multiple of 64 then) it also tests the rule and wave (a.first + i) / 64 of the live list writes how many of its lanes go on.
// launch_bake_adaptive_compact: the scan of the n_live / 64 (rounded up) wave counts, the number of survivors behind them, and
// the stored indices of the survivors of live_in (nullptr: 0 .. n_live - 1) into live_out, in live_in's order.
struct BakeAdaptiveState {
    float *table, *m2;
    uint32_t *counts;
    float rel_tol, abs_tol;
    uint32_t zero_samples;
};
hipError_t launch_bake_adaptive_fold(const BakeTraceArgs &a, const float4 *frames, uint32_t stride, uint32_t passes, uint32_t done,
                                     const BakeAdaptiveState &st, uint32_t *waves, hipStream_t stream);
// ct_bake_load: the count pass alone over the stored entries [0, n) of active nodes (a.first == 0, a.live == nullptr): waves[w] =
// the lanes of wave w whose stored state fails the rule.  Scan and compact follow as behind a round.
hipError_t launch_bake_adaptive_count(const BakeTraceArgs &a, const BakeAdaptiveState &st, uint32_t n, uint32_t *waves, hipStream_t stream);
hipError_t launch_bake_adaptive_scan(uint32_t *waves, uint32_t n_live, hipStream_t stream);
hipError_t launch_bake_adaptive_compact(const BakeTraceArgs &a, const BakeAdaptiveState &st, const uint32_t *live_in, uint32_t n_live,
                                        const uint32_t *waves, uint32_t *live_out, hipStream_t stream);
// A bake on a group (ct_group_bake_*): a shard's span of an adaptive bake's live list.  launch_bake_live_iota: live[i] = first + i
// for i < n, the list of its first round.  launch_bake_live_bounds: bounds[0] and bounds[1] = how many entries of the ascending
// live[0 .. n) lie below key_lo and below key_hi -- the span's sub-range of a merged or loaded list.
hipError_t launch_bake_live_iota(uint32_t *live, uint32_t first, uint32_t n, hipStream_t stream);
hipError_t launch_bake_live_bounds(const uint32_t *live, uint32_t n, uint32_t key_lo, uint32_t key_hi, uint32_t *bounds, hipStream_t stream);
// ct_collector_* (ct_collect.hip): an update of the device collector of include/cloudtrace.h, "the radiance collector on the
// device".  live: the n live task ids, ascending; r = T / n replicas per task, thread i = t * r + j replica j of live[t].
// positions / directions / mean / m2 / counts / converged_update are indexed by task id.  launch_collect_rays writes
// primary[2 i], primary[2 i + 1] and pixels[i] for i < n_pad (a multiple of 64, >= n * r) as launch_point_rays does for a task
// array with those replicas.  launch_collect_fold folds frames[f * stride + i].x, f < launches, per replica (replica 0 from the
// stored state, which holds `done` experiments; the others from zero), merges replicas 1 .. r - 1 into replica 0 in that order
// with PointRadianceTask::operator+=, stores the triple, tests the rule, stores `update` into converged_update of a task that
// passes, and writes waves[g] = the survivors of group g: a group is one task (r > 1: one wave per task) or 64 consecutive
// tasks of the list (r == 1: one lane per task).  launch_collect_compact: the scan of those counts, the number of survivors
// behind them in waves[groups], and the survivors' ids into live_out in live's order.
struct CollectArgs {
    const uint32_t *live;
    const float *positions, *directions;
    float *mean, *m2;
    uint32_t *counts, *converged_update;
    uint32_t n, r, n_pad;
    float rel_tol, abs_tol;
    uint32_t zero_samples;
};
inline uint32_t collect_groups(const CollectArgs &a)
{
    return a.r > 1u ? a.n : (a.n + 63u) / 64u;
}
hipError_t launch_collect_rays(const DevScene &sc, const CollectArgs &a, float4 *primary, uint32_t *pixels, hipStream_t stream);
hipError_t launch_collect_fold(const CollectArgs &a, const float4 *frames, uint32_t stride, uint32_t launches, uint32_t done,
                               uint32_t update, uint32_t *waves, hipStream_t stream);
hipError_t launch_collect_compact(const CollectArgs &a, uint32_t *waves, uint32_t *live_out, hipStream_t stream);
// ct_adaptive_frame_* (ct_adaptive.hip): a round of the adaptive frame of include/cloudtrace.h, "the adaptive frame".  A chunk is
// the entries [first, first + n) of the live list: pixels live[first + i] (y * width + x, ascending), or first + i while the list
// is the whole frame (live == nullptr).  mean / m2 / counts are indexed by pixel.  launch_adaptive_rays writes primary[2 i],
// primary[2 i + 1] and pixels[i] for i < n_pad (a multiple of 64, >= n) as launch_primary_rays forms the pixel's ray, with the
// entry as the estimator's pixel.  launch_adaptive_fold folds frames[f * stride + i], f < passes, as subframes done + 1 .. onto
// the pixel's mean and m2 with welford() and stores count = done + passes; with `waves` (the round's last pass; first is a
// multiple of 64 then) wave (first + i) / 64 of the list also writes how many of its lanes go on: count < min_samples, or the
// rule fails.  launch_adaptive_compact (first == 0, n == the list's length): the scan of the n / 64 (rounded up) wave counts, the
// number of survivors behind them, and the survivors' pixels into live_out in the list's order.
struct AdaptiveArgs {
    const uint32_t *live;
    uint32_t first, n, n_pad;
    float4 *mean, *m2;
    uint32_t *counts;
    float rel_tol, abs_tol;
    uint32_t min_samples;
};
hipError_t launch_adaptive_rays(const DevScene &sc, const AdaptiveArgs &a, float4 *primary, uint32_t *pixels, hipStream_t stream);
hipError_t launch_adaptive_fold(const AdaptiveArgs &a, const float4 *frames, uint32_t stride, uint32_t passes, uint32_t done,
                                uint32_t *waves, hipStream_t stream);
hipError_t launch_adaptive_compact(const AdaptiveArgs &a, uint32_t *waves, uint32_t *live_out, hipStream_t stream);
// ct_adaptive_frame_create_shard: the first live list of a shard frame, the pixels p = y * width + x < pixels whose 8 x 8 tile is
// the shard's (tile_owner), ascending.  launch_adaptive_own_count: waves[w], w < pixels / 64 (rounded up), becomes the number of
// own pixels before wave w of 64 consecutive pixels and waves[that wave count] their total (the count pass, then the round's
// scan); launch_adaptive_own_list writes the list behind it -- the host reads the total in between and sizes live_out by it.
struct AdaptiveShard {
    uint32_t width, pixels, shard_index, shard_count;
};
hipError_t launch_adaptive_own_count(const AdaptiveShard &s, uint32_t *waves, hipStream_t stream);
hipError_t launch_adaptive_own_list(const AdaptiveShard &s, const uint32_t *waves, uint32_t *live_out, hipStream_t stream);
// Density pyramid (Resources::generateMipmaps) and the descriptor gather.
constexpr int kMaxMipLevels = 16;
struct MipPyramid {
    const uint8_t *base;               // all levels, level l at base + offset[l], [Z][Y][X]
    uint32_t levels;
    uint32_t offset[kMaxMipLevels];
    int32_t nx[kMaxMipLevels], ny[kMaxMipLevels], nz[kMaxMipLevels];
};
hipError_t launch_mip_level(const uint8_t *prev, int px, int py, int pz, uint8_t *cur, int cx, int cy, int cz,
                            hipStream_t stream);
hipError_t launch_descriptors(const DevScene &sc, const MipPyramid &mp, const float *positions, const float *directions,
                              uint32_t count, float level0, float voxel_m, float cloud_size_m, uint8_t *out,
                              hipStream_t stream);
LaunchShape persistent_shape(int device, bool delta, int blocks_per_cu = 0);   // blocks_per_cu: 0 = as many as fit
#ifdef CT_EXPERIMENTS
// The estimators with a block-wide exchange of paths between waves (ct_exchange.hpp): one 1024-thread block per CU.
LaunchShape exchange_shape(int device);
hipError_t launch_render_delta_x(const DevScene &sc, const BatchArgs &ba, LaunchShape shape, hipStream_t stream);
LaunchShape wave_exchange_shape(int device);   // the exchange within a wave (render_delta_w_kernel): pool_slots = slots per wave
hipError_t launch_render_delta_w(const DevScene &sc, const BatchArgs &ba, LaunchShape shape, hipStream_t stream);
#endif

} // namespace ct
