// ct_handle.hpp -- the handle behind CtHandle and what the host translation units that work on it share (ct_api.cpp: lifetime,
// scheduler, buffers and diagnostics; ct_neural.cpp: descriptors, the scattering network and its renderer; ct_bake.cpp: the bakes).  Private: not installed, and
// ct_group.hip keeps to the C ABI.
#pragma once

#include <algorithm>
#include <array>
#include <cstdlib>
#include <functional>
#include <string>
#include <utility>
#include <vector>

#include "../../include/cloudtrace.h"
#include "ct_devmem.hpp"
#include "ct_internal.hpp"

using namespace ct;

// ---- tuning knobs ----------------------------------------------------------------------------------------------------------
// Every environment variable the library reads, copied ONCE per ct_create into the handle (DESIGN.md 4.4 lists them with
// what they do and what was measured).  Knobs choose schedules, scratch sizes, layouts and diagnostics; none changes a
// result (tests/test_gpu_parity.py: the knob test).  get() returns the variable's text as it was at ct_create, or NULL.
struct Knob {
    bool is_set = false;
    std::string text;
    const char *get() const { return is_set ? text.c_str() : nullptr; }
    explicit operator bool() const { return is_set; }
};
#define CT_KNOBS(X) X(BAKE_MASK_BYTES) X(BAKE_TRACE_RESULTS) X(BURST_IDLE) X(BURST_MARCH_MIN) X(BURST_SCATTER) X(CHUNK_INTERLEAVE) X(CHUNK_MORTON) X(CONTINUATION) X(DEBUG_INVARIANTS) X(DELTA_INTERIOR) X(DELTA_NEE) X(EXCHANGE) X(HAND_ON_JOBS) X(HINT_PERIOD) X(JOB_MAX) X(JOB_WORK) X(MARCH_BURST) X(MAX_AGE) X(NEE_CACHE) X(NET_DESC_RECORDS) X(NO_ADVANCE) X(POINT_BLOCKS_PER_CU) X(POINT_ORDER) X(REGEN_MIN) X(RENDER_AHEAD) X(SCATTER_MIN) X(SCATTER_RATIO) X(SCRATCH_GIB) X(SCRATCH_MIB) X(SERPENTINE) X(SHARED_DEPTH) X(SPARSE) X(STATS) X(TAIL_BURST) X(TILE_ORDER) X(TIMELINE) X(TRACE) X(TUNE_SUBFRAMES) X(XCD_QUEUES) X(XCD_QUEUES_UNTUNED) X(XCD_REGIONS) X(BLOCKS_PER_CU) X(WIDE_OFFSETS) X(START_RECORDS) X(THROUGH_PIXELS)
struct CtTuning {
#define X(name) Knob name;
    CT_KNOBS(X)
#undef X
    static CtTuning from_env()
    {
        CtTuning t;
#define X(name)                                  \
    if (const char *e = getenv("CT_" #name)) {   \
        t.name.is_set = true;                    \
        t.name.text = e;                         \
    }
        CT_KNOBS(X)
#undef X
        return t;
    }
};

// One way to read an integer knob: atoi's reading (text that is not a number reads as 0), clamped to [lo, hi]; dflt when unset.
inline int knob_int(const Knob &k, int lo, int hi, int dflt)
{
    return k ? std::min(hi, std::max(lo, atoi(k.get()))) : dflt;
}

// ... and an on/off knob: on for any non-zero number.
inline bool knob_flag(const Knob &k, bool dflt)
{
    return k ? atoi(k.get()) != 0 : dflt;
}

struct CtHandle_ {
    CtTuning tune;         // the environment's knobs as they were at ct_create
    CtScene scene{};       // as given (host pointers are NOT retained)
    int device = 0;
    hipStream_t own_stream = nullptr;   // (release() destroys it after the delete: the buffers below are freed first)
    hipStream_t stream = nullptr;
    Event ev[3];

    DevScene dev{};
    bool camera_set = false;

    // device memory: every buffer is a member that owns it (ct_devmem.hpp), so deleting the handle frees them all
    DevBuf<uint8_t> d_density, d_inscatter, d_dist, d_dist_tmp, d_majorant, d_maj_cells, d_maj_codes;
    DevBuf<uint8_t> d_dbricks, d_ibricks, d_mbricks, d_tbricks;
    DevBuf<uint2> d_mrows;             // sparse march bricks: extent of every brick row (DevScene::m_rows)
    DevBuf<uint8_t> d_mcoarse;         // ... and the clearance of the coarse cells outside the extents
    size_t mbricks_dense_bytes = 0, mbricks_bytes = 0;
    int nee_skip_r = 0;   // radius of the march bricks' shadow-zero flags (0: none set)
    // kept from ct_create for ct_set_light, which has neither the density nor the Mie tables on the host any more
    uint32_t zero_faces = 0;   // empty boundary layers of the density (zero_faces(); launch_inscatter)
    bool mie_finite = true;    // both phase tables are finite (nee_skip_radius)
    // CT_FLAG_VMM_BRICKS: d_mbricks holds a reserved virtual range (not a hipMalloc: release() detaches it), backed chunk by chunk
    struct VmmBricks {
        void *va = nullptr;
        size_t size = 0, chunk = 0;
        std::vector<hipMemGenericAllocationHandle_t> handles;   // one per chunk with memory of its own + the shared ones
        size_t real_chunks = 0, shared_chunks = 0, mapped_chunks = 0;
    } vmm;
    DevBuf<uint8_t> d_pyramid;        // density mip pyramid, built on first use (ct_collect_descriptors)
    MipPyramid pyramid{};
    DevBuf<float> d_mie, d_chopped, d_cdf;
    DevBuf<uint16_t> d_guide;
    DevBuf<float4> d_frame, d_mean, d_m2;
    DevBuf<uchar4> d_screen;
    // Batches enqueued with ct_render_accumulate_async form a pipeline on the handle's stream (M = max_age):
    //     R1  R2 .. R(1+M) A1  R(2+M) A2  ...  (flush:) Rf A(n-M+1) .. An
    // The estimator launch R(k) does not run its surviving paths to their end when its job list is empty: it suspends
    // them (BatchArgs::cont_out) and R(k+1) resumes them first, so no launch ends with a tail of waves that carry a few
    // long paths each.  A path may be suspended M times, so batch k is complete once R(k+M) has run, and A(k), its
    // accumulate kernel, follows that launch (or the flush launch Rf, which only resumes and runs everything to its end).
    // The per-sample scratch is a ring of n_regions = M + 1 regions ([S][stride] compact, or [S][H][W] for the simple
    // kernel): batch k writes region k mod n_regions, which A(k - n_regions) has long left.  M = 1 (two regions) is
    // round 2's scheme and what long batches use -- a launch of 20 ms outlasts the longest path (2000 bounces, ~10 ms);
    // short batches (the reference renders 10 subframes per display update, Camera.cpp:189) get more regions, so that a
    // launch never has to wait for a path that an earlier one handed to it.
    // A slot owns a region, its queue counters and its events; the suspended paths alternate between two buffers.
    static constexpr int kMaxRegions = 64;
    struct Slot {
        DevBuf<uint32_t> queue;
        Event ev_in, ev_start, ev_done, ev_acc0, ev_acc1;
        bool pending = false;              // launched, kernel times not booked yet
        bool accumulated = false;          // its accumulate kernel has been enqueued (ev_acc0/1 valid)
        bool awaits_accumulate = false;    // in `waiting`: some of its subframes are still to be accumulated
        bool complete = false;             // no path of the batch is in flight any more (max_age launches have followed, or a flush)
        uint32_t acc_done = 0;             // subframes of the batch whose accumulate kernels are enqueued
        uint32_t first = 0, S = 0;
        uint32_t rank_base = 0, groups = 0;   // the chunk of pixel groups this launch renders (places in the job order)
        bool with_misses = false;          // its accumulate kernel also accounts for the pixels that miss the box (once per batch)
        bool last_chunk = true;            // ... and is the last of its batch: the running mean is a whole image again after it
    };
    Slot slots[kMaxRegions];
    int n_regions = 2;                     // regions of the scratch in use
    int next_slot = 0;
    std::vector<int> waiting;              // slots with subframes still to be accumulated, oldest first
    // Render-ahead (ct_set_render_ahead, CT_RENDER_AHEAD): enqueued calls of fewer subframes than `ahead` -- the reference's
    // display loop asks for 10 at a time, Camera.cpp:189 -- are served by estimator launches of `ahead` subframes, of which
    // every call accumulates its own share: R(k) a(k-M,0) a(k-M,1) .. R(k+1) a(k-M+1,0) ..  A launch of 10 subframes is
    // mostly beginning and end -- every lane resumes a path and suspends one -- which a launch of `ahead` amortises (DESIGN.md
    // 4.3 item 13).  `rendered` >= `subframes`: the subframes the estimator has been launched for / the caller has asked
    // for; the running mean follows the calls by M * ahead subframes until something waits (flush: exactly `subframes`).
    uint32_t ahead = 0;
    uint32_t rendered = 0;
    // Stop-when-converged (ct_set_stop_when_converged): behind the accumulate kernel of every `stop_cadence`-th subframe (from
    // `stop_min` on) the convergence test runs on the device, and once it holds the accumulate kernels leave the running
    // mean alone -- Camera::render's `if (!isConverged())` (Camera.cpp:179) without a host round trip per update.
    // d_freeze: converged_freeze_kernel's state words; freeze_host: their first four, copied back after every test (pinned).
    uint32_t stop_cadence = 0, stop_min = 100;
    DevBuf<uint32_t> d_freeze;
    HostBuf<uint32_t> freeze_host;
    DevBuf<uint32_t> cont[2];                 // suspended paths: launch k writes cont[k & 1], launch k+1 reads it
    uint64_t launch_no = 0;                // estimator launches enqueued so far
    bool cont_live = false;                // the last launch may have suspended paths: the next one resumes them
    DevBuf<float4> d_frames_all;           // the whole per-sample scratch
    size_t slot_capacity = 0;              // float4 per region
    uint64_t scratch_cap_bytes = 0;        // 0 = CT_SCRATCH_GIB / the default; else what an out-of-memory allocation left us with
    uint32_t layout_S = 0;                 // batch size the regions were laid out for
    DevBuf<uint32_t> left[2];                 // job remainders handed on the same way (BatchArgs::left_out)
    size_t left_capacity = 0;              // entries per buffer: one per wave
    DevBuf<uint32_t> d_cont_count;         // [0,1] entries in cont[i], [2] resume cursor, [3,4] entries in left[i], [5] its cursor
    DevBuf<unsigned long long> d_cont_total;    // paths handed from one launch to the next so far (ct_debug_suspended)
    size_t cont_capacity = 0;              // entries per buffer
    Event ev_flush0, ev_flush1;
    bool continuation = true;              // CT_CONTINUATION=0: async batches run every path to its end
    int max_age_override = 0;              // CT_MAX_AGE=n: n + 1 regions whatever the batch size (0 = by batch duration)
    bool hand_on_jobs = true;              // CT_HAND_ON_JOBS=0: a wave finishes its own job before it suspends (A/B)
    bool serpentine = false;               // CT_SERPENTINE=1: short launches walk their job queues alternately forwards and backwards
    // work queue of the persistent kernel (rebuilt when the camera moves)
    DevBuf<float4> d_primary;         // cached primary rays, 2 float4 per pixel
    DevBuf<float4> d_advance;         // per pixel: pre-walked prefix of the primary march (MARCH estimator)
    DevBuf<uint32_t> d_pixels;        // this shard's box-hitting pixels, padded to groups of 64
    DevBuf<float4> d_start;           // ... and what a sample of each of those slots starts from (BatchArgs::start; MARCH, CT_START_RECORDS=0: none)
    // per pixel: its class, 0 = misses the box, 1 = listed, 2 = through (hit_flags_kernel; device, pinned host copy); behind
    // the plane, at the next multiple of 8 bytes, one 64-bit word: the lookups of one sample of every through pixel, summed
    DevBuf<uint8_t> d_hit;
    HostBuf<uint8_t> hit_host;
    DevBuf<uint32_t> d_cost;          // measured per group: [0,n) sum of path costs, [n,2n) deepest path
    DevBuf<uint32_t> d_touched[2];    // ct_debug_track_lines: one bit per line of the density / shadow arrays
    size_t touched_lines[2] = { 0, 0 };
    DevBuf<unsigned long long> d_timeline;      // CT_TIMELINE=1: [start, end] of every wave of the last enqueued estimator launch (MARCH)
    DevBuf<uint2> d_cost_plane;       // ... as the cost-measuring launch leaves them, per sample (BatchArgs::cost)
    DevBuf<uint32_t> d_job_group, d_job_sub;               // job list of the current batch size 
    uint32_t n_groups = 0;
    uint32_t n_jobs = 0, jobs_S = 0;
    HostBuf<uint32_t> jobs_host_g, jobs_host_s;                // the list as built on the host (pinned)
    bool jobs_brief = false;          // the list was laid out for short launches (short_batch)
    // The job list is built chunk by chunk: a chunk is a contiguous piece of `chunk_groups` groups of the cost-sorted
    // group order, and a launch renders all S subframes of ONE chunk into a scratch region of chunk_groups * 64 columns --
    // so the per-sample scratch does not have to hold the whole frame, while a launch still works through a few pixel groups at
    // a time for all their subframes (what keeps its paths close together in the volume; cutting a batch by SUBFRAMES
    // instead makes every launch sweep the whole image and costs 9-14 %).
    uint32_t chunk_groups = 0, n_chunks = 0;
    std::vector<std::array<uint32_t, kQueues + 2>> chunk_q_begin;   // per chunk: job ranges of the queues (absolute indices)
    DevBuf<uint32_t> d_group_rank, d_group_order;                   // place of a group in the job order / the group at a place
    uint32_t jobs_hint = 0;           // batch size the caller asked for last (job lists are built for it)
    // subframes per job at most (cheap groups), and the bounces (x cost unit) a job's lane is expected to run.
    // Re-swept on the final kernels (8 / 256 before): +4.3 % at 512^3, +5.6 % at 1024^3, +2.6 % at 256^3, +1.3 % DELTA
    // (16 / 48 until the end of round 2; 16 / 16 since: the whole-frame launch does not care, 3288 either way, a rank's
    // launch of an eighth of the tiles is 1.6 % shorter, 43.6 instead of 44.3 ms)
    uint32_t job_max = 16;
    float job_work = 16.f;
    // This shard's pixels; those whose primary ray hits the box (what short_batch and the other heuristics are tuned on) =
    // listed_pixels (in the pixel list: their samples are rendered) + through_pixels (the ray crosses the box without meeting
    // a non-zero footprint: every sample is (0,0,0,1) after through_steps / through_pixels lookups on average, settled by the
    // host's counters and the accumulate kernel's constant blocks; 0 unless through_on())
    uint64_t own_pixels = 0, hit_pixels = 0, listed_pixels = 0, through_pixels = 0, through_steps = 0;
    uint64_t miss_pixels = 0;            // own_pixels - hit_pixels (ct_debug_pixel_classes)
    bool queue_dirty = true, order_tuned = false;
    bool no_advance = false;             // CT_NO_ADVANCE=1: samples start at the box face (A/B)
    bool queues_enabled = false;         // per-XCD regions (CT_XCD_QUEUES=1; default: one global list)
    float shared_depth = 1e30f;          // groups at least this deep (bounces) use the shared queue
    uint32_t regions = 128;              // image regions dealt to the per-XCD queues
    std::vector<uint32_t> group_order;   // groups, most expensive first (until tuned: by what the last pose measured for their tiles)
    std::vector<uint32_t> group_tile;    // the 8x8 tile of a group's first pixel
    std::vector<uint32_t> tile_deepest;  // per tile of the image: the deepest path the last measured pose produced there (0 = never measured)
    std::vector<uint32_t> job_order;     // the order the job list is built in: group_order, or its chunks interleaved (build_jobs)
    bool chunk_interleave = false;       // CT_CHUNK_INTERLEAVE=1: every chunk is every C-th group of group_order (A/B: worse, the neighbours are gone)
    bool chunk_morton = false;           // CT_CHUNK_MORTON=1: chunks are compact image regions (A/B)
    bool tile_hilbert = false;           // CT_TILE_ORDER=hilbert: pixel groups along a Hilbert curve instead of Morton order (A/B)
    std::vector<float> group_depth;      // measured mean path cost per group (0 until tuned), in the
                                         // units of BatchArgs::cost
    unsigned long long host_paths = 0, host_hits = 0; // paths / box hits of the persistent path
    unsigned long long host_lookups = 0;  // density lookups of the samples of through pixels, which no kernel marches
    unsigned long long host_settled = 0;  // ... and their number (ct_debug_invariants: dealt and written include them)
    DevBuf<uint32_t> d_queue;
    DevBuf<unsigned long long> d_counters;    // kCounterCount + 1 (unconverged) + kStatCount
    DevBuf<float> d_colsum, d_avg;
    uint32_t reinhard_generation = 0;   // launches on d_avg's barrier counter (launch_reinhard)

    // CT_DEBUG_INVARIANTS=1: the diagnostics build of the estimator counts samples dealt / paths resumed / results
    // written / paths suspended, the scratch is filled with NaNs before every launch, and every point at which
    // nothing is in flight checks: dealt + resumed == written + suspended, resumed == suspended, dealt == what the
    // host handed out, no sample without alpha 1 reached an accumulate kernel.  A violation fails the call.
    bool debug_invariants = false;
    uint64_t iv_expected_dealt = 0, iv_checks = 0, iv_violations = 0;

    // ct_point_radiance_launch: a collector calls it about a thousand times per scene setup, each call a launch of a few
    // milliseconds, so its device buffers stay (grown on demand; freeing one would wait for the whole device, i.e. for
    // the launches of the other scene setups in flight)
    struct PointBuffers {
        DevBuf<CtPointRadianceTask> tasks;
        DevBuf<float4> primary, frames;
        DevBuf<uint32_t> pixels, jg, js;
    } pt;
    bool point_order = true;             // CT_POINT_ORDER=0: jobs of 8 frames in task order over 8 queues, as until round 2 (A/B)

    size_t volume_bytes = 0;
    LaunchShape shape{ 1024, 256, false };
    // CT_EXCHANGE=1: the estimator kernels with a block-wide exchange of paths between waves (ct_exchange.hpp) render the
    // batches whose job order is tuned; the cost-measuring launch of a pose keeps the per-lane kernels
    int exchange = 0;                  // 0 per-lane kernels, 1 block-wide exchange, 2 exchange within a wave
    LaunchShape xshape{ 256, 1024, false };
    uint32_t subframes = 0;
    double render_ms = 0, accum_ms = 0;
    double dframe_scatter_ms = 0, dframe_gather_ms = 0;   // the last ct_descriptor_frame (ct_debug_descriptor_frame_time)
    // ct_network_render_*, ct_baked_render_* and the bake's chunks: the temporaries of a band stay with the handle (a frame is
    // many bands, a render many frames).  The baked renderer uses found / waves / direct only, reserved at the same sizes.
    // found / waves / pos / dir / aux / out hold a band of band_cap pixels; desc holds desc_records() records, the largest count
    // seen so far (or what the device gave: a band with more records goes through gather and network in pieces).  direct holds
    // a band of direct.capacity() pixels and exists from the first call with CT_NET_ADD_SINGLE_SCATTER on; omega likewise, from
    // the first ct_baked_render_hybrid_* call on.
    struct NetScratch {
        DevBuf<float4> found, direct, omega;
        DevBuf<uint32_t> waves;
        DevBuf<float> pos, dir, aux, out;
        DevBuf<uint8_t> desc;
        size_t band_cap = 0;             // (found .. out: six buffers at different multiples of it)
        size_t desc_records() const { return desc.capacity() / CT_DESCRIPTOR_BYTES; }
        double ms[4] = { 0, 0, 0, 0 };   // the last ct_network_render_* call (ct_debug_network_render_time); a baked call leaves it
        // ct_network_render_shard_*: this shard's 8x8 tiles in ascending ty * tiles_x + tx (ct_shard_tiles), built on first use
        DevBuf<uint32_t> tiles;
        uint32_t n_tiles = 0;
        bool tiles_built = false;
    } net;
    uint64_t light_epoch = 0;   // bumped by ct_set_light: a CtBake remembers the one it was baked under
    double baked_ms = 0;        // the last ct_baked_render_* (ct_debug_baked_render_time)
    uint64_t launches = 0;
    std::string error;
};

namespace ct {

// Sets the handle's error text (h == NULL: the thread's ct_create error) and returns `code`.
int fail(CtHandle h, int code, const char *fmt, ...);

// The scheduler's part (ct_api.cpp) in a call that does not go through it.
int flush(CtHandle h);            // waits for the batches in flight
void discard_ahead(CtHandle h);
int enqueue_convergence_test(CtHandle h, uint32_t subframes);
// ct_point_radiance_launch's launch half (ct_api.cpp), shared with the traced bake and the device collector: job list, queue split, grid share, the
// estimator launch with `sc`, its time and the host counters.  rays / fold enqueue what fills h->pt.primary and h->pt.pixels
// before the estimator and what reads h->pt.frames[f * pad64(count) + i] behind it; the stream is idle when it returns.
int point_launch(CtHandle h, const DevScene &sc, uint32_t count, uint32_t first_frame_id, uint32_t launches,
                 const std::function<int()> &rays, const std::function<int()> &fold);

// ct_neural.cpp: the density mip pyramid, built on first use (ct_debug_layout reads it too).
int ensure_pyramid(CtHandle h);

} // namespace ct

#define HIPCHK(h, expr)                                                                              \
    do {                                                                                             \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess) {                                                                      \
            return fail((h), e_ == hipErrorOutOfMemory ? CT_E_NOMEM : CT_E_HIP, "%s failed: %s", #expr, \
                        hipGetErrorString(e_));                                                      \
        }                                                                                            \
    } while (0)

#define NEED_NOFLUSH(h)                                \
    do {                                               \
        if (!(h)) {                                    \
            return fail(nullptr, CT_E_INVAL, "null handle"); \
        }                                              \
        if (hipSetDevice((h)->device) != hipSuccess) { \
            return fail((h), CT_E_HIP, "hipSetDevice(%d) failed", (h)->device); \
        }                                              \
        (void)hipGetLastError(); /* a stale error of another library in this thread (RCCL leaves them) is not ours */ \
    } while (0)

// Every entry point except the *_async ones first waits for the batches in flight.
#define NEED(h)                                        \
    do {                                               \
        NEED_NOFLUSH(h);                               \
        const int rc_flush_ = flush(h);                \
        if (rc_flush_ != CT_OK) {                      \
            return rc_flush_;                          \
        }                                              \
    } while (0)
