// ct_plan.hpp -- the host scheduler's planning as pure functions: which pixels form the list and in which tile order, which
// group goes to which XCD queue, how long a job is, how chunks are cut, how a measured pose re-sorts the groups.  Plain C++17
// over values and vectors: no device, no handle, no C ABI.  ct_api.cpp launches and downloads, calls in here, then reserves and
// copies; tests/sanitize/plan_driver.cpp checks the properties of a plan on the CPU under ASan + UBSan (tests/test_plan.py).
// Nothing in here changes a result: the order and the job lengths only change the schedule.
#pragma once

#include <algorithm>
#include <array>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace ct {
namespace plan {

// (ct_internal.hpp's kTile and kQueues and the handle's kMaxRegions: ct_api.cpp asserts that they are equal)
constexpr int kTile = 8;
constexpr int kQueues = 8;
constexpr int kMaxRegions = 64;

// Class of a cost or depth: 0 for 0, else k with 2^(k-1) <= c < 2^k.
inline uint32_t log2_class(uint32_t c)
{
    uint32_t k = 0;
    while (c) {
        k++;
        c >>= 1;
    }
    return k;
}

inline uint32_t morton2(uint32_t x, uint32_t y)
{
    auto spread = [](uint32_t v) {
        v &= 0xffffu;
        v = (v | (v << 8)) & 0x00ff00ffu;
        v = (v | (v << 4)) & 0x0f0f0f0fu;
        v = (v | (v << 2)) & 0x33333333u;
        v = (v | (v << 1)) & 0x55555555u;
        return v;
    };
    return spread(x) | (spread(y) << 1);
}

// Position of tile (x, y) along a Hilbert curve over a 2^15 x 2^15 grid (the standard xy2d): like the Morton index a
// locality-preserving order of the tiles, but without its jumps -- consecutive tiles are always neighbours.
inline uint32_t hilbert2(uint32_t x, uint32_t y)
{
    const uint32_t n = 1u << 15;
    uint32_t d = 0;
    for (uint32_t s = n / 2; s > 0; s /= 2) {
        const uint32_t rx = (x & s) ? 1u : 0u, ry = (y & s) ? 1u : 0u;
        d += s * s * ((3u * rx) ^ ry);
        if (ry == 0) {
            if (rx == 1) {
                x = n - 1u - x;
                y = n - 1u - y;
            }
            const uint32_t t = x;
            x = y;
            y = t;
        }
    }
    return d;
}

// ---- the pixel list ----------------------------------------------------------------------------------------------------------

struct PixelCounts {
    uint64_t own = 0, listed = 0, through = 0;   // (the rest of `own` misses the box)
};

// The list of a shard's pixels whose samples need a path -- class plane value 1; 2 = through pixel, anything else misses -- in
// tile-Morton (or Hilbert) order, a tile's 64 pixels row by row, padded with 0xffffffff to groups of 64 (one wave's worth);
// group_tile[i] = the 8x8 tile of group i's first pixel.  owns(tx, ty): is the tile this shard's?
// (always inlined: out of line, over a list behind a reference, the walk over a 1024^2 frame takes 1.49 ms instead of the 1.26 ms
// it takes as a loop over rebuild_queue's own locals -- profiles/r11a/host_phases.txt)
template <class Owns>
__attribute__((always_inline)) inline PixelCounts list_pixels(const uint8_t *cls, uint32_t W, uint32_t H, uint32_t tiles_x, uint32_t tiles_y, bool hilbert, Owns owns,
                               std::vector<uint32_t> &list, std::vector<uint32_t> &group_tile)
{
    std::vector<std::pair<uint32_t, uint32_t>> tiles;
    for (uint32_t ty = 0; ty < tiles_y; ty++) {
        for (uint32_t tx = 0; tx < tiles_x; tx++) {
            if (owns(tx, ty)) {
                tiles.emplace_back(hilbert ? hilbert2(tx, ty) : morton2(tx, ty), ty * tiles_x + tx);
            }
        }
    }
    std::sort(tiles.begin(), tiles.end());
    uint64_t own = 0, through = 0;
    list.clear();
    for (const auto &t : tiles) {
        const uint32_t ty = t.second / tiles_x, tx = t.second - ty * tiles_x;
        for (uint32_t l = 0; l < 64; l++) {
            const uint32_t x = tx * kTile + (l & 7u), y = ty * kTile + (l >> 3);
            if (x < W && y < H) {
                own++;
                const uint32_t p = y * W + x;
                if (cls[p] == 1u) {
                    list.push_back(p);
                } else if (cls[p] == 2u) {
                    through++;
                }
            }
        }
    }
    PixelCounts n;
    n.own = own;
    n.listed = list.size();
    n.through = through;
    while (list.size() % 64 != 0) {
        list.push_back(0xffffffffu);
    }
    group_tile.resize(list.size() / 64);
    for (size_t i = 0; i < group_tile.size(); i++) {
        const uint32_t p = list[i * 64];
        group_tile[i] = (p / W / kTile) * tiles_x + (p % W) / kTile;
    }
    return n;
}

// The group order of a pose that has measured nothing yet: index order, i.e. tile order -- or, where the last measured pose
// left the deepest path of every tile (tile_deepest has n_tiles entries), by that.
inline void seed_group_order(const std::vector<uint32_t> &group_tile, const std::vector<uint32_t> &tile_deepest, size_t n_tiles,
                             std::vector<uint32_t> &group_order)
{
    group_order.resize(group_tile.size());
    for (size_t i = 0; i < group_order.size(); i++) {
        group_order[i] = (uint32_t)i;
    }
    if (tile_deepest.size() == n_tiles) {
        // The cost-measuring launch of this pose is waited for to its last path, so it should START with the groups whose paths
        // are long.  Where those were for the last pose that was measured is a good guess while the camera is dragged
        // (Camera::rotate, Camera.cpp:93-98): classes of the deepest path seen in a group's tile, deepest first, tile order within.
        std::stable_sort(group_order.begin(), group_order.end(), [&](uint32_t a, uint32_t b) {
            return log2_class(tile_deepest[group_tile[a]]) > log2_class(tile_deepest[group_tile[b]]);
        });
    }
}

// ---- the measured order ------------------------------------------------------------------------------------------------------

// Longest-processing-time-first: visit the groups whose paths were deepest first, so that the
// 2000-bounce paths start at the head of the launch instead of becoming its tail.  Groups of
// the same cost class (power of two) keep their Morton order for cache locality.
// cost: [0, n) the groups' summed path costs over `measured_subframes` subframes, [n, 2n) their deepest paths.
inline void tune_groups(const uint32_t *cost, uint32_t n_groups, uint32_t measured_subframes, const std::vector<uint32_t> &group_tile,
                        size_t n_tiles, std::vector<uint32_t> &group_order, std::vector<float> &group_depth,
                        std::vector<uint32_t> &tile_deepest)
{
    // Order: by the deepest path a group has produced (a launch ends when its last path does, so
    // the groups that can produce long paths must not be the last ones running), then by mean cost.
    const uint32_t *deepest = cost + n_groups;
    tile_deepest.assign(n_tiles, 0u);
    group_order.resize(n_groups);
    group_depth.resize(n_groups);
    for (uint32_t g = 0; g < n_groups; g++) {
        group_order[g] = g;
        group_depth[g] = (float)cost[g] / (64.f * (float)measured_subframes);
        if (g < group_tile.size()) {
            uint32_t &t = tile_deepest[group_tile[g]];
            t = std::max(t, deepest[g]);   // (a guess for the next pose's cost-measuring launch: seed_group_order)
        }
    }
    std::stable_sort(group_order.begin(), group_order.end(), [&](uint32_t a, uint32_t b) {
        const uint32_t ka = log2_class(deepest[a]), kb = log2_class(deepest[b]);
        if (ka != kb) {
            return ka > kb;
        }
        return log2_class(cost[a]) > log2_class(cost[b]);
    });
}

// Share of the measured cost by class of the deepest path seen (CT_STATS).
struct CostShare {
    std::array<double, 34> share{};
    std::array<uint32_t, 34> count{};
    double total = 0;
};

inline CostShare cost_share(const uint32_t *cost, uint32_t n_groups)
{
    const uint32_t *deepest = cost + n_groups;
    CostShare s;
    for (uint32_t g = 0; g < n_groups; g++) {
        s.share[log2_class(deepest[g])] += cost[g];
        s.count[log2_class(deepest[g])] += 1;
        s.total += cost[g];
    }
    return s;
}

// ---- batch sizes, regions, chunks --------------------------------------------------------------------------------------------

// A launch of about 5 ms or less (10-40 subframes of a 1024^2 frame: the reference's display cadence, Camera.cpp:189).  Such a
// launch works on EVERY pixel group at once instead of a few neighbouring ones for a thousand subframes each, and its paths
// miss L2 half again as often at the same instruction count (profiles/r03f/pmc_prog.txt: hit rate 41 % instead of 62 %); what
// helps is keeping an XCD on a compact part of the image -- per-XCD queues over 16 regions -- with single-subframe jobs for
// every group deeper than four bounces and refills of 16 lanes at a time: 5.43 -> 4.74 ms per 10-subframe update.
inline bool short_batch(bool delta, uint32_t S, uint64_t hit_pixels)
{
    // (MARCH only: the DELTA kernel, which makes a sixteenth of the fetches, loses 3 % with this layout -- 3.94 vs 3.82 ms)
    return !delta && (double)S * (double)std::max<uint64_t>(hit_pixels, 1) < 4.0e7;
}

// How many regions a batch that needs `need` entries of scratch should have: enough launches between a batch and its accumulate
// kernel that no path of it is still running -- a path needs up to ~10 ms (2000 bounces) of running time, a launch lasts about
// as long as its samples take at ~3 Gsamples/s -- but never more than the budget holds.  max_age_override > 0: that many + 1.
inline int wanted_regions(int max_age_override, uint64_t need, uint64_t budget_float4)
{
    int r;
    if (max_age_override > 0) {
        r = max_age_override + 1;
    } else {
        const double est_ms = std::max(0.05, (double)need / 3.0e6);
        r = 1 + (int)std::ceil(15.0 / est_ms);
    }
    r = (int)std::min<uint64_t>((uint64_t)r, std::max<uint64_t>(budget_float4 / std::max<uint64_t>(need, 1), 2));
    return std::min(kMaxRegions, std::max(2, r));
}

// Pixel groups whose S subframes fit a scratch region of `region_float4` entries (0: not even one).
inline uint64_t region_groups(uint64_t region_float4, uint32_t S)
{
    // (two regions at least, and result indices are 32 bits)
    const uint64_t cap = std::min<uint64_t>(region_float4, 0xffffffffull / 2);
    return cap / ((uint64_t)std::max(S, 1u) * 64);
}

// How many pixel groups a launch of S subframes renders at once: what one scratch region holds (all of them when it can).
inline uint32_t groups_per_chunk(uint64_t region_float4, uint32_t S, uint32_t n_groups)
{
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(region_groups(region_float4, S), std::max(n_groups, 1u)));
}

// ---- the job list ------------------------------------------------------------------------------------------------------------

// What the handle and the knobs decide about a job list (ct_api.cpp: job_policy).
struct JobPolicy {
    float unit = 16.f;             // cost units per bounce (BatchArgs::cost): MARCH counts fetches + 4 per bounce, DELTA bounces
    bool brief = false;            // the list is laid out for short launches (short_batch)
    uint32_t nq = 1;               // queues in use: kQueues, one per XCD, or 1
    uint32_t regions_wanted = 128; // image regions dealt to the per-XCD queues
    float job_work = 16.f;         // the bounces (x unit) a job's lane is expected to run ...
    uint32_t job_max = 16;         // ... and subframes per job at most (cheap groups)
    float shared_depth = 1e30f;    // groups at least this deep (bounces) use the shared queue
    bool order_tuned = false;      // group_depth is measured (else: all zero, one-subframe jobs)
    bool chunk_interleave = false, chunk_morton = false;
};

// A job is (group, subframe range); its length is chosen
// so that a job's expected serial work per lane stays bounded: groups whose paths are deep get
// one-subframe jobs, cheap groups up to 16 subframes per job (job_max, job_work).
// (Round 10, with the through pixels off the list: 98.7 % of the benchmark pose's cost is in groups that this rule gives
// one-subframe jobs already.  One subframe for EVERY group measures the same (4083 against 4080 Msamples/s, L2 hit rate 74.8 %
// both); 2 / 4 / 8 subframes for every group 4080 / 4079 / 4066, and at 8 the hit rate falls to 71.0 %: longer jobs lose
// locality now, shorter ones have nothing left to gain.  The rule stays.  profiles/r10a)
inline uint32_t job_length(const JobPolicy &p, float depth)
{
    if (!p.order_tuned) {
        // the cost-measuring launch of a pose knows no depths yet: ONE subframe per job, or the wave that gets a group of the
        // cloud's body runs its eight or ten subframes one after another in the same 64 lanes -- 21 ms for 10 subframes
        // of a 1024^2 frame that are 13 ms once the order is set
        return 1u;
    }
    uint32_t len = p.job_max;
    if (depth > 0.f) {
        len = (uint32_t)std::min((float)p.job_max, std::max(1.f, p.job_work * p.unit / depth));
    }
    return len;
}

// The count pass: jobs of a list for batches of S subframes.
inline size_t count_jobs(const JobPolicy &p, const std::vector<float> &group_depth, uint32_t S)
{
    size_t total_jobs = 0;
    for (const float d : group_depth) {
        const uint32_t len = job_length(p, d);
        total_jobs += (S + len - 1) / len;
    }
    return total_jobs;
}

// Chunk size as the job list uses it: at least one group, at most all of them.
inline uint32_t clamp_chunk_groups(uint32_t chunk_groups, uint32_t n_groups)
{
    return std::max(1u, std::min(chunk_groups, std::max(n_groups, 1u)));
}

struct JobPlan {
    std::vector<uint32_t> job_order;   // the order the list is built in: group_order, or its chunks interleaved
    std::vector<uint32_t> rank;        // ... and its inverse: the place of a group
    std::vector<std::array<uint32_t, kQueues + 2>> chunk_q_begin;   // per chunk: job ranges of the queues (absolute indices)
    uint32_t n_chunks = 1;
    size_t n_jobs = 0;
    std::array<double, kQueues + 1> q_weight{};   // per queue: the cost estimate of its groups (CT_STATS)
};

// The fill pass.  jg / js have room for count_jobs() entries: (group, first subframe | count << 16), chunk by chunk (a
// contiguous piece of `chunk_groups` places of the job order each), and within a chunk queue by queue.
// (the list itself is written into pinned host memory that stays with the handle: a new pose builds it twice, and 860 k
// jobs in two fresh vectors cost 9 ms of page faults and staged copies)
inline void fill_jobs(const JobPolicy &p, const std::vector<float> &group_depth, const std::vector<uint32_t> &group_order, uint32_t S,
                      uint32_t chunk_groups, uint32_t *jg, uint32_t *js, JobPlan &out)
{
    const uint32_t n_groups = (uint32_t)group_depth.size(), nq = p.nq;
    const float unit = p.unit;
    // One queue per XCD: groups are in tile-Morton order, so a contiguous range of them is a
    // compact image region whose paths read a compact part of the volume.  The ranges are cut at
    // equal shares of the measured cost (path depth + the primary march), not of the pixel count.
    // Groups whose paths are deep (mean cost >= shared_depth bounces) go to the shared queue.
    const float shared_cost = p.shared_depth * unit;
    std::vector<uint8_t> queue_of(n_groups, 0);
    {
        double total = 0;
        for (uint32_t g = 0; g < n_groups; g++) {
            if (nq > 1u && group_depth[g] >= shared_cost) {
                queue_of[g] = (uint8_t)kQueues;
            } else {
                total += (double)group_depth[g] + unit;
            }
        }
        double run = 0;
        for (uint32_t g = 0; g < n_groups; g++) {
            if (queue_of[g] == (uint8_t)kQueues) {
                continue;
            }
            const double w = (double)group_depth[g] + unit;
            // regions_wanted compact image regions of equal cost, dealt round-robin to the queues: every
            // XCD still works on 1/8 of the image (a handful of compact pieces), and errors of the
            // cost estimate, which are correlated in space, average out over its pieces
            const uint32_t regions = std::max(nq, p.regions_wanted);
            const uint32_t r = (uint32_t)std::min<double>(regions - 1, std::floor((run + 0.5 * w) / total * regions));
            queue_of[g] = (uint8_t)(r % nq);
            run += w;
        }
    }
    const uint32_t n_chunks = n_groups ? (n_groups + chunk_groups - 1) / chunk_groups : 1u;
    if (n_chunks > 1 && p.chunk_interleave) {
        // Every chunk gets the same mix of expensive and cheap groups (2 % of the groups make 98 % of the cost): the job order
        // becomes places 0, C, 2C, ... of the cost-sorted order, then 1, C + 1, ..., so that a contiguous piece of it is every
        // C-th group -- launches of equal length instead of a few long ones and many that are over before the paths they
        // resumed have moved.
        // (pieces must be whole chunks: with n_groups not a multiple of n_chunks the first chunks are one group longer than
        // chunk_groups allows only if chunk_groups * n_chunks < n_groups, which the rounding above excludes)
        out.job_order.clear();
        out.job_order.reserve(n_groups);
        for (uint32_t c = 0; c < n_chunks; c++) {
            for (uint32_t r = c; r < n_groups; r += n_chunks) {
                out.job_order.push_back(group_order[r]);
            }
        }
    } else if (n_chunks > 1 && p.chunk_morton) {
        // (probe: chunks = compact image regions -- the groups in tile-Morton order, which is their index order)
        out.job_order.resize(n_groups);
        for (uint32_t g = 0; g < n_groups; g++) {
            out.job_order[g] = g;
        }
    } else {
        out.job_order = group_order;
    }
    // the job order both ways: where a group's results go in its chunk's scratch, and whose a column is
    out.rank.resize(n_groups);
    for (uint32_t r = 0; r < n_groups; r++) {
        out.rank[out.job_order[r]] = r;
    }
    size_t nj = 0;
    out.q_weight.fill(0.0);
    out.chunk_q_begin.assign(n_chunks, std::array<uint32_t, kQueues + 2>{});
    for (uint32_t c = 0; c < n_chunks; c++) {
        const uint32_t r0 = c * chunk_groups, r1 = std::min(n_groups, r0 + chunk_groups);
        for (uint32_t x = 0; x <= (uint32_t)kQueues; x++) {
            out.chunk_q_begin[c][x] = (uint32_t)nj;
            // (nq == 1: everything sits in queue 0 and the other XCDs' waves steal from it -- one global
            // cost-sorted list, the behaviour before the queues were split)
            if (x != 0u && nq == 1u && x != (uint32_t)kQueues) {
                continue;
            }
            for (uint32_t r = r0; r < r1; r++) {
                const uint32_t g = out.job_order[r];
                if (queue_of[g] != x) {
                    continue;
                }
                out.q_weight[x] += (double)group_depth[g] + unit;
                const uint32_t len = job_length(p, group_depth[g]);
                for (uint32_t s0 = 0; s0 < S; s0 += len) {
                    jg[nj] = g;
                    js[nj] = s0 | (std::min(len, S - s0) << 16);
                    nj += 1;
                }
            }
        }
        out.chunk_q_begin[c][kQueues + 1] = (uint32_t)nj;
    }
    out.n_chunks = n_chunks;
    out.n_jobs = nj;
}

} // namespace plan
} // namespace ct
