// Sanitizer driver for the host scheduler's planner (csrc/ct_plan.hpp: pixel list, tile order, job list, chunks, measured
// order; tests/test_plan.py; built by tests/sanitize/Makefile with -fsanitize=address,undefined).  TEST INFRASTRUCTURE.
//   plan_asan      plans over synthetic class planes and costs and checks what holds for ANY correct plan -- every listed
//                  pixel once, every group's subframes covered once, chunks and queues that abut, orders that are permutations --
//                  never a number taken from the planner itself.  Exit 0 and "plan ok", or the first violated property.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <limits>
#include <string>
#include <vector>

#include "../../deepestscatter_amd/csrc/ct_plan.hpp"

using namespace ct::plan;

static std::string g_case;   // what is being planned, for the message of a failed check

#define CHECK(cond)                                                                                         \
    do {                                                                                                    \
        if (!(cond)) {                                                                                      \
            std::fprintf(stderr, "plan_driver: line %d: %s\n  in: %s\n", __LINE__, #cond, g_case.c_str()); \
            std::exit(1);                                                                                   \
        }                                                                                                   \
    } while (0)

static bool is_permutation(const std::vector<uint32_t>& v)
{
    std::vector<uint8_t> seen(v.size(), 0);
    for (const uint32_t e : v)
    {
        if (e >= v.size() || seen[e]) return false;
        seen[e] = 1;
    }
    return true;
}

// ---- the curves ----------------------------------------------------------------------------------------------------------------

static void check_curves()
{
    g_case = "curves";
    std::vector<uint8_t> seen_m(64 * 64 * 4, 0), seen_h(64 * 64, 0);
    for (uint32_t y = 0; y < 64; y++)
        for (uint32_t x = 0; x < 64; x++)
        {
            uint32_t bits = 0;
            for (int i = 0; i < 16; i++) bits |= ((x >> i) & 1u) << (2 * i) | ((y >> i) & 1u) << (2 * i + 1);
            const uint32_t m = morton2(x, y), hb = hilbert2(x, y);
            CHECK(m == bits && m < 64 * 64);
            CHECK(!seen_m[m]);
            seen_m[m] = 1;
            CHECK(hb < 64 * 64 && !seen_h[hb]);
            seen_h[hb] = 1;
        }
    for (const uint32_t v : { 0x7fffu, 0xffffu, 0x5555u })
    {
        uint32_t bits = 0;
        for (int i = 0; i < 16; i++) bits |= ((v >> i) & 1u) << (2 * i) | ((~v >> i) & 1u) << (2 * i + 1);
        CHECK(morton2(v, ~v & 0xffffu) == bits);
    }
    // Hilbert: along a 2^k square the ranks are 0 .. 4^k - 1 and consecutive ranks are edge neighbours
    for (uint32_t k = 1; k <= 6; k++)
    {
        const uint32_t n = 1u << k;
        std::vector<int> at_x(n * n, -1), at_y(n * n, -1);
        for (uint32_t y = 0; y < n; y++)
            for (uint32_t x = 0; x < n; x++)
            {
                const uint32_t d = hilbert2(x, y);
                CHECK(d < n * n && at_x[d] < 0);
                at_x[d] = (int)x;
                at_y[d] = (int)y;
            }
        for (uint32_t d = 1; d < n * n; d++) CHECK(std::abs(at_x[d] - at_x[d - 1]) + std::abs(at_y[d] - at_y[d - 1]) == 1);
    }
}

// ---- frames ----------------------------------------------------------------------------------------------------------------------

struct Frame
{
    const char* name;
    uint32_t W, H, shard_index, shard_count;
    int plane;   // 0: a disc of 1s with a rim of 2s, 1: all 1, 2: all miss
};

struct Planned
{
    uint32_t tiles_x = 0, tiles_y = 0;
    std::vector<uint8_t> cls;
    std::vector<uint32_t> list, group_tile;
    PixelCounts n;
};

static bool owns(const Frame& f, uint32_t tx, uint32_t ty)
{
    return f.shard_count <= 1 || (tx + 3u * ty) % f.shard_count == f.shard_index;
}

static Planned plan_frame(const Frame& f, bool hilbert)
{
    Planned p;
    p.tiles_x = (f.W + kTile - 1) / kTile;
    p.tiles_y = (f.H + kTile - 1) / kTile;
    p.cls.assign((size_t)f.W * f.H, 0);
    for (uint32_t y = 0; y < f.H; y++)
        for (uint32_t x = 0; x < f.W; x++)
        {
            const double dx = (x + 0.5) / f.W - 0.5, dy = (y + 0.5) / f.H - 0.5, r = std::sqrt(dx * dx + dy * dy);
            p.cls[(size_t)y * f.W + x] = f.plane == 1 ? 1 : f.plane == 2 ? 0 : r < 0.36 ? 1 : r < 0.43 ? 2 : (x + y) % 7 == 0 ? 3 : 0;
        }
    p.list.assign(5, 12345u);   // (stale contents must not survive)
    p.group_tile.assign(3, 777u);
    p.n = list_pixels(p.cls.data(), f.W, f.H, p.tiles_x, p.tiles_y, hilbert, [&](uint32_t tx, uint32_t ty) { return owns(f, tx, ty); }, p.list,
                      p.group_tile);
    // brute force over the pixels: what is owned, listed, through
    uint64_t own = 0, listed = 0, through = 0, miss = 0;
    for (uint32_t y = 0; y < f.H; y++)
        for (uint32_t x = 0; x < f.W; x++)
            if (owns(f, x / kTile, y / kTile))
            {
                own++;
                const uint8_t c = p.cls[(size_t)y * f.W + x];
                (c == 1 ? listed : c == 2 ? through : miss)++;
            }
    CHECK(p.n.own == own && p.n.listed == listed && p.n.through == through && own == listed + through + miss);
    CHECK(p.list.size() % 64 == 0 && p.list.size() >= listed && p.list.size() - listed < 64);
    std::vector<uint8_t> seen(p.cls.size(), 0);
    uint32_t last_key = 0, last_tile = 0xffffffffu, last_lane = 0;
    for (size_t i = 0; i < p.list.size(); i++)
    {
        const uint32_t px = p.list[i];
        if (i >= listed)
        {
            CHECK(px == 0xffffffffu);   // padding, at the end only
            continue;
        }
        CHECK(px < p.cls.size() && p.cls[px] == 1 && !seen[px]);
        seen[px] = 1;
        const uint32_t x = px % f.W, y = px / f.W, tx = x / kTile, ty = y / kTile, tile = ty * p.tiles_x + tx;
        CHECK(owns(f, tx, ty));
        // the order: tiles along the curve, a tile's pixels row by row
        const uint32_t key = hilbert ? hilbert2(tx, ty) : morton2(tx, ty), lane = (y % kTile) * kTile + x % kTile;
        if (tile == last_tile)
            CHECK(lane > last_lane);
        else
            CHECK(last_tile == 0xffffffffu || key > last_key);
        last_key = key;
        last_tile = tile;
        last_lane = lane;
    }
    CHECK(p.group_tile.size() == p.list.size() / 64);
    for (size_t g = 0; g < p.group_tile.size(); g++)
    {
        const uint32_t px = p.list[g * 64];
        CHECK(p.group_tile[g] == (px / f.W / kTile) * p.tiles_x + (px % f.W) / kTile);
    }
    return p;
}

// ---- the measured order ----------------------------------------------------------------------------------------------------------

// is `order` a permutation sorted by key(g), greatest first, index order within equal keys?
template <class Key>
static void check_sorted_stable(const std::vector<uint32_t>& order, Key key)
{
    CHECK(is_permutation(order));
    for (size_t r = 1; r < order.size(); r++)
    {
        const uint64_t a = key(order[r - 1]), b = key(order[r]);
        CHECK(a >= b);
        if (a == b) CHECK(order[r - 1] < order[r]);
    }
}

constexpr uint32_t kMeasured = 16;

// A fixed LCG sequence of costs in which about 2 % of the groups are a thousand times deeper than the rest.
static std::vector<uint32_t> synthetic_costs(uint32_t n_groups)
{
    std::vector<uint32_t> cost(2 * (size_t)n_groups);
    uint32_t x = 2463534242u;
    for (uint32_t g = 0; g < n_groups; g++)
    {
        x = x * 1664525u + 1013904223u;
        const bool deep = (x >> 8) % 50u == 0u || g == n_groups / 3;   // (one at least)
        const uint32_t bounces = 1u + (x >> 20) % 8u;                  // mean depth 1 .. 8, in units of BatchArgs::cost
        cost[g] = 64u * kMeasured * bounces * (deep ? 1000u : 1u);
        cost[n_groups + g] = deep ? 1000u + (x >> 12) % 1000u : (x >> 12) % 17u;   // deepest path (0: nothing measured)
    }
    return cost;
}

struct Tuned
{
    std::vector<uint32_t> group_order, tile_deepest;
    std::vector<float> group_depth;
};

static Tuned tune_frame(const Planned& p, const std::vector<uint32_t>& cost)
{
    const uint32_t n = (uint32_t)p.group_tile.size();
    const size_t n_tiles = (size_t)p.tiles_x * p.tiles_y;
    Tuned t;
    t.tile_deepest.assign(2, 99u);   // (stale)
    tune_groups(cost.data(), n, kMeasured, p.group_tile, n_tiles, t.group_order, t.group_depth, t.tile_deepest);
    const uint32_t* deepest = cost.data() + n;
    CHECK(t.group_order.size() == n && t.group_depth.size() == n && t.tile_deepest.size() == n_tiles);
    check_sorted_stable(t.group_order, [&](uint32_t g) { return (uint64_t)log2_class(deepest[g]) << 32 | log2_class(cost[g]); });
    std::vector<uint32_t> tile_max(n_tiles, 0);
    for (uint32_t g = 0; g < n; g++)
    {
        CHECK(t.group_depth[g] == (float)cost[g] / (64.f * (float)kMeasured));
        tile_max[p.group_tile[g]] = std::max(tile_max[p.group_tile[g]], deepest[g]);
    }
    CHECK(tile_max == t.tile_deepest);
    // ... and the next pose's first order, seeded from these tiles
    std::vector<uint32_t> seeded(1, 5u);
    seed_group_order(p.group_tile, t.tile_deepest, n_tiles, seeded);
    CHECK(seeded.size() == n);
    check_sorted_stable(seeded, [&](uint32_t g) { return (uint64_t)log2_class(t.tile_deepest[p.group_tile[g]]); });
    return t;
}

// ---- the job list ------------------------------------------------------------------------------------------------------------------

static std::vector<uint32_t> g_jg, g_js;   // the caller-provided storage, grown as needed, with one guard entry behind the list

static void check_jobs(const JobPolicy& pol, const std::vector<float>& depth, const std::vector<uint32_t>& group_order, uint32_t S,
                       uint32_t chunk_groups_asked)
{
    const uint32_t n = (uint32_t)depth.size(), cg = clamp_chunk_groups(chunk_groups_asked, n);
    CHECK(cg >= 1 && cg <= std::max(n, 1u));
    const size_t total = count_jobs(pol, depth, S);
    if (g_jg.size() < total + 1)
    {
        g_jg.resize(total + 1);
        g_js.resize(total + 1);
    }
    g_jg[total] = g_js[total] = 0xdeadbeefu;
    JobPlan jp;
    jp.job_order.assign(3, 9u);   // (stale)
    fill_jobs(pol, depth, group_order, S, cg, g_jg.data(), g_js.data(), jp);
    CHECK(jp.n_jobs == total);   // the count pass sized the storage
    CHECK(g_jg[total] == 0xdeadbeefu && g_js[total] == 0xdeadbeefu);
    CHECK(jp.job_order.size() == n && is_permutation(jp.job_order) && jp.rank.size() == n);
    for (uint32_t r = 0; r < n; r++) CHECK(jp.rank[jp.job_order[r]] == r);
    CHECK(jp.n_chunks == (n ? (n + cg - 1) / cg : 1u) && jp.chunk_q_begin.size() == jp.n_chunks);
    const float shared_cost = pol.shared_depth * pol.unit;
    std::vector<uint32_t> next_sub(n, 0), queue_of(n, 0xffffffffu);
    std::array<double, kQueues + 1> weight{};
    double weight_all = 0;
    size_t at = 0;
    const uint32_t *jg = g_jg.data(), *js = g_js.data(), *rank = jp.rank.data();   // (raw pointers: millions of jobs at -O1)
    uint32_t *next = next_sub.data(), *queue = queue_of.data();
    for (uint32_t c = 0; c < jp.n_chunks; c++)
    {
        const auto& qb = jp.chunk_q_begin[c];
        CHECK(qb[0] == at);   // chunks abut, the first begins at 0
        const uint32_t r0 = c * cg, r1 = std::min(n, r0 + cg);
        for (uint32_t x = 0; x <= (uint32_t)kQueues; x++)
        {
            CHECK(qb[x] <= qb[x + 1] && qb[x + 1] <= total);
            for (size_t j = qb[x]; j < qb[x + 1]; j++)
            {
                const uint32_t g = jg[j], begin = js[j] & 0xffffu, count = js[j] >> 16;
                CHECK(g < n && rank[g] >= r0 && rank[g] < r1);
                CHECK(queue[g] == 0xffffffffu || queue[g] == x);   // a group has one queue (and so one chunk)
                if (queue[g] == 0xffffffffu)
                {
                    weight[x] += (double)depth[g] + pol.unit;
                    weight_all += (double)depth[g] + pol.unit;
                }
                queue[g] = x;
                CHECK(begin == next[g]);   // ascending, no gap, no overlap
                CHECK(count >= 1 && count <= pol.job_max && count <= 0xffffu && begin + count <= S);
                CHECK(pol.order_tuned || count == 1);
                next[g] += count;
            }
        }
        at = qb[kQueues + 1];
    }
    CHECK(at == total);
    for (uint32_t g = 0; g < n; g++)
    {
        CHECK(next_sub[g] == S);
        if (pol.nq == 1) CHECK(queue_of[g] == 0);
        if (pol.nq == (uint32_t)kQueues) CHECK((queue_of[g] == (uint32_t)kQueues) == (depth[g] >= shared_cost));
        CHECK(queue_of[g] == (uint32_t)kQueues || queue_of[g] < pol.nq);
    }
    for (int x = 0; x <= kQueues; x++) CHECK(std::fabs(jp.q_weight[x] - weight[x]) <= 1e-9 * std::max(1.0, weight_all));
}

static void check_frame(const Frame& f)
{
    for (const bool hilbert : { false, true })
    {
        g_case = std::string(f.name) + (hilbert ? ", Hilbert" : ", Morton");
        const Planned p = plan_frame(f, hilbert);
        const uint32_t n = (uint32_t)p.group_tile.size();
        if (f.plane == 2) CHECK(n == 0 && p.list.empty());
        // untuned: index order (nothing measured before), every depth 0
        std::vector<uint32_t> first_order;
        seed_group_order(p.group_tile, {}, (size_t)p.tiles_x * p.tiles_y, first_order);
        CHECK(first_order.size() == n);
        for (uint32_t g = 0; g < n; g++) CHECK(first_order[g] == g);
        const std::vector<uint32_t> cost = synthetic_costs(n);
        const Tuned t = tune_frame(p, cost);
        const std::vector<float> zero_depth(n, 0.f);
        for (const bool tuned : { false, true })
            for (const uint32_t S : { 1u, 4u, 17u, 0xffffu })
                for (const uint32_t chunk_groups : { 1u, 5u, n })
                    for (const uint32_t nq : { 1u, (uint32_t)kQueues })
                        for (const float shared_depth : { 1e30f, 31.25f })   // (x unit 16 = 500: above the cheap groups' 8, below the deep ones' 1000)
                            for (int mode = 0; mode < 3; mode++)
                            {
                                if (nq > 1 && n < (uint32_t)kQueues) continue;   // (per-XCD queues need a group per queue at least)
                                // (the longest batch is millions of jobs per list: it runs with one tile order -- a job list sees the
                                // tile order through group_order alone, which the shorter batches cover -- and without a shared depth
                                // over depths that are all zero, which none of them reaches; untuned, when every job is one subframe,
                                // the frames of up to 32 groups have the same 65535 jobs per group as the larger ones)
                                if (S == 0xffffu && (hilbert || (!tuned && (shared_depth < 1e30f || n > 32)))) continue;
                                JobPolicy pol;
                                pol.nq = nq;
                                pol.shared_depth = shared_depth;
                                pol.order_tuned = tuned;
                                pol.chunk_interleave = mode == 1;
                                pol.chunk_morton = mode == 2;
                                pol.brief = nq > 1;   // the short-launch layout: 16 regions, job_work 4
                                pol.regions_wanted = pol.brief ? 16u : mode == 1 ? 3u : 128u;
                                pol.job_work = pol.brief ? 4.f : 16.f;
                                g_case = std::string(f.name) + (hilbert ? ", Hilbert" : ", Morton") + (tuned ? ", tuned" : ", untuned") + ", S " +
                                         std::to_string(S) + ", chunk_groups " + std::to_string(chunk_groups) + ", nq " + std::to_string(nq) +
                                         ", shared_depth " + std::to_string(shared_depth) + ", chunk mode " + std::to_string(mode);
                                check_jobs(pol, tuned ? t.group_depth : zero_depth, tuned ? t.group_order : first_order, S, chunk_groups);
                            }
    }
}

// ---- the small arithmetic ----------------------------------------------------------------------------------------------------------

static void check_arithmetic()
{
    g_case = "log2_class";
    CHECK(log2_class(0) == 0 && log2_class(1) == 1 && log2_class(2) == 2 && log2_class(3) == 2 && log2_class(4) == 3 && log2_class(0xffffffffu) == 32);
    for (uint32_t k = 1; k < 32; k++) CHECK(log2_class(1u << k) == k + 1 && log2_class((1u << k) - 1) == k);
    g_case = "wanted_regions";
    for (const int max_age : { 0, 1, 7, 63, 100 })
        for (const uint64_t need : std::initializer_list<uint64_t>{ 0, 1, 1000, 3000000, 1000000000, 0xffffffffull })
            for (const uint64_t budget : std::initializer_list<uint64_t>{ 0, need, 2 * need, 3 * need + 1, 100 * need, ~0ull })
            {
                const int r = wanted_regions(max_age, need, budget);
                CHECK(r >= 2 && r <= kMaxRegions);
                CHECK(r == 2 || (uint64_t)r * std::max<uint64_t>(need, 1) <= budget);   // (two at least, whatever the budget)
                if (max_age > 0) CHECK(r <= max_age + 1);
            }
    g_case = "region_groups / groups_per_chunk";
    const uint64_t half = 0xffffffffull / 2;
    for (const uint64_t region : std::initializer_list<uint64_t>{ 0, 1, 63, 64, 65536, 1ull << 30, 0xffffffffull, 1ull << 40, ~0ull })
        for (const uint32_t S : { 0u, 1u, 4u, 17u, 0xffffu, 0xffffffffu })
            for (const uint32_t n : { 0u, 1u, 64u, 16384u, 0xffffffffu })
            {
                const uint64_t per_group = (uint64_t)std::max(S, 1u) * 64, rg = region_groups(region, S);
                CHECK(rg * per_group <= std::min(region, half) && (rg + 1) * per_group > std::min(region, half));
                const uint32_t gc = groups_per_chunk(region, S, n);
                CHECK(gc >= 1 && gc <= std::max(n, 1u));
                CHECK(gc == 1 || gc * per_group <= std::min(region, half));   // (one group at least, whatever the region)
                CHECK(gc == std::max(n, 1u) || (gc + 1) * per_group > std::min(region, half));   // all of them when it can
            }
    g_case = "short_batch";
    CHECK(short_batch(false, 10, 1000000) && !short_batch(true, 10, 1000000) && !short_batch(false, 1024, 1000000) && short_batch(false, 0xffff, 0));
    g_case = "job_length";
    JobPolicy pol;
    CHECK(job_length(pol, 1e9f) == 1);   // untuned
    pol.order_tuned = true;
    CHECK(job_length(pol, 0.f) == pol.job_max && job_length(pol, 1e-30f) == pol.job_max && job_length(pol, 1e30f) == 1 &&
          job_length(pol, std::numeric_limits<float>::infinity()) == 1);
}

int main()
{
    check_curves();
    check_arithmetic();
    const Frame frames[] = {
        { "8 x 8 disc", 8, 8, 0, 1, 0 },          { "8 x 8 all listed", 8, 8, 0, 1, 1 },
        { "13 x 9 disc", 13, 9, 0, 1, 0 },        { "13 x 9 all listed", 13, 9, 0, 1, 1 },
        { "64 x 64 disc", 64, 64, 0, 1, 0 },      { "64 x 64 all listed", 64, 64, 0, 1, 1 },
        { "64 x 64 disc, shard 1 of 3", 64, 64, 1, 3, 0 }, { "64 x 64 all listed, shard 1 of 3", 64, 64, 1, 3, 1 },
        { "64 x 64 all miss", 64, 64, 0, 1, 2 },  { "13 x 9 all miss, shard 1 of 3", 13, 9, 1, 3, 2 },
    };
    for (const Frame& f : frames) check_frame(f);
    std::puts("plan ok");
    return 0;
}
