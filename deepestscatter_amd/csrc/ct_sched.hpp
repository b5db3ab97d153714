// ct_sched.hpp -- what the persistent-wave estimator kernels share: render_persistent_kernel (MARCH), render_delta_kernel
// (DELTA) and the experiments of ct_exchange.hpp.  Included by ct_kernels.hip (inside namespace ct, before the first of them).
//
//   jobs      xcd_id, JobState, group_column, take_leftover, hand_on_job, take_job, lane_rank
//   flights   Dda (the state of a DELTA flight), load_dda_prefix
//   epilogue  wave_sum, flush_counters
//
// Every function is force-inlined.  The resume / regenerate / suspend blocks are still written out in both kernel bodies: the
// kernels' register allocation follows the order in which their values are first named, and every helper tried for those
// blocks (with by-reference outputs, with a struct of the wave-uniform state) moved the allocation of all estimator kernels.

// The XCD this wave runs on (XCC_ID, hardware register 20, bits 3:0).
CT_DEV uint32_t xcd_id()
{
    return (uint32_t)__builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11)) & (uint32_t)(kQueues - 1);
}

// A job the previous launch handed on (BatchArgs::left_in).  Wave-uniform.
struct JobState {
    uint32_t g, next, end;       // pixel group; samples [next, end) still to start: sample q is lane q & 63 of the job's subframe q >> 6
    uint32_t base;               // scratch index of the job's first subframe, lane 0 (absolute: region, row and the group's column)
    uint32_t first;              // subframe id of the job's first subframe
    uint32_t age;                // the age its samples start with
};   // (six SGPRs that live through the whole scheduler loop; the scratch's row stride is the same for every job in flight)

// Where group g's 64 results of a subframe go within a subframe's row of the scratch (BatchArgs::group_rank).
CT_DEV uint32_t group_column(const BatchArgs &ba, uint32_t g)
{
    return (ba.group_rank ? __builtin_amdgcn_readfirstlane(ba.group_rank[g]) - ba.rank_base : g) * 64u;
}

CT_DEV bool take_leftover(const BatchArgs &ba, uint32_t lane, bool &left_done, JobState &job)
{
    if (!ba.left_in || left_done) {
        return false;
    }
    uint32_t i = 0;
    if (lane == 0) {
        i = atomicAdd(ba.left_cursor, 1u);
    }
    i = __builtin_amdgcn_readfirstlane(i);
    if (i >= __builtin_amdgcn_readfirstlane(*ba.left_in_count)) {
        left_done = true;
        return false;
    }
    const uint32_t *r = ba.left_in + (size_t)i * kLeftWords;
    job.g = __builtin_amdgcn_readfirstlane(r[0]);
    job.next = __builtin_amdgcn_readfirstlane(r[1]);
    job.end = __builtin_amdgcn_readfirstlane(r[2]);
    job.base = __builtin_amdgcn_readfirstlane(r[3]);
    job.first = __builtin_amdgcn_readfirstlane(r[4]);
    job.age = __builtin_amdgcn_readfirstlane(r[5]);
    return true;
}

// The rest of this wave's job goes to the next launch (see BatchArgs::left_out).  Returns false if there is no room.
CT_DEV bool hand_on_job(const BatchArgs &ba, uint32_t lane, const JobState &job)
{
    uint32_t i = 0;
    if (lane == 0) {
        i = atomicAdd(ba.left_out_count, 1u);
        if (i >= ba.left_capacity) {
            atomicSub(ba.left_out_count, 1u);
            i = 0xffffffffu;
        } else {
            uint4 *r = (uint4 *)(ba.left_out + (size_t)i * kLeftWords);
            r[0] = make_uint4(job.g, job.next, job.end, job.base);
            r[1] = make_uint4(job.first, job.age + 1u, 0u, 0u);
        }
    }
    return __builtin_amdgcn_readfirstlane(i) != 0xffffffffu;
}

// Next job for this wave: from the queue it is working on (first the shared one), else from its
// XCD's, else from the following ones.  Wave-uniform.  Returns false when every queue is empty.
CT_DEV bool take_job(const BatchArgs &ba, uint32_t lane, uint32_t &q_cur, uint32_t &q_tried, uint32_t &job)
{
    while (q_tried < (uint32_t)kQueues) {
        const uint32_t begin = ba.q_begin[q_cur], end = ba.q_begin[q_cur + 1];
        if (begin != end) {
            uint32_t j = 0;
            if (lane == 0) {
                j = atomicAdd(&ba.queue[q_cur], 1u);
            }
            j = __builtin_amdgcn_readfirstlane(j);
            if (j < end - begin) {
                job = ba.reverse ? end - 1u - j : begin + j;
                if (j + 1u == end - begin && lane == 0) {
                    // The last job of THIS queue.  The list is empty when that has happened to every queue that had jobs; whoever
                    // finds it so raises the flag that the other waves look at now and then (see poll_empty_hint).  (Until round
                    // 3 the flag went up with the job of the highest index, which is "the list is empty" for one queue only: with
                    // per-XCD queues the waves did not look at it, and a busy wave learnt that nothing was left only when 16 of
                    // its lanes had run out of work -- a launch of 10 subframes drained for 0.9 of its 4.3 ms.)
                    uint32_t with_jobs = 0;
                    for (uint32_t x = 0; x <= (uint32_t)kQueues; x++) {
                        with_jobs += (ba.q_begin[x] != ba.q_begin[x + 1u]) ? 1u : 0u;
                    }
                    if (atomicAdd(&ba.queue[kQueueDone], 1u) + 1u == with_jobs) {
                        __atomic_store_n(ba.queue + kQueueFlag, 1u, __ATOMIC_RELAXED);
                    }
                }
                return true;
            }
        }
        if (q_cur == (uint32_t)kQueues) {
            q_cur = xcd_id();
        } else {
            q_tried += 1;
            q_cur = (q_cur + 1u) & (uint32_t)(kQueues - 1);
        }
    }
    return false;
}

CT_DEV uint32_t lane_rank(uint64_t mask)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// The state of a DELTA flight.
struct Dda {
    f3 org;            // origin of the flight (box coordinates), positions are fma(dir, t, org)
    float t;
    f3 tmax, tdelta;   // ray parameter at the next cell boundary per axis / between boundaries
    int32_t bx, by, bz;
};

// The pixel's pre-walked DDA prefix (primary_advance_delta_kernel): the same seven values as four float4.
CT_DEV void load_dda_prefix(const BatchArgs &ba, uint32_t pixel, Dda &dda)
{
    const float4 a0 = ba.advance[4 * (size_t)pixel], a1 = ba.advance[4 * (size_t)pixel + 1];
    const float4 a2 = ba.advance[4 * (size_t)pixel + 2], a3 = ba.advance[4 * (size_t)pixel + 3];
    dda.org = mk3(a0.x, a0.y, a0.z);
    dda.t = a0.w;
    dda.tmax = mk3(a1.x, a1.y, a1.z);
    dda.bx = __float_as_int(a1.w);
    dda.tdelta = mk3(a2.x, a2.y, a2.z);
    dda.by = __float_as_int(a2.w);
    dda.bz = __float_as_int(a3.x);
}

// ---------------------------------------------------------------------------------------------
// Epilogue: per-lane tallies -> one atomic per counter per wave
// ---------------------------------------------------------------------------------------------
CT_DEV uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        v += __shfl_xor(v, off);
    }
    return v;
}

// Counters 2-7 from wave sums: density lookups, NEE lookups (= scatter events), capped paths as the algorithm counts them,
// and the march / shadow-volume fetches the wave issued (ct_fetch_counters).
CT_DEV void flush_counters(const BatchArgs &ba, uint32_t lane, uint32_t n_dl, uint32_t n_il, uint32_t n_cap, uint32_t n_fetch, uint32_t n_nee)
{
    if (lane == 0) {
        atomicAdd(&ba.counters[2], (unsigned long long)n_dl);
        atomicAdd(&ba.counters[3], (unsigned long long)n_il);
        atomicAdd(&ba.counters[4], (unsigned long long)n_il); // scatter events == NEE lookups
        atomicAdd(&ba.counters[5], (unsigned long long)n_cap);
        atomicAdd(&ba.counters[6], (unsigned long long)n_fetch);
        atomicAdd(&ba.counters[7], (unsigned long long)n_nee);
    }
}
