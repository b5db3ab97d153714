// ct_bake_group.hpp -- the seam between ct_bake.cpp (the bakes) and ct_group.hip (ct_group_bake_*): a bake that
// builds one shard's span of the node list, the checks a group call passes through from shard 0 before any shard works, and the
// exchange that leaves every shard with the complete bake.  Private; only the C ABI's types.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/cloudtrace.h"

namespace ct {

// ct_network_bake* (n), ct_bake_traced (samples) or ct_bake_traced_adaptive (p) of `kind` on h, cut for shard `shard` of `shards`:
// only the span is baked or traced.  The arguments are checked as the single-GPU calls check them.
int bake_create_shard(CtHandle h, CtNetwork n, const CtBakeDesc *d, uint32_t kind, const uint32_t *samples, const CtBakeAdaptive *p,
                      uint32_t shard, uint32_t shards, CtBake *out);
// A loaded bake, complete, cut for what follows.
int bake_cut_shard(CtBake b, uint32_t shard, uint32_t shards);
void bake_shard_span(CtBake b, uint64_t lo_hi_out[2]);

// The checks of the single-GPU call, up to but not including its first change: nothing of the handle or the bake is touched.
enum BakeOp { BAKE_OP_UPDATE, BAKE_OP_TRACE_MORE, BAKE_OP_RETRACE, BAKE_OP_ADAPTIVE_MORE, BAKE_OP_RETRACE_ADAPTIVE };
int bake_op_checks(CtHandle h, CtNetwork n, CtBake b, BakeOp op, uint32_t arg);

// Every shard has built or continued its span of bakes[0 .. count) and is idle.  Every shard's range of the table (an adaptive
// bake: of m2 and counts too) goes to every other shard -- a peer copy across devices, a plain one within a device -- the
// survivors' lists are concatenated in shard order into every shard's live list, and every shard gets the scalars of the whole:
// samples and rounds the maximum, live the sum, paths = paths_before + the sum of what the shards added to it, the millisecond
// fields the slowest shard's.  *bytes_out: what was copied between shards.  A failure's text goes to error.
int bake_exchange(CtBake const *bakes, uint32_t count, uint64_t paths_before, uint64_t *bytes_out, char *error, size_t error_bytes);

} // namespace ct
