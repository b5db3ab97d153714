// ct_bake.hpp -- the seam between ct_neural.cpp (pyramid, descriptors, network, renderer) and ct_bake.cpp (the bakes): what the
// renderer needs of a bake, and what a bake needs of the network path.  Private, like ct_handle.hpp.
#pragma once

#include "ct_handle.hpp"

namespace ct {

// ---- ct_bake.cpp, for the renderer (CtBake_ stays incomplete there) -----------------------------------------------------------
// A bake that belongs to h and holds h's light: CT_E_INVAL / CT_E_STATE otherwise.
int bake_foreign(CtHandle h, CtBake b, const char *who);
int bake_stale(CtHandle h, CtBake b, const char *who);
BakeTable bake_table(const CtBake_ *b);

// ---- ct_neural.cpp, for the bake ----------------------------------------------------------------------------------------------
// VDBCloud::getVoxelSizeInMeters / getVoxelSizeInTermsOfFreePath (VDBCloud.cpp:35-46), DisneyDescriptor.cuh:83
struct DescriptorScale {
    float level0, voxel_m;
};
DescriptorScale descriptor_scale(CtHandle h);
int net_validate_network(CtHandle h, CtNetwork n, const char *who);
// Records the descriptor array may hold at most: 2^20 (a band has no more), or CT_NET_DESC_RECORDS.
size_t net_descriptor_limit(CtHandle h);
// Everything a call needs before its first kernel: the band-sized temporaries and a first piece of the descriptor array.  The
// stream is idle.  A failed growth leaves what the handle had.  direct: the call carries CT_NET_ADD_SINGLE_SCATTER.
int net_reserve(CtHandle h, size_t band_pixels, bool direct, bool hybrid = false);
// The descriptor array follows the largest record count seen.  Between bands, the stream idle.  When the device has no room
// for it the array stays as it is and the band's records are gathered and evaluated in pieces of its size.
void net_grow_descriptors(CtHandle h, size_t count);

// Runs `body`; when it fails, what it has enqueued is waited for before the call returns.
template <typename F>
int drained(CtHandle h, F &&body)
{
    const int rc = body();
    if (rc != CT_OK) {
        hipStreamSynchronize(h->stream);
    }
    return rc;
}

// `launches` between the handle's first two events, waited for; *ms_sum grows by their GPU time.  count_dev: a count the
// launches leave on the device, read into *count_out behind them (the one 4-byte read of a band, a frame or a mask).
template <typename F>
int timed(CtHandle h, double *ms_sum, F &&launches, const uint32_t *count_dev = nullptr, uint32_t *count_out = nullptr)
{
    HIPCHK(h, hipEventRecord(h->ev[0], h->stream));
    const int rc = launches();
    if (rc != CT_OK) {
        return rc;
    }
    HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
    if (count_dev) {
        HIPCHK(h, hipMemcpyAsync(count_out, count_dev, sizeof *count_out, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    } else {
        HIPCHK(h, hipEventSynchronize(h->ev[1]));
    }
    float ms = 0;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
    *ms_sum += ms;
    return CT_OK;
}

} // namespace ct
