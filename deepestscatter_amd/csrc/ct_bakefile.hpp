// ct_bakefile.hpp -- the bake file of include/cloudtrace.h, "bake files": its layout, checksum, parser and validator, and the
// float32 -> binary16 rounding of "half tables".  Device-free like ct_plan.hpp: it depends on the C ABI's types and the C++
// standard library only, so ct_bake_file_info and tests/sanitize_bakefile compile it without HIP.  The parser reads untrusted
// bytes: every offset it forms is checked against the length first, and nothing is read through the header's own counts
// before they are inside the ABI's ranges.
#pragma once

#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/cloudtrace.h"

#if defined(__HIPCC__)
#define CT_BAKEFILE_HD __host__ __device__
#else
#define CT_BAKEFILE_HD
#endif

namespace ct {

static_assert(sizeof(CtBakeFileHeader) == 256, "the bake file's header is 256 packed bytes");
static_assert(sizeof(CtBakeFileInfo) == 312, "CtBakeFileInfo");

// float32 bits -> binary16 bits: the nearest value, ties to even, subnormals included, the sign of zero kept; an infinity for
// |v| >= 65520 and for an infinity, a quiet NaN for a NaN.  In integers: no rounding or denormal mode can change it.
CT_BAKEFILE_HD inline uint16_t half_round_bits(uint32_t f)
{
    const uint32_t sign = (f >> 16) & 0x8000u, a = f & 0x7fffffffu;
    if (a > 0x7f800000u) {
        return (uint16_t)(sign | 0x7e00u);
    }
    if (a >= 0x477ff000u) {   // 65520 = the tie between 65504 and 2^16, which goes to the even 2^16: an infinity
        return (uint16_t)(sign | 0x7c00u);
    }
    if (a >= 0x38800000u) {   // >= 2^-14: a normal binary16
        uint32_t r = a - 0x38000000u;
        r += 0xfffu + ((r >> 13) & 1u);
        return (uint16_t)(sign | (r >> 13));
    }
    const uint32_t e = a >> 23;
    if (e < 102u) {           // < 2^-25: nearer to zero than to the smallest subnormal
        return (uint16_t)sign;
    }
    const uint32_t m = (a & 0x7fffffu) | 0x800000u, shift = 126u - e;   // units of 2^-24: m >> shift, shift 14 .. 24
    uint32_t q = m >> shift;
    const uint32_t rem = m & ((1u << shift) - 1u), tie = 1u << (shift - 1u);
    if (rem > tie || (rem == tie && (q & 1u))) {
        q++;
    }
    return (uint16_t)(sign | q);
}

// Does half_round_bits give an infinity or a NaN for these bits?  (ct_bake_half's refusal rule.)
CT_BAKEFILE_HD inline bool half_refused(uint32_t f)
{
    return (f & 0x7fffffffu) >= 0x477ff000u;
}

// binary16 bits -> the float32 of the same value (exact).
inline float half_widen(uint16_t hbits)
{
    const uint32_t sign = (uint32_t)(hbits & 0x8000u) << 16, e = (hbits >> 10) & 31u, m = hbits & 0x3ffu;
    uint32_t f;
    if (e == 31u) {
        f = sign | 0x7f800000u | (m << 13);
    } else if (e != 0u) {
        f = sign | ((e + 112u) << 23) | (m << 13);
    } else if (m == 0u) {
        f = sign;
    } else {
        float v = (float)m * 5.9604644775390625e-8f;   // m * 2^-24, exact
        uint32_t bits;
        std::memcpy(&bits, &v, sizeof bits);
        f = sign | bits;
    }
    float out;
    std::memcpy(&out, &f, sizeof out);
    return out;
}

inline uint64_t fnv1a64(const uint8_t *p, size_t n, uint64_t hash = 0xCBF29CE484222325ull)
{
    for (size_t i = 0; i < n; i++) {
        hash = (hash ^ p[i]) * 0x100000001B3ull;
    }
    return hash;
}

// The volume hash on the host (the device reduces the same sum in another order).
inline uint64_t volume_hash(const uint8_t *texels, uint64_t count)
{
    uint64_t sum = 0;
    for (uint64_t i = 0; i < count; i++) {
        sum += ((uint64_t)texels[i] + 1u) * ((i + 1u) * 0x9E3779B97F4A7C15ull);
    }
    return sum;
}

inline float bits_float(uint32_t bits)
{
    float v;
    std::memcpy(&v, &bits, sizeof v);
    return v;
}

inline uint32_t float_bits(float v)
{
    uint32_t bits;
    std::memcpy(&bits, &v, sizeof bits);
    return bits;
}

struct BakeFileError {
    char text[256] = {};
    int set(const char *fmt, ...)
    {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(text, sizeof text, fmt, ap);
        va_end(ap);
        return CT_E_INVAL;
    }
};

// The header's own consistency: every range ct_network_bake, ct_bake_traced and ct_bake_traced_adaptive check, and the counts
// against each other.  Nothing of the payload is looked at.
inline int bakefile_check_header(const CtBakeFileHeader &hd, BakeFileError &err)
{
    if (std::memcmp(hd.magic, CT_BAKE_FILE_MAGIC, 8) != 0) {
        return err.set("not a bake file (wrong magic)");
    }
    if (hd.version != CT_BAKE_FILE_VERSION) {
        return err.set("bake file version %u, this library reads version %u", hd.version, CT_BAKE_FILE_VERSION);
    }
    if (hd.header_bytes != sizeof(CtBakeFileHeader)) {
        return err.set("a header of %u bytes, version %u has %zu", hd.header_bytes, CT_BAKE_FILE_VERSION, sizeof(CtBakeFileHeader));
    }
    if (hd.kind > (uint32_t)CT_BAKE_COMPACT) {
        return err.set("unknown kind %u", hd.kind);
    }
    if (hd.format > (uint32_t)CT_BAKE_F16) {
        return err.set("unknown format %u", hd.format);
    }
    if (hd.traced > 1u || hd.adaptive > 1u || hd.tex_fixed8 > 1u) {
        return err.set("traced, adaptive and tex_fixed8 are 0 or 1 (%u, %u, %u)", hd.traced, hd.adaptive, hd.tex_fixed8);
    }
    if (hd.adaptive && (!hd.traced || hd.format != (uint32_t)CT_BAKE_F32)) {
        return err.set("an adaptive bake is traced and float32");
    }
    uint64_t nodes = 1;
    for (int axis = 0; axis < 3; axis++) {
        if (hd.grid[axis] < 2u || hd.grid[axis] > 256u) {
            return err.set("grid[%d] = %u, a grid has 2 .. 256 nodes per axis", axis, hd.grid[axis]);
        }
        nodes *= hd.grid[axis];
    }
    if (hd.azimuths < 4u || hd.azimuths > 64u || hd.azimuths % 4u != 0u) {
        return err.set("%u azimuths; a multiple of 4 in 4 .. 64", hd.azimuths);
    }
    if (hd.cosines < 2u || hd.cosines > 64u) {
        return err.set("%u cosines; 2 .. 64", hd.cosines);
    }
    const uint64_t block = (uint64_t)hd.azimuths * hd.cosines, entries = nodes * block;   // (<= 2^36)
    if (hd.entries != entries) {
        return err.set("%llu entries, the grid has %llu", (unsigned long long)hd.entries, (unsigned long long)entries);
    }
    if (hd.kind == (uint32_t)CT_BAKE_DENSE ? hd.active_nodes != nodes : hd.active_nodes > nodes) {
        return err.set("%llu active nodes of %llu", (unsigned long long)hd.active_nodes, (unsigned long long)nodes);
    }
    if (hd.kind == (uint32_t)CT_BAKE_DENSE && hd.margin_texels != 0u) {
        return err.set("a dense bake has no margin (%u)", hd.margin_texels);
    }
    const uint64_t stored = hd.kind == (uint32_t)CT_BAKE_COMPACT ? (hd.active_nodes + 1u) * block : entries;
    if (hd.stored_entries != stored) {
        return err.set("%llu stored entries, kind %u with %llu active nodes stores %llu", (unsigned long long)hd.stored_entries, hd.kind,
                       (unsigned long long)hd.active_nodes, (unsigned long long)stored);
    }
    if (stored > (1ull << 26)) {
        return err.set("%llu stored entries, a table holds at most 2^26", (unsigned long long)stored);
    }
    for (int axis = 0; axis < 3; axis++) {
        if (hd.dims[axis] == 0u || hd.dims[axis] > 2048u) {
            return err.set("volume dims[%d] = %u", axis, hd.dims[axis]);
        }
    }
    if (hd.estimator != CT_EST_MARCH && hd.estimator != CT_EST_DELTA) {
        return err.set("unknown estimator %d", hd.estimator);
    }
    if (hd.samples > (1u << 24)) {
        return err.set("%u samples, an entry holds at most 2^24 experiments", hd.samples);
    }
    if (!hd.traced && (hd.samples != 0u || hd.paths != 0u)) {
        return err.set("a network's bake with samples or paths");
    }
    if (hd.adaptive) {
        const float rel = bits_float(hd.rel_tol_bits), abs_tol = bits_float(hd.abs_tol_bits);
        if (hd.round_samples == 0u || hd.round_samples > 0xffffu) {
            return err.set("round_samples %u, a round traces 1 .. 65535 experiments per entry", hd.round_samples);
        }
        if (hd.max_samples == 0u || hd.max_samples % hd.round_samples != 0u || hd.max_samples > (1u << 24)) {
            return err.set("max_samples %u; a multiple of round_samples (%u), at most 2^24", hd.max_samples, hd.round_samples);
        }
        if (!std::isfinite(rel) || !std::isfinite(abs_tol) || rel < 0.f || abs_tol < 0.f) {
            return err.set("rel_tol and abs_tol must be finite and not negative");
        }
        if ((uint64_t)hd.rounds * hd.round_samples != hd.samples || hd.samples > hd.max_samples) {
            return err.set("%u rounds of %u experiments, %u samples, a cap of %u", hd.rounds, hd.round_samples, hd.samples, hd.max_samples);
        }
        const uint64_t total = hd.active_nodes * block;
        if (hd.capped > total || hd.converged != (hd.rounds != 0u ? total - hd.capped : 0u)) {
            return err.set("%llu converged and %llu capped entries of %llu", (unsigned long long)hd.converged,
                           (unsigned long long)hd.capped, (unsigned long long)total);
        }
    } else if (hd.round_samples || hd.max_samples || hd.zero_samples || hd.rel_tol_bits || hd.abs_tol_bits || hd.rounds || hd.converged ||
               hd.capped) {
        return err.set("adaptive parameters in a bake that is not adaptive");
    }
    for (uint8_t byte : hd.reserved) {
        if (byte != 0u) {
            return err.set("non-zero reserved bytes");
        }
    }
    return CT_OK;
}

// The sections of a file with this (checked) header: out->header is set, the rest is filled in.
inline void bakefile_layout(CtBakeFileInfo *out)
{
    const CtBakeFileHeader &hd = out->header;
    const auto pad16 = [](uint64_t v) { return (v + 15u) & ~(uint64_t)15u; };
    uint64_t at = sizeof(CtBakeFileHeader);
    out->nodes_offset = out->m2_offset = out->counts_offset = 0;
    if (hd.kind != (uint32_t)CT_BAKE_DENSE) {
        out->nodes_offset = at = pad16(at);
        at += (uint64_t)hd.grid[0] * hd.grid[1] * hd.grid[2];
    }
    out->table_offset = at = pad16(at);
    at += hd.stored_entries * (hd.format == (uint32_t)CT_BAKE_F16 ? 2u : 4u);
    if (hd.adaptive) {
        out->m2_offset = at = pad16(at);
        at += hd.stored_entries * 4u;
        out->counts_offset = at = pad16(at);
        at += hd.stored_entries * 4u;
    }
    out->checksum_offset = at = (at + 7u) & ~(uint64_t)7u;
    out->file_bytes = at + 8u;
}

// A whole file in memory -> *out, or CT_E_INVAL with the reason in err.  In the order of include/cloudtrace.h: length of the
// fixed part, magic, version, ranges, the sections against the length, the gaps, the checksum, the node bytes.
inline int bakefile_parse(const uint8_t *data, size_t size, CtBakeFileInfo *out, BakeFileError &err)
{
    *out = CtBakeFileInfo{};
    if (size < sizeof(CtBakeFileHeader) + 8u) {
        return err.set("%zu bytes: shorter than a bake file's header and checksum", size);
    }
    std::memcpy(&out->header, data, sizeof(CtBakeFileHeader));
    const int rc = bakefile_check_header(out->header, err);
    if (rc != CT_OK) {
        return rc;
    }
    bakefile_layout(out);
    if (out->file_bytes != (uint64_t)size) {
        const char *part = "the file";
        const uint64_t len = size;
        if (len > out->file_bytes) {
            part = "bytes behind the checksum";
        } else if (len < out->table_offset) {
            part = "the node bytes";
        } else if (len < (out->m2_offset ? out->m2_offset : out->checksum_offset)) {
            part = "the table";
        } else if (out->m2_offset && len < out->counts_offset) {
            part = "m2";
        } else if (out->m2_offset && len < out->checksum_offset) {
            part = "the counts";
        } else {
            part = "the checksum";
        }
        return err.set("%llu bytes, the header implies %llu: truncated in %s", (unsigned long long)len, (unsigned long long)out->file_bytes, part);
    }
    std::memcpy(&out->checksum, data + out->checksum_offset, 8);
    const uint64_t sum = fnv1a64(data, (size_t)out->checksum_offset);
    if (sum != out->checksum) {
        return err.set("checksum %016llx, the bytes give %016llx", (unsigned long long)out->checksum, (unsigned long long)sum);
    }
    {   // the gaps in front of the sections and the checksum are zero: a file is determined by what it holds
        const CtBakeFileHeader &hd = out->header;
        const uint64_t nodes = (uint64_t)hd.grid[0] * hd.grid[1] * hd.grid[2], value = hd.format == (uint32_t)CT_BAKE_F16 ? 2u : 4u;
        const uint64_t gaps[4][2] = {
            { out->nodes_offset ? out->nodes_offset + nodes : out->table_offset, out->table_offset },
            { out->table_offset + hd.stored_entries * value, out->m2_offset ? out->m2_offset : out->checksum_offset },
            { out->m2_offset ? out->m2_offset + hd.stored_entries * 4u : out->checksum_offset, out->m2_offset ? out->counts_offset : out->checksum_offset },
            { out->counts_offset ? out->counts_offset + hd.stored_entries * 4u : out->checksum_offset, out->checksum_offset },
        };
        for (const auto &gap : gaps) {
            for (uint64_t i = gap[0]; i < gap[1]; i++) {
                if (data[i] != 0u) {
                    return err.set("byte %llu, in a gap between two sections, is not zero", (unsigned long long)i);
                }
            }
        }
    }
    if (out->nodes_offset) {
        const uint64_t nodes = (uint64_t)out->header.grid[0] * out->header.grid[1] * out->header.grid[2];
        uint64_t ones = 0;
        for (uint64_t i = 0; i < nodes; i++) {
            const uint8_t v = data[out->nodes_offset + i];
            if (v > 1u) {
                return err.set("node byte %llu is %u, not 0 or 1", (unsigned long long)i, v);
            }
            ones += v;
        }
        if (ones != out->header.active_nodes) {
            return err.set("%llu node bytes are set, the header counts %llu active nodes (and sizes stored_entries by them)",
                           (unsigned long long)ones, (unsigned long long)out->header.active_nodes);
        }
    }
    return CT_OK;
}

} // namespace ct
