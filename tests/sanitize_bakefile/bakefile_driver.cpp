// The bake file parser (deepestscatter_amd/csrc/ct_bakefile.hpp) under AddressSanitizer and UBSan, stand-alone: valid files of
// every kind and format, then seeded mutations of them -- byte flips, truncations, enlarged counts with the checksum put right
// -- each of which must be accepted with a consistent info or refused with CT_E_INVAL.  Prints "ok <inputs> <accepted>".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../deepestscatter_amd/csrc/ct_bakefile.hpp"

using namespace ct;

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

static void seal(std::vector<uint8_t> &f)
{
    const uint64_t sum = fnv1a64(f.data(), f.size() - 8u);
    std::memcpy(f.data() + f.size() - 8u, &sum, 8);
}

static std::vector<uint8_t> make(uint32_t kind, uint32_t format, bool traced, bool adaptive)
{
    CtBakeFileInfo fi{};
    CtBakeFileHeader &hd = fi.header;
    std::memcpy(hd.magic, CT_BAKE_FILE_MAGIC, 8);
    hd.version = CT_BAKE_FILE_VERSION;
    hd.header_bytes = sizeof hd;
    hd.kind = kind;
    hd.format = format;
    hd.traced = traced;
    hd.adaptive = adaptive;
    hd.grid[0] = 5, hd.grid[1] = 4, hd.grid[2] = 3;
    hd.azimuths = 4;
    hd.cosines = 3;
    const uint64_t nodes = 60, block = 12, active = kind == CT_BAKE_DENSE ? nodes : 23;
    hd.margin_texels = kind == CT_BAKE_DENSE ? 0u : 4u;
    hd.entries = nodes * block;
    hd.active_nodes = active;
    hd.stored_entries = kind == CT_BAKE_COMPACT ? (active + 1u) * block : hd.entries;
    hd.dims[0] = hd.dims[1] = hd.dims[2] = 32;
    hd.sample_step_bits = float_bits(1.f / 512.f);
    hd.estimator = CT_EST_DELTA;
    if (traced) {
        hd.samples = 8;
        hd.paths = 8u * active * block;
    }
    if (adaptive) {
        hd.round_samples = 4;
        hd.max_samples = 8;
        hd.zero_samples = 100000;
        hd.rel_tol_bits = float_bits(0.7f);
        hd.abs_tol_bits = float_bits(1e-4f);
        hd.rounds = 2;
        hd.capped = 17;
        hd.converged = active * block - 17u;
    }
    bakefile_layout(&fi);
    std::vector<uint8_t> f((size_t)fi.file_bytes, 0);
    std::memcpy(f.data(), &hd, sizeof hd);
    if (fi.nodes_offset) {
        for (uint64_t i = 0; i < active; i++) {
            f[fi.nodes_offset + (i * 2u) % nodes + (i * 2u >= nodes ? 1u : 0u)] = 1;
        }
    }
    for (uint64_t i = fi.table_offset; i < (fi.m2_offset ? fi.m2_offset : fi.checksum_offset) - 16u; i++) {
        f[i] = (uint8_t)rnd();
    }
    seal(f);
    return f;
}

// 0: refused with CT_E_INVAL and a message; 1: accepted, and the info describes exactly these bytes.  Anything else aborts.
static int feed(const std::vector<uint8_t> &f)
{
    // (a copy of exactly f.size() bytes on the heap: one byte too far is the sanitizer's to see)
    uint8_t *exact = (uint8_t *)std::malloc(f.size() ? f.size() : 1u);
    std::memcpy(exact, f.data(), f.size());
    CtBakeFileInfo fi;
    BakeFileError err;
    const int rc = bakefile_parse(exact, f.size(), &fi, err);
    bool fine;
    if (rc == CT_OK) {
        CtBakeFileInfo again{};
        again.header = fi.header;
        bakefile_layout(&again);
        BakeFileError none;
        fine = fi.file_bytes == f.size() && again.file_bytes == fi.file_bytes && again.table_offset == fi.table_offset &&
               fi.checksum_offset + 8u == fi.file_bytes && fi.checksum == fnv1a64(exact, (size_t)fi.checksum_offset) &&
               bakefile_check_header(fi.header, none) == CT_OK && std::memcmp(&fi.header, exact, sizeof fi.header) == 0 &&
               fi.table_offset + fi.header.stored_entries * (fi.header.format ? 2u : 4u) <= fi.checksum_offset;
    } else {
        fine = rc == CT_E_INVAL && err.text[0] != 0;
    }
    std::free(exact);
    if (!fine) {
        std::fprintf(stderr, "inconsistent answer %d (%s) for a file of %zu bytes\n", rc, err.text, f.size());
        std::abort();
    }
    return rc == CT_OK ? 1 : 0;
}

int main()
{
    std::vector<std::vector<uint8_t>> valid;
    for (uint32_t kind = 0; kind < 3u; kind++) {
        for (uint32_t format = 0; format < 2u; format++) {
            valid.push_back(make(kind, format, false, false));
            valid.push_back(make(kind, format, true, false));
        }
        valid.push_back(make(kind, CT_BAKE_F32, true, true));
    }
    unsigned long inputs = 0, accepted = 0;
    for (const auto &f : valid) {
        inputs++;
        if (feed(f) != 1) {
            std::fprintf(stderr, "valid file %lu refused\n", inputs);
            return 1;
        }
        accepted++;
    }
    for (uint32_t round = 0; round < 4500u; round++) {
        std::vector<uint8_t> f = valid[rnd() % valid.size()];
        switch (rnd() % 6u) {
        case 0:   // a flipped byte anywhere
            f[rnd() % f.size()] ^= (uint8_t)(1u << (rnd() % 8u));
            break;
        case 1:   // truncated anywhere, to nothing included
            f.resize(rnd() % f.size());
            break;
        case 2: { // a header word replaced, the checksum put right: only the ranges stand in the way
            const uint32_t v = (rnd() & 1u) ? (uint32_t)rnd() : (uint32_t)(rnd() % 300u);
            std::memcpy(f.data() + 4u * (rnd() % 64u), &v, 4);
            seal(f);
            break;
        }
        case 3: { // an enlarged count (entries, stored_entries, active_nodes), sealed
            const uint64_t v = (rnd() & 1u) ? rnd() : (uint64_t)1 << (rnd() % 40u);
            std::memcpy(f.data() + 56u + 8u * (rnd() % 3u), &v, 8);
            seal(f);
            break;
        }
        case 4:   // a flipped payload byte, sealed: node bytes and gaps
            f[256u + rnd() % (f.size() - 264u)] ^= (uint8_t)(1u << (rnd() % 8u));
            seal(f);
            break;
        default:  // grown by garbage
            for (uint64_t n = 1u + rnd() % 64u; n != 0u; n--) {
                f.push_back((uint8_t)rnd());
            }
            if (rnd() & 1u) {
                seal(f);
            }
            break;
        }
        inputs++;
        accepted += (unsigned long)feed(f);
    }
    std::printf("ok %lu %lu\n", inputs, accepted);
    return 0;
}
