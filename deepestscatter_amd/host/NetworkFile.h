// NetworkFile.h -- the weight file of `cloudtrace --network` (written by deepestscatter_amd/network.py, save_weights):
// a 32-byte little-endian header -- magic "CTNW", u32 version (1), u32 blocks, width, aux, head_layers, u64 weight count --
// followed by weight_count float32 values in the order of CtNetworkDesc::weights_host (include/cloudtrace.h).
// Pure host code: a file is read and checked against the formula of the header before any device is touched.
#pragma once

#include <cstdint>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

namespace DeepestScatter
{
    struct NetworkFile
    {
        uint32_t blocks = 0, width = 0, aux = 0, headLayers = 0;
        std::vector<float> weights;

        // Wd (225 + A) + 9 Wd (Wd + 225 + A) + 10 (Wd Wd + 2 Wd) + (H - 1)(Wd Wd + Wd) + Wd + 1
        static uint64_t weightCount(uint64_t w, uint64_t a, uint64_t h)
        {
            return w * (225 + a) + 9 * w * (w + 225 + a) + 10 * (w * w + 2 * w) + (h - 1) * (w * w + w) + w + 1;
        }

        static NetworkFile load(const std::string& path)
        {
            std::ifstream f(path, std::ios::binary | std::ios::ate);
            if (!f) throw std::runtime_error("cannot open network file " + path);
            const uint64_t size = (uint64_t)f.tellg();
            f.seekg(0);
            unsigned char head[32];
            if (size < sizeof head || !f.read(reinterpret_cast<char*>(head), sizeof head))
                throw std::runtime_error(path + ": shorter than the 32-byte header of a network file");
            const auto u32 = [&](size_t at) { return (uint32_t)head[at] | (uint32_t)head[at + 1] << 8 | (uint32_t)head[at + 2] << 16 | (uint32_t)head[at + 3] << 24; };
            if (std::memcmp(head, "CTNW", 4) != 0) throw std::runtime_error(path + ": not a network file (wrong magic)");
            if (u32(4) != 1u) throw std::runtime_error(path + ": network file version " + std::to_string(u32(4)) + ", this reader knows 1");
            NetworkFile n;
            n.blocks = u32(8); n.width = u32(12); n.aux = u32(16); n.headLayers = u32(20);
            const uint64_t count = (uint64_t)u32(24) | (uint64_t)u32(28) << 32;
            if (n.blocks != 10 || n.width < 16 || n.width > 256 || n.width % 8 != 0 || n.aux > 8 || n.headLayers < 1 || n.headLayers > 4)
                throw std::runtime_error(path + ": network shapes out of range");
            if (count != weightCount(n.width, n.aux, n.headLayers))
                throw std::runtime_error(path + ": " + std::to_string(count) + " weights, the shapes imply " + std::to_string(weightCount(n.width, n.aux, n.headLayers)));
            if (size - sizeof head != 4 * count)
                throw std::runtime_error(path + ": " + std::to_string(size - sizeof head) + " bytes of weights, " + std::to_string(count) + " weights need " + std::to_string(4 * count));
            std::vector<unsigned char> raw(4 * count);
            if (!f.read(reinterpret_cast<char*>(raw.data()), (std::streamsize)raw.size())) throw std::runtime_error(path + ": short read");
            n.weights.resize(count);
            for (uint64_t i = 0; i < count; i++)
            {
                const uint32_t bits = (uint32_t)raw[4 * i] | (uint32_t)raw[4 * i + 1] << 8 | (uint32_t)raw[4 * i + 2] << 16 | (uint32_t)raw[4 * i + 3] << 24;
                std::memcpy(&n.weights[i], &bits, sizeof bits);
            }
            return n;
        }
    };
}
