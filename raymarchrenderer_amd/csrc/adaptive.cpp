// adaptive.cpp — see adaptive.hpp. HIP-free.
#include "adaptive.hpp"

#include <cmath>

namespace rmr {

bool adaptive_params_ok(const rmr_adaptive_params& p) {
    return std::isfinite(p.threshold) && p.threshold >= 0.0f && std::isfinite(p.offset) && p.offset > 0.0f &&
           p.min_samples >= 2u && p.pass_samples >= 1u && p.max_samples >= p.min_samples && p.block_tiles >= 1 &&
           p.block_tiles <= 8;
}

int adaptive_select(const float* err, int tx, int ty, int block_tiles, float threshold, uint8_t* open) {
    const int bx = adaptive_blocks(tx, block_tiles), by = adaptive_blocks(ty, block_tiles);
    int n_open = 0;
    for (int j = 0; j < by; j++)
        for (int i = 0; i < bx; i++) {
            uint8_t& o = open[(size_t)j * bx + i];
            if (!o) continue;
            bool above = false;
            for (int y = j * block_tiles; y < ty && y < (j + 1) * block_tiles; y++)
                for (int x = i * block_tiles; x < tx && x < (i + 1) * block_tiles; x++)
                    above = above || err[(size_t)y * tx + x] > threshold;
            o = above ? 1 : 0;
            n_open += above ? 1 : 0;
        }
    return n_open;
}

std::vector<int32_t> adaptive_tiles(const uint8_t* open, int tx, int ty, int block_tiles) {
    const int bx = adaptive_blocks(tx, block_tiles);
    std::vector<int32_t> t;
    for (int y = 0; y < ty; y++)
        for (int x = 0; x < tx; x++)
            if (open[(size_t)(y / block_tiles) * bx + x / block_tiles]) {
                t.push_back(8 * x);
                t.push_back(8 * y);
            }
    return t;
}

}  // namespace rmr

extern "C" {

void rmr_default_adaptive_params(rmr_adaptive_params* p) {
    if (!p) return;
    p->threshold = 0.1f;
    p->offset = 1e-4f;
    p->min_samples = 16;
    p->pass_samples = 16;
    p->max_samples = 0;   // no default: the length of the caller's times[]
    p->block_tiles = 2;
}

int rmr_check_adaptive_params(const rmr_adaptive_params* p) {
    return p && rmr::adaptive_params_ok(*p) ? RMR_OK : RMR_E_INVALID;
}

int rmr_adaptive_select(const float* err, int tx, int ty, int block_tiles, float threshold, uint8_t* open_io) {
    if (!err || !open_io || tx <= 0 || ty <= 0 || tx > 4096 || ty > 4096 || block_tiles < 1 || block_tiles > 8 ||
        !std::isfinite(threshold) || threshold < 0.0f)
        return RMR_E_INVALID;
    return rmr::adaptive_select(err, tx, ty, block_tiles, threshold, open_io);
}

}  // extern "C"
