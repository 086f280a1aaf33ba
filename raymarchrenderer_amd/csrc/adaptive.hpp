// adaptive.hpp — the host side of adaptive sampling that needs no GPU (adaptive.cpp):
// the parameter ranges, the decision rule over the tile errors and the tile list of the open blocks.
// No HIP, no context: rmr_api.cpp's loop calls these between launches, the tests without a device.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/rmr.h"

namespace rmr {

// The ranges of rmr_adaptive_params (rmr.h).
bool adaptive_params_ok(const rmr_adaptive_params& p);

// Decision blocks per axis for `tiles` 8x8 tiles of that axis.
inline int adaptive_blocks(int tiles, int block_tiles) { return (tiles + block_tiles - 1) / block_tiles; }

// The decision rule: err is ty x tx tile errors, open ceil(ty / bt) x ceil(tx / bt) bytes (non-zero:
// open). An open block stays open iff one of its tiles has an error > threshold (the block's maximum,
// whatever the order; a NaN error is not above any threshold); a closed block stays closed. Returns the
// number of blocks still open.
int adaptive_select(const float* err, int tx, int ty, int block_tiles, float threshold, uint8_t* open);

// The 8x8 tiles of the open blocks, row-major: the pixel origin (x, y) of each, two values per tile.
std::vector<int32_t> adaptive_tiles(const uint8_t* open, int tx, int ty, int block_tiles);

}  // namespace rmr
