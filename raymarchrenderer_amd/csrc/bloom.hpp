// bloom.hpp — the host's part of the HDR bloom stage (rmr_bloom.hip): the parameter
// ranges and the level sizes of the pyramid. No HIP.
#pragma once
#include <stddef.h>

#include "rmr_bloom_rule.h"

namespace rmr {

bool bloom_params_ok(const rmr_bloom_params& p);

// The pyramid of a W x H image: level k = 1..levels is w[k] x h[k] float4 at off[k] (in float4) of one
// allocation of `total` float4; w[0] x h[0] is the image itself.
struct BloomLevels {
    int w[kBloomMaxLevels + 1], h[kBloomMaxLevels + 1];
    size_t off[kBloomMaxLevels + 1];
    size_t total;
};
BloomLevels bloom_levels(int W, int H, int levels);

}  // namespace rmr
