// tonemap.hpp — the host's part of the tone-mapping stage (rmr_tonemap.hip): the
// parameter ranges and the constants the kernels take from the host. No HIP.
#pragma once
#include "rmr_tonemap_rule.h"

namespace rmr {

bool tonemap_params_ok(const rmr_tonemap_params& p);
// lc[b - 1] = e + log2(1 + (m + 0.5) / 8), e = (b >> 3) - 16, m = b & 7, for b = 1..255
void tonemap_lc_table(double lc[255]);
ToneMeter tonemap_meter(const rmr_tonemap_params& p);
// (float)(1 / ((double)white * white))
float tonemap_iw2(const rmr_tonemap_params& p);

}  // namespace rmr
