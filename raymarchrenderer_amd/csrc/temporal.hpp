// temporal.hpp — the host's part of the temporal reprojection stage (rmr_temporal.hip; DESIGN.md
// §4.12): the parameter ranges and the inverse of the history view's ray basis. No HIP.
#pragma once
#include "../../include/rmr.h"

namespace rmr {

bool temporal_params_ok(const rmr_temporal_params& p);

// view: eye, r00, r01, r10, r11 (shader order). With a = r01 - r00, b = r10 - r00 and
// c = (r11 - r10) - (r01 - r00), all in double from the float values: out[0..8] = [a | b | r00]^-1
// row-major, out[9..11] = that inverse times c. False for a view that is not finite, has a zero corner
// ray, or whose |det [a | b | r00]| <= 1e-9 |a| |b| |r00|.
bool temporal_view_inverse(const float view[15], double out[12]);

}  // namespace rmr
