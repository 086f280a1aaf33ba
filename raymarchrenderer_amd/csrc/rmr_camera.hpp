// rmr_camera.hpp — camera models and caller-supplied rays: what the host works out without a GPU
// (camera.cpp: no HIP, no context, like adaptive.cpp) and the generator kernel's argument.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/rmr.h"

namespace rmr {

// k_camera_rays' second argument (rmr_camera.hip): the model, its four floats (aperture, focus, width,
// height) and the camera frame of rmr_camera_frame
struct CamParams {
    int32_t model;
    float p[4];
    float U[3], V[3], F[3];
};

// bytes of a unit's ray record on the device (rmr_trace.h kRayRecord float4: origin and time, direction
// and chain state, seeds and the "no ray" mark)
constexpr size_t kRayRecordBytes = 48;

bool camera_model_ok(const rmr_camera_model& m);
// U, V, FWD of a view (eye, r00, r01, r10, r11) in double, rounded to float; false for a degenerate view
bool camera_frame(const float view[15], float out[9]);
// index of the first bad ray, or -1 (rmr_check_rays)
long long first_bad_ray(const rmr_ray* rays, size_t n);
// the largest |coordinate| an origin of the model's rays can have (the escape boxes' inflation,
// accel.hpp escape_inflation, takes it in the eye's place)
double camera_origin_extent(const rmr_camera_model& m, const float eye[3]);

}  // namespace rmr
