// camera.cpp — the host side of the camera models and ray lists that needs no GPU: range checks, the
// camera frame of a view, the checks of a caller's rays (rmr_camera.hpp). No HIP, no context.
#include "rmr_camera.hpp"
#include "rmr_ray_check.h"

#include <algorithm>
#include <cmath>

namespace rmr {

bool camera_model_ok(const rmr_camera_model& m) {
    switch (m.model) {
    case RMR_CAMERA_VIEW:
    case RMR_CAMERA_EQUIRECT:
        return true;
    case RMR_CAMERA_THIN_LENS:
        return std::isfinite(m.aperture) && m.aperture >= 0.0f && std::isfinite(m.focus) && m.focus > 0.0f;
    case RMR_CAMERA_ORTHO:
        return std::isfinite(m.width) && m.width > 0.0f && std::isfinite(m.height) && m.height > 0.0f;
    default:
        return false;
    }
}

namespace {
double dot3(const double a[3], const double b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
// a / |a|; false unless 0 < |a| < inf, and unless |a| > rel (what is left of a vector of length rel
// after the projections: below 1e-9 of it the direction is rounding noise)
bool unit3(double a[3], double rel) {
    const double l = std::sqrt(dot3(a, a));
    if (!std::isfinite(l) || !(l > 0.0) || !(l > 1e-9 * rel)) return false;
    for (int k = 0; k < 3; k++) a[k] /= l;
    return true;
}
}  // namespace

bool camera_frame(const float view[15], float out[9]) {
    for (int i = 0; i < 15; i++)
        if (!std::isfinite(view[i])) return false;
    const float *r00 = view + 3, *r01 = view + 6, *r10 = view + 9, *r11 = view + 12;
    double U[3], V[3], F[3];
    for (int k = 0; k < 3; k++) {
        U[k] = (double)r01[k] - (double)r00[k];
        V[k] = (double)r10[k] - (double)r00[k];
        F[k] = (((double)r00[k] + (double)r01[k]) + (double)r10[k]) + (double)r11[k];
    }
    const double lv = std::sqrt(dot3(V, V)), lf = std::sqrt(dot3(F, F));
    if (!unit3(U, 0.0)) return false;
    const double vu = dot3(V, U);
    for (int k = 0; k < 3; k++) V[k] -= vu * U[k];
    if (!unit3(V, lv)) return false;
    const double fu = dot3(F, U), fv = dot3(F, V);
    for (int k = 0; k < 3; k++) F[k] = (F[k] - fu * U[k]) - fv * V[k];
    if (!unit3(F, lf)) return false;
    for (int k = 0; k < 3; k++) {
        out[k] = (float)U[k];
        out[3 + k] = (float)V[k];
        out[6 + k] = (float)F[k];
    }
    return true;
}

long long first_bad_ray(const rmr_ray* rays, size_t n) {
    for (size_t i = 0; i < n; i++)
        if (!ray_ok(rays[i])) return (long long)i;   // (rmr_ray_check.h: the rule the kernels apply too)
    return -1;
}

double camera_origin_extent(const rmr_camera_model& m, const float eye[3]) {
    double e = 0.0;
    for (int k = 0; k < 3; k++) e = std::max(e, std::fabs((double)eye[k]));
    if (m.model == RMR_CAMERA_THIN_LENS) e += 2.0 * (double)m.aperture;   // |lx U + ly V|_inf <= |lx| + |ly| <= 2
    // |u - 1/2|, |v - 1/2| <= 1/2 up to float rounding
    if (m.model == RMR_CAMERA_ORTHO) e += 0.501 * ((double)m.width + (double)m.height);
    return e;
}

}  // namespace rmr

extern "C" {

void rmr_default_camera_model(rmr_camera_model* m) {
    if (!m) return;
    m->model = RMR_CAMERA_VIEW;
    m->aperture = 0.0f;
    m->focus = 1.0f;
    m->width = 1.0f;
    m->height = 1.0f;
}

int rmr_check_camera_model(const rmr_camera_model* m) {
    return (m && rmr::camera_model_ok(*m)) ? RMR_OK : RMR_E_INVALID;
}

int rmr_camera_frame(const float view[15], float out[9]) {
    if (!view || !out) return RMR_E_INVALID;
    return rmr::camera_frame(view, out) ? RMR_OK : RMR_E_INVALID;
}

int rmr_check_rays(const rmr_ray* rays, size_t n) {
    if (!rays && n) return RMR_E_INVALID;
    return rmr::first_bad_ray(rays, n) < 0 ? RMR_OK : RMR_E_INVALID;
}

}  // extern "C"
