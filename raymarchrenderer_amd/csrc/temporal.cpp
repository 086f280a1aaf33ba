// temporal.cpp — see temporal.hpp. No HIP: built into librmr.so and, with temporal_test.cpp, into a
// stand-alone CPU check (plain and under the sanitizers).
#include "temporal.hpp"

#include <cmath>

namespace rmr {

bool temporal_params_ok(const rmr_temporal_params& p) {
    return std::isfinite(p.max_history) && p.max_history >= 1.0f && std::isfinite(p.sigma_z) && p.sigma_z > 0.0f &&
           p.normal_pow2 >= 0 && p.normal_pow2 <= 7;
}

bool temporal_view_inverse(const float view[15], double out[12]) {
    for (int i = 0; i < 15; i++)
        if (!std::isfinite(view[i])) return false;
    double r[4][3];   // r00, r01, r10, r11
    for (int k = 0; k < 4; k++) {
        double n2 = 0.0;
        for (int i = 0; i < 3; i++) {
            r[k][i] = (double)view[3 + 3 * k + i];
            n2 += r[k][i] * r[k][i];
        }
        if (n2 == 0.0) return false;
    }
    double a[3], b[3], c[3];
    for (int i = 0; i < 3; i++) {
        a[i] = r[1][i] - r[0][i];
        b[i] = r[2][i] - r[0][i];
        c[i] = (r[3][i] - r[2][i]) - a[i];
    }
    const double* z = r[0];
    auto cross = [](const double* p, const double* q, double* o) {
        o[0] = p[1] * q[2] - p[2] * q[1];
        o[1] = p[2] * q[0] - p[0] * q[2];
        o[2] = p[0] * q[1] - p[1] * q[0];
    };
    auto dot = [](const double* p, const double* q) { return p[0] * q[0] + p[1] * q[1] + p[2] * q[2]; };
    // the rows of [a | b | z]^-1 are (b x z, z x a, a x b) / det, det = a . (b x z)
    double bz[3], za[3], ab[3];
    cross(b, z, bz);
    cross(z, a, za);
    cross(a, b, ab);
    const double det = dot(a, bz);
    const double scale = std::sqrt(dot(a, a) * dot(b, b) * dot(z, z));
    if (!std::isfinite(det) || !(std::fabs(det) > 1e-9 * scale)) return false;
    for (int i = 0; i < 3; i++) {
        out[i] = bz[i] / det;
        out[3 + i] = za[i] / det;
        out[6 + i] = ab[i] / det;
    }
    for (int k = 0; k < 3; k++) out[9 + k] = dot(out + 3 * k, c);
    for (int i = 0; i < 12; i++)
        if (!std::isfinite(out[i])) return false;
    return true;
}

}  // namespace rmr

extern "C" {

void rmr_default_temporal_params(rmr_temporal_params* p) {
    if (!p) return;
    p->max_history = 64.0f;
    p->sigma_z = 0.02f;
    p->normal_pow2 = 5;
}

int rmr_check_temporal_params(const rmr_temporal_params* p) {
    return p && rmr::temporal_params_ok(*p) ? RMR_OK : RMR_E_INVALID;
}

int rmr_temporal_view_inverse(const float view[15], double out[12]) {
    if (!view || !out) return RMR_E_INVALID;
    return rmr::temporal_view_inverse(view, out) ? RMR_OK : RMR_E_INVALID;
}

}  // extern "C"
