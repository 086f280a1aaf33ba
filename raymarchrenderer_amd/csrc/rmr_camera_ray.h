// rmr_camera_ray.h — the primary ray of a camera model for one pixel and one seed (include/rmr.h
// rmr_camera_model states each model operation by operation; this is that statement), written once for
// the kernels that generate rays: k_camera_rays (rmr_camera.hip) and k_aov (rmr_aov.hip).
// Same float semantics as the trace kernels: -ffp-contract=off, sqrt_cr, det_sin / det_cos, rand_step for
// every random number.
#pragma once
#include "rmr_camera.hpp"
#include "rmr_trace.h"

namespace rmr {

// main()'s three jitter rand() calls (primary_dir's own, RM1:569-584) for the models that use the
// jitters themselves: u = px / W + j1 / W, v = py / H + j3 / H
RMR_D void camera_uv(const KParams& P, int px, int py, float time, float& rc, float& u, float& v) {
    const float gxt = (float)px + time, gyt = (float)py + time;
    rc = 0.0f;
    const float j1 = rand_step(gxt, gyt, rc, v2(gxt, gyt));
    (void)rand_step(gxt, gyt, rc, v2(gxt, gyt));
    const float j3 = rand_step(gxt, gyt, rc, v2(gyt, gxt));
    u = (float)px / P.Wf + j1 / P.Wf;
    v = (float)py / P.Hf + j3 / P.Hf;
}

// The ray (o, d) of pixel (px, py) seeded `time` under the model C, and the chain state `rc` after the
// model's rand() calls.
RMR_D void camera_ray(const KParams& P, const CamParams& C, int px, int py, float time, V3& o, V3& d, float& rc) {
    const float gxt = (float)px + time, gyt = (float)py + time;
    const V3 eye = v3(P.eye[0], P.eye[1], P.eye[2]);
    const V3 U = v3(C.U[0], C.U[1], C.U[2]), V = v3(C.V[0], C.V[1], C.V[2]), FWD = v3(C.F[0], C.F[1], C.F[2]);
    o = eye;
    if (C.model == RMR_CAMERA_EQUIRECT) {
        float u, v;
        camera_uv(P, px, py, time, rc, u, v);
        const float lon = 6.28318548202514648438f * (u - 0.5f), pol = 3.14159274101257324219f * v;
        const float sp = det_sin(pol), cp = det_cos(pol), sl = det_sin(lon), cl = det_cos(lon);
        const float a = sp * sl, b = sp * cl, m = -cp;
        d = normalize(v3(fmaf(U.x, a, fmaf(FWD.x, b, V.x * m)), fmaf(U.y, a, fmaf(FWD.y, b, V.y * m)),
                         fmaf(U.z, a, fmaf(FWD.z, b, V.z * m))));
    } else if (C.model == RMR_CAMERA_ORTHO) {
        float u, v;
        camera_uv(P, px, py, time, rc, u, v);
        const float a = (u - 0.5f) * C.p[2], b = (v - 0.5f) * C.p[3];
        o = vfma(V, b, vfma(U, a, eye));
        d = FWD;
    } else {   // RMR_CAMERA_THIN_LENS (and RMR_CAMERA_VIEW, the same ray as the view's own)
        d = primary_dir(P, px, py, time, rc);
        const float ap = C.p[0];
        if (C.model == RMR_CAMERA_THIN_LENS && ap > 0.0f) {
            const float r1 = rand_step(gxt, gyt, rc, v2(gxt, gyt));
            const float r2 = rand_step(gxt, gyt, rc, v2(gyt, gxt));
            const float rad = sqrt_cr(r1), phi = 6.28318548202514648438f * r2;
            const float lx = rad * det_cos(phi), ly = rad * det_sin(phi);
            const V3 F = vfma(d, C.p[1], eye);
            o = vfma(V, ap * ly, vfma(U, ap * lx, eye));
            d = normalize(F - o);
        }
    }
}

}  // namespace rmr
