// rmr_temporal.hip — temporal reprojection of the preview across camera moves (rmr_temporal_accumulate,
// DESIGN.md §4.12): one thread per pixel of the current view projects its first hit into the history
// view, gathers the history's four nearest pixels with the a-trous filter's normal and plane-distance
// weights, and blends the result with the current frame by effective sample count.
//
// With x, n, id, t the pixel's guides, d = x - eye', (U0, V0, w0) = Minv d, k = Minv twist:
//   the history ray through x is lambda (r00' + u a + v b + u v c), so with U = lambda u, V = lambda v,
//   w = lambda:  (U, V, w) = (U0, V0, w0) - T k,  T = U V / w,  i.e.  A T^2 - B T + C = 0 with
//   A = k0 k1 + k2, B = w0 + U0 k1 + V0 k0, C = U0 V0; T = C / B, then three Newton steps.
//   fx = (U / w) W, fy = (V / w) H; no history when w <= 0 or fx, fy is not finite.
//   taps q0 + {0,1}^2, q0 = floor((fx, fy) - 0.5), bilinear weights b_q; a tap counts when it is on the
//   image, Hn(q) > 0 and id_q == id, with g_q = b_q a_q z_q (rmr_atrous.h tap_weight, no colour term).
//   G = sum g_q, h = sum g_q Hc(q) / G, m = min(max_history, sum g_q Hn(q))
//   out.rgb = (m h + n_cur S.rgb) / (m + n_cur), n_out = min(m + n_cur, max_history)
// A pixel that is not live: out = S, n_out = 0. No usable history (no projection, G = 0, m = 0 or h not
// finite): out = S, n_out = min(n_cur, max_history).
#include "rmr_atrous.h"

namespace rmr {

__global__ __launch_bounds__(256) void k_temporal(TemporalPass T) {
    const DenoisePass& A = T.d;
    const int x = (int)(blockIdx.x * 32 + threadIdx.x), y = (int)(blockIdx.y * 8 + threadIdx.y);
    if (x >= A.W || y >= A.H) return;
    const size_t o = (size_t)y * (size_t)A.W + (size_t)x;
    const float4 S = A.in[o], np = A.nrm[o];
    const float nan = __builtin_nanf("");
    float2 xy = make_float2(nan, nan);
    float4 res = S;
    float n_res = 0.0f;
    if (live(S, np)) {
        n_res = fminf(T.n_cur, T.max_history);
        const float4 hp = A.hit[o];
        const float dx = hp.x - T.eye[0], dy = hp.y - T.eye[1], dz = hp.z - T.eye[2];
        const float U0 = fmaf(T.minv[0], dx, fmaf(T.minv[1], dy, T.minv[2] * dz));
        const float V0 = fmaf(T.minv[3], dx, fmaf(T.minv[4], dy, T.minv[5] * dz));
        const float w0 = fmaf(T.minv[6], dx, fmaf(T.minv[7], dy, T.minv[8] * dz));
        const float k0 = T.twist[0], k1 = T.twist[1], k2 = T.twist[2];
        const float qa = fmaf(k0, k1, k2), qb = fmaf(U0, k1, fmaf(V0, k0, w0)), qc = U0 * V0;
        float tw = qc / qb;
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const float g = fmaf(fmaf(qa, tw, -qb), tw, qc);
            const float gp = fmaf(qa + qa, tw, -qb);
            tw = tw - g / gp;
        }
        const float U = fmaf(-tw, k0, U0), V = fmaf(-tw, k1, V0), w = fmaf(-tw, k2, w0);
        const float fx = (U / w) * T.Wf, fy = (V / w) * T.Hf;
        if (w > 0.0f && __builtin_isfinite(fx) && __builtin_isfinite(fy)) {
            xy = make_float2(fx, fy);
            const float gx = fx - 0.5f, gy = fy - 0.5f;
            // (a tap is on the image only for q0 in [-1, W - 1] x [-1, H - 1]; also keeps the int conversion in range)
            if (gx >= -1.0f && gy >= -1.0f && gx < T.Wf && gy < T.Hf) {
                const float flx = floorf(gx), fly = floorf(gy);
                const int qx0 = (int)flx, qy0 = (int)fly;
                const float tx = gx - flx, ty = gy - fly;
                const float inv_z = inv_depth_scale(A, hp);
                Acc s{0.0f, 0.0f, 0.0f, 0.0f};
                float m = 0.0f;
#pragma unroll
                for (int j = 0; j < 2; j++) {
#pragma unroll
                    for (int i = 0; i < 2; i++) {
                        const int qx = qx0 + i, qy = qy0 + j;
                        if (qx < 0 || qy < 0 || qx >= A.W || qy >= A.H) continue;
                        const size_t q = (size_t)qy * (size_t)A.W + (size_t)qx;
                        const float hn = T.h_n[q];
                        if (!(hn > 0.0f)) continue;
                        const float4 nq = T.h_nrm[q];
                        if (nq.w != np.w) continue;
                        const float b = (i ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty);
                        const float g = b * tap_weight(A, S, hp, np, inv_z, S, T.h_hit[q], nq);
                        add_tap(s, g, T.h_col[q]);
                        m = fmaf(g, hn, m);
                    }
                }
                m = fminf(T.max_history, m);
                const float hr = s.r / s.w, hg = s.g / s.w, hb = s.b / s.w;
                if (s.w > 0.0f && m > 0.0f && __builtin_isfinite(hr) && __builtin_isfinite(hg) && __builtin_isfinite(hb)) {
                    const float den = m + T.n_cur;
                    res = make_float4((m * hr + T.n_cur * S.x) / den, (m * hg + T.n_cur * S.y) / den,
                                      (m * hb + T.n_cur * S.z) / den, S.w);
                    n_res = fminf(den, T.max_history);
                }
            }
        }
    }
    A.out[o] = res;
    T.n_out[o] = n_res;
    if (T.xy_out) T.xy_out[o] = xy;
}

hipError_t launch_temporal(const TemporalPass& T, hipStream_t s) {
    const dim3 block(32, 8), grid((unsigned)((T.d.W + 31) / 32), (unsigned)((T.d.H + 7) / 8));
    k_temporal<<<grid, block, 0, s>>>(T);
    return hipGetLastError();
}

}  // namespace rmr
