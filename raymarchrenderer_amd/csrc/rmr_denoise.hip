// rmr_denoise.hip — edge-avoiding a-trous preview filter (rmr_denoise): one pass of
// the 5x5 B3-spline kernel h (x) h, h = (1/16, 1/4, 3/8, 1/4, 1/16), with taps `step` pixels apart,
// weighted by the first-hit guides (same id, normal, plane distance) and optionally by colour.
//
// A pixel is live iff its guide id >= 0, its alpha != 0 and its rgb is finite. A live centre p gets
//   out(p).rgb = sum_q k_q w_q in(q).rgb / sum_q k_q w_q,   alpha unchanged,   w_p = 1 exactly,
//   w_q = 0 off the image or not live, else [id_q == id_p] max(0, n_p.n_q)^(2^normal_pow2)
//         exp(-|n_p.(x_q - x_p)| / (sigma_z step max(t_p, FLT_MIN))) [exp(-|c_q - c_p|^2 / sigma_c_i^2)];
// every other centre is copied bit for bit. The centre tap alone keeps the denominator >= 9/64.
//
// Two forms of the same arithmetic (the same taps in the same order): the plain form reads every tap
// through the vector cache; the tiled form (steps 1 and 2) first stages the block's 32x8 pixels and
// their 2 x step halo of the three planes in LDS.
#include "rmr_atrous.h"

namespace rmr {

// plain form: any step, every tap a global load
__global__ __launch_bounds__(256) void k_atrous(DenoisePass A) {
    const int x = (int)(blockIdx.x * 32 + threadIdx.x), y = (int)(blockIdx.y * 8 + threadIdx.y);
    if (x >= A.W || y >= A.H) return;
    const size_t o = (size_t)y * (size_t)A.W + (size_t)x;
    const float4 cp = A.in[o], hp = A.hit[o], np = A.nrm[o];
    if (!live(cp, np)) { A.out[o] = cp; return; }
    const float inv_z = inv_depth_scale(A, hp);
    Acc s{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = y + dy * A.step;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + dx * A.step;
            const float k = kern(dx) * kern(dy);
            if (dx == 0 && dy == 0) { add_tap(s, k, cp); continue; }
            if (qx < 0 || qy < 0 || qx >= A.W || qy >= A.H) continue;
            const size_t q = (size_t)qy * (size_t)A.W + (size_t)qx;
            const float4 cq = A.in[q], hq = A.hit[q], nq = A.nrm[q];
            // a tap that is not live adds nothing (its colour may be NaN or infinite: 0 x NaN would
            // poison the sum)
            if (live(cq, nq)) add_tap(s, k * tap_weight(A, cp, hp, np, inv_z, cq, hq, nq), cq);
        }
    }
    A.out[o] = make_float4(s.r / s.w, s.g / s.w, s.b / s.w, cp.w);
}

// tiled form: step S in {1, 2}; the block's (32 + 4S) x (8 + 4S) pixels of the three planes in LDS,
// plane by plane, rows of float4 (a 16-lane group of ds_read_b128 reads 16 consecutive 16-B slots).
// Liveness is settled once per staged pixel instead of once per tap: a pixel that is not live, or off
// the image, is staged with id -1 and colour 0, so no tap weighs it and its colour is safe to multiply;
// the rare centre that is not live copies its pixel from the input image itself.
template <int S>
__global__ __launch_bounds__(256) void k_atrous_lds(DenoisePass A) {
    constexpr int TW = 32 + 4 * S, TH = 8 + 4 * S;
    __shared__ float4 s_c[TW * TH], s_h[TW * TH], s_n[TW * TH];
    const int bx = (int)blockIdx.x * 32 - 2 * S, by = (int)blockIdx.y * 8 - 2 * S;
    const int tid = (int)(threadIdx.y * 32 + threadIdx.x);
    for (int i = tid; i < TW * TH; i += 256) {
        const int gx = bx + i % TW, gy = by + i / TW;
        float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f), h = c, n = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
        if (gx >= 0 && gy >= 0 && gx < A.W && gy < A.H) {
            const size_t q = (size_t)gy * (size_t)A.W + (size_t)gx;
            c = A.in[q]; h = A.hit[q]; n = A.nrm[q];
            if (!live(c, n)) {
                c = make_float4(0.0f, 0.0f, 0.0f, c.w);
                n.w = -1.0f;
            }
        }
        s_c[i] = c; s_h[i] = h; s_n[i] = n;
    }
    __syncthreads();
    const int x = (int)(blockIdx.x * 32 + threadIdx.x), y = (int)(blockIdx.y * 8 + threadIdx.y);
    if (x >= A.W || y >= A.H) return;
    const size_t o = (size_t)y * (size_t)A.W + (size_t)x;
    const int lp = ((int)threadIdx.y + 2 * S) * TW + (int)threadIdx.x + 2 * S;
    const float4 cp = s_c[lp], hp = s_h[lp], np = s_n[lp];
    if (np.w < 0.0f) { A.out[o] = A.in[o]; return; }
    const float inv_z = inv_depth_scale(A, hp);
    Acc s{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const float k = kern(dx) * kern(dy);
            if (dx == 0 && dy == 0) { add_tap(s, k, cp); continue; }
            const int q = lp + dy * S * TW + dx * S;
            const float4 cq = s_c[q], hq = s_h[q], nq = s_n[q];
            add_tap(s, k * tap_weight(A, cp, hp, np, inv_z, cq, hq, nq), cq);
        }
    }
    A.out[o] = make_float4(s.r / s.w, s.g / s.w, s.b / s.w, cp.w);
}

// One pass. tiled: the LDS form (A.step 1 or 2 only; other steps run the plain form).
hipError_t launch_atrous(const DenoisePass& A, bool tiled, hipStream_t s) {
    const dim3 block(32, 8), grid((unsigned)((A.W + 31) / 32), (unsigned)((A.H + 7) / 8));
    if (tiled && A.step == 1) k_atrous_lds<1><<<grid, block, 0, s>>>(A);
    else if (tiled && A.step == 2) k_atrous_lds<2><<<grid, block, 0, s>>>(A);
    else k_atrous<<<grid, block, 0, s>>>(A);
    return hipGetLastError();
}

}  // namespace rmr
