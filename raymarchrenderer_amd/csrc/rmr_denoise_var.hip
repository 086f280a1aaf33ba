// rmr_denoise_var.hip — variance-guided mode of the a-trous preview filter (rmr_denoise_variance,
// DESIGN.md §4.11): rmr_denoise.hip's pass with one more edge-stopping weight, on luminance, scaled by a
// per-pixel variance estimate that is filtered alongside the image.
//
// lum(v) = (0.2126 v.r + 0.7152 v.g) + 0.0722 v.b, always of a per-channel difference of two colours.
// A pixel is v-live iff it is live (rmr_denoise.hip) and B.w != 0 and B.rgb is finite: settled once by
// the seed kernel, which writes variance -1 for every other pixel; the passes read "v-live" as
// "variance >= 0", copy a centre that is not v-live (image and variance) and weigh no such tap.
//
//   seed:  var_0(p) = mean of lum(A(q).rgb - B(q).rgb)^2 over the v-live q of p's id with |dx|, |dy| <= radius
//   pass:  w_q = rmr_denoise's tap weight x exp(-|lum(c(q).rgb - c(p).rgb)| / (sigma_l sqrt(max(var(p), 0)) + 1e-8))
//          c'(p).rgb = sum k_q w_q c(q).rgb / sum k_q w_q       (alpha unchanged, w_p = 1)
//          var'(p)   = sum (k_q w_q)^2 var(q) / (sum k_q w_q)^2
//
// The passes come in rmr_denoise.hip's two forms with its tap order; the tiled form keeps its three
// float4 planes in LDS: a staged colour's .w carries the tap's variance (alpha is only the centre's
// business, and the centre reads its own pixel again for it).
#include "rmr_atrous.h"

namespace rmr {

namespace {

__device__ __forceinline__ float lum_diff(float4 a, float4 b) {
    return (0.2126f * (a.x - b.x) + 0.7152f * (a.y - b.y)) + 0.0722f * (a.z - b.z);
}

// 1 / (sigma_l sqrt(var_p) + 1e-8) of a v-live centre, once per centre
__device__ __forceinline__ float inv_lum_scale(float sigma_l, float vp) {
    return 1.0f / (sigma_l * sqrtf(fmaxf(vp, 0.0f)) + 1e-8f);
}

// k_q w_q of a tap that is v-live and on the image, or staged as zeros with id -1 (then 0)
__device__ __forceinline__ float guided_weight(const DenoisePass& A, float k, float4 cp, float4 hp, float4 np,
                                               float inv_z, float inv_l, float4 cq, float4 hq, float4 nq) {
    const float w = tap_weight(A, cp, hp, np, inv_z, cq, hq, nq);
    return k * (w * __expf(-fabsf(lum_diff(cq, cp)) * inv_l));
}

constexpr int kSeedMaxRadius = 4;
constexpr int kSeedTW = 32 + 2 * kSeedMaxRadius, kSeedTH = 8 + 2 * kSeedMaxRadius;

}  // namespace

// The seed. The block's 32x8 pixels and their `radius` halo as (d^2, id) in LDS; a pixel off the image
// or not v-live is staged as (0, -1), so the id compare drops it (a v-live centre's id is >= 0).
__global__ __launch_bounds__(256) void k_variance_seed(VarianceSeed V) {
    __shared__ float2 s_d[kSeedTW * kSeedTH];
    const int R = V.radius, TW = 32 + 2 * R, TH = 8 + 2 * R;
    const int bx = (int)blockIdx.x * 32 - R, by = (int)blockIdx.y * 8 - R;
    const int tid = (int)(threadIdx.y * 32 + threadIdx.x);
    for (int i = tid; i < TW * TH; i += 256) {
        const int gx = bx + i % TW, gy = by + i / TW;
        float2 e = make_float2(0.0f, -1.0f);
        if (gx >= 0 && gy >= 0 && gx < V.W && gy < V.H) {
            const size_t q = (size_t)gy * (size_t)V.W + (size_t)gx;
            const float4 a = V.a[q], b = V.b[q], n = V.nrm[q];
            if (live(a, n) && live(b, n)) {
                const float d = lum_diff(a, b);
                e = make_float2(d * d, n.w);
            }
        }
        s_d[i] = e;
    }
    __syncthreads();
    const int x = (int)(blockIdx.x * 32 + threadIdx.x), y = (int)(blockIdx.y * 8 + threadIdx.y);
    if (x >= V.W || y >= V.H) return;
    const size_t o = (size_t)y * (size_t)V.W + (size_t)x;
    const int lp = ((int)threadIdx.y + R) * TW + (int)threadIdx.x + R;
    const float id = s_d[lp].y;
    if (id < 0.0f) { V.out[o] = -1.0f; return; }
    float sum = 0.0f, n = 0.0f;
    for (int dy = -R; dy <= R; dy++)
        for (int dx = -R; dx <= R; dx++) {
            const float2 e = s_d[lp + dy * TW + dx];
            if (e.y == id) { sum += e.x; n += 1.0f; }
        }
    V.out[o] = sum / n;   // (the centre is in its own window: n >= 1)
}

// plain form: any step, every tap a global load
__global__ __launch_bounds__(256) void k_atrous_var(DenoiseVarPass P) {
    const DenoisePass& A = P.d;
    const int x = (int)(blockIdx.x * 32 + threadIdx.x), y = (int)(blockIdx.y * 8 + threadIdx.y);
    if (x >= A.W || y >= A.H) return;
    const size_t o = (size_t)y * (size_t)A.W + (size_t)x;
    const float4 cp = A.in[o];
    const float vp = P.var_in[o];
    if (!(vp >= 0.0f)) { A.out[o] = cp; P.var_out[o] = vp; return; }
    const float4 hp = A.hit[o], np = A.nrm[o];
    const float inv_z = inv_depth_scale(A, hp), inv_l = inv_lum_scale(P.sigma_l, vp);
    Acc s{0.0f, 0.0f, 0.0f, 0.0f};
    float sv = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = y + dy * A.step;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + dx * A.step;
            const float k = kern(dx) * kern(dy);
            if (dx == 0 && dy == 0) { add_tap(s, k, cp); sv = fmaf(k * k, vp, sv); continue; }
            if (qx < 0 || qy < 0 || qx >= A.W || qy >= A.H) continue;
            const size_t q = (size_t)qy * (size_t)A.W + (size_t)qx;
            const float4 cq = A.in[q], hq = A.hit[q], nq = A.nrm[q];
            const float vq = P.var_in[q];
            // a tap that is not v-live adds nothing (its colour may be NaN or infinite)
            if (vq >= 0.0f) {
                const float kw = guided_weight(A, k, cp, hp, np, inv_z, inv_l, cq, hq, nq);
                add_tap(s, kw, cq);
                sv = fmaf(kw * kw, vq, sv);
            }
        }
    }
    A.out[o] = make_float4(s.r / s.w, s.g / s.w, s.b / s.w, cp.w);
    P.var_out[o] = sv / (s.w * s.w);
}

// tiled form: step S in {1, 2}; k_atrous_lds's tile, with the pixel's variance in the staged colour's
// .w. A pixel that is not v-live, or off the image, is staged with id -1, colour 0 and variance 0: no
// tap weighs it and everything of it is safe to multiply.
template <int S>
__global__ __launch_bounds__(256) void k_atrous_var_lds(DenoiseVarPass P) {
    const DenoisePass& A = P.d;
    constexpr int TW = 32 + 4 * S, TH = 8 + 4 * S;
    __shared__ float4 s_c[TW * TH], s_h[TW * TH], s_n[TW * TH];
    const int bx = (int)blockIdx.x * 32 - 2 * S, by = (int)blockIdx.y * 8 - 2 * S;
    const int tid = (int)(threadIdx.y * 32 + threadIdx.x);
    for (int i = tid; i < TW * TH; i += 256) {
        const int gx = bx + i % TW, gy = by + i / TW;
        float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f), h = c, n = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
        if (gx >= 0 && gy >= 0 && gx < A.W && gy < A.H) {
            const size_t q = (size_t)gy * (size_t)A.W + (size_t)gx;
            const float v = P.var_in[q];
            c = A.in[q]; h = A.hit[q]; n = A.nrm[q];
            c.w = v;
            if (!(v >= 0.0f)) {
                c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
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
    if (np.w < 0.0f) { A.out[o] = A.in[o]; P.var_out[o] = P.var_in[o]; return; }
    const float vp = cp.w;
    const float inv_z = inv_depth_scale(A, hp), inv_l = inv_lum_scale(P.sigma_l, vp);
    Acc s{0.0f, 0.0f, 0.0f, 0.0f};
    float sv = 0.0f;
    // rows one at a time (a row of taps in flight: 57 VGPRs; all 24 taps unrolled hold 235)
#pragma unroll 1
    for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const float k = kern(dx) * kern(dy);
            if (dx == 0 && dy == 0) { add_tap(s, k, cp); sv = fmaf(k * k, vp, sv); continue; }
            const int q = lp + dy * S * TW + dx * S;
            const float4 cq = s_c[q], hq = s_h[q], nq = s_n[q];
            const float kw = guided_weight(A, k, cp, hp, np, inv_z, inv_l, cq, hq, nq);
            add_tap(s, kw, cq);
            sv = fmaf(kw * kw, cq.w, sv);
        }
    }
    A.out[o] = make_float4(s.r / s.w, s.g / s.w, s.b / s.w, A.in[o].w);
    P.var_out[o] = sv / (s.w * s.w);
}

hipError_t launch_variance_seed(const VarianceSeed& V, hipStream_t s) {
    if (V.radius < 0 || V.radius > kSeedMaxRadius) return hipErrorInvalidValue;   // (the LDS tile's size)
    const dim3 block(32, 8), grid((unsigned)((V.W + 31) / 32), (unsigned)((V.H + 7) / 8));
    k_variance_seed<<<grid, block, 0, s>>>(V);
    return hipGetLastError();
}

hipError_t launch_atrous_var(const DenoiseVarPass& P, bool tiled, hipStream_t s) {
    const dim3 block(32, 8), grid((unsigned)((P.d.W + 31) / 32), (unsigned)((P.d.H + 7) / 8));
    if (tiled && P.d.step == 1) k_atrous_var_lds<1><<<grid, block, 0, s>>>(P);
    else if (tiled && P.d.step == 2) k_atrous_var_lds<2><<<grid, block, 0, s>>>(P);
    else k_atrous_var<<<grid, block, 0, s>>>(P);
    return hipGetLastError();
}

}  // namespace rmr
