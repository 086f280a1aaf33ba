// rmr_bloom.hip — the HDR bloom stage ahead of tone mapping (rmr_bloom). The rule is
// rmr_bloom_rule.h, shared with the host (bloom.cpp).
//
//   k_bloom_down0    the bright part P of the source and the first down in one pass (P is never stored):
//                    a 32 x 8 tile of level 1 per block; the block first filters along x the 18 source
//                    rows the tile and its one-pixel halo need into LDS, 18 rows of 32 float4 (row-major:
//                    the 16 lanes of a ds_read_b128 group read 16 consecutive 16-B slots), then every
//                    thread filters its column of four staged rows along y.
//   k_bloom_down     the same from one level to the next.
//   k_bloom_up       U_k = B_k + s up(U_{k+1}) in place, one thread per pixel of level k: its own B_k and
//                    four taps of U_{k+1} (along x in the near and the far row, then along y).
//   k_bloom_tail     the small levels in one launch: one block of 1024 threads runs the downs of levels
//                    k0..N into LDS (12 B per pixel; its first input comes from memory, the source through P
//                    when k0 = 1), then the ups N-1..k0 in place in LDS, and stores U_k0. The same
//                    arithmetic: a thread filters four rows along x itself, then along y.
//   k_bloom_compose  out = S + gain up(U_1) with the copy rule: 16 B in, four taps of the quarter-size
//                    U_1 through the cache, 16 B out.
#include <hip/hip_runtime.h>

#include "rmr_internal.h"
#include "rmr_bloom_rule.h"

namespace rmr {

constexpr int kBloomTW = 32, kBloomTH = 8;             // a block's tile, in pixels of the level it writes
constexpr int kBloomRows = 2 * kBloomTH + 2;           // staged rows: two per output row and the halo
constexpr int kBloomThreads = kBloomTW * kBloomTH;

// What the down pass reads at (x, y) of its w x h input: the bright part of a source pixel, or a level.
struct BloomSrcBright {
    const float4* p;
    int w;
    float T, clamp;
    __device__ Bloom3 operator()(int x, int y) const {
        const float4 s = p[(size_t)y * w + x];
        return bloom_bright(s.x, s.y, s.z, s.w, T, clamp);
    }
};
struct BloomSrcLevel {
    const float4* p;
    int w;
    __device__ Bloom3 operator()(int x, int y) const {
        const float4 s = p[(size_t)y * w + x];
        const Bloom3 v = {s.x, s.y, s.z};
        return v;
    }
};

template <class Src>
__device__ inline void bloom_down_tile(const Src& src, int w, int h, float4* __restrict__ out) {
    __shared__ float4 xs[kBloomRows][kBloomTW];
    const int w2 = bloom_half(w), h2 = bloom_half(h);
    const int ox0 = (int)blockIdx.x * kBloomTW, oy0 = (int)blockIdx.y * kBloomTH;
    // along x: staged row r is the input row cl(2 oy0 - 1 + r); a column past the level repeats its last
    // one (never stored)
    for (int idx = (int)threadIdx.x; idx < kBloomRows * kBloomTW; idx += kBloomThreads) {
        const int r = idx / kBloomTW, j = idx % kBloomTW;
        const int sy = bloom_cl(2 * oy0 - 1 + r, h);
        const int i = 2 * bloom_cl(ox0 + j, w2);
        const Bloom3 d = bloom_down3(src(bloom_cl(i - 1, w), sy), src(i, sy), src(bloom_cl(i + 1, w), sy),
                                     src(bloom_cl(i + 2, w), sy));
        xs[r][j] = make_float4(d.x, d.y, d.z, 0.0f);
    }
    __syncthreads();
    // along y: the taps cl(2 oy + d), d = -1..2, of output row oy = oy0 + ty are the staged rows 2 ty + d + 1
    const int tx = (int)threadIdx.x % kBloomTW, ty = (int)threadIdx.x / kBloomTW;
    const int ox = ox0 + tx, oy = oy0 + ty;
    if (ox >= w2 || oy >= h2) return;
    const float4 am = xs[2 * ty][tx], a0 = xs[2 * ty + 1][tx], a1 = xs[2 * ty + 2][tx], a2 = xs[2 * ty + 3][tx];
    out[(size_t)oy * w2 + ox] = make_float4(bloom_down1(am.x, a0.x, a1.x, a2.x), bloom_down1(am.y, a0.y, a1.y, a2.y),
                                            bloom_down1(am.z, a0.z, a1.z, a2.z), 0.0f);
}

__global__ __launch_bounds__(kBloomThreads) void k_bloom_down0(const float4* __restrict__ src, int w, int h, float T, float clamp,
                                                              float4* __restrict__ out) {
    const BloomSrcBright s = {src, w, T, clamp};
    bloom_down_tile(s, w, h, out);
}

__global__ __launch_bounds__(kBloomThreads) void k_bloom_down(const float4* __restrict__ in, int w, int h, float4* __restrict__ out) {
    const BloomSrcLevel s = {in, w};
    bloom_down_tile(s, w, h, out);
}

// up(b) at (x, y), b being mw x mh
template <class Src>
__device__ inline Bloom3 bloom_up_at(const Src& b, int mw, int mh, int x, int y) {
    const int jx = x >> 1, fx = bloom_up_far(x, mw), jy = y >> 1, fy = bloom_up_far(y, mh);
    const Bloom3 near = bloom_up3(b(jx, jy), b(fx, jy));
    const Bloom3 far = bloom_up3(b(jx, fy), b(fx, fy));
    return bloom_up3(near, far);
}

__global__ __launch_bounds__(kBloomThreads) void k_bloom_up(float4* __restrict__ bk, int w, int h, const float4* __restrict__ uk1,
                                                           float s) {
    const int x = (int)blockIdx.x * kBloomTW + (int)threadIdx.x % kBloomTW;
    const int y = (int)blockIdx.y * kBloomTH + (int)threadIdx.x / kBloomTW;
    if (x >= w || y >= h) return;
    const BloomSrcLevel up = {uk1, bloom_half(w)};
    const Bloom3 u = bloom_up_at(up, bloom_half(w), bloom_half(h), x, y);
    const size_t i = (size_t)y * w + x;
    const float4 b = bk[i];
    bk[i] = make_float4(bloom_mad(b.x, s, u.x), bloom_mad(b.y, s, u.y), bloom_mad(b.z, s, u.z), 0.0f);
}

__global__ __launch_bounds__(kBloomThreads) void k_bloom_compose(const float4* __restrict__ src, int w, int h,
                                                                const float4* __restrict__ u1, float gain, float4* __restrict__ out) {
    const int x = (int)blockIdx.x * kBloomTW + (int)threadIdx.x % kBloomTW;
    const int y = (int)blockIdx.y * kBloomTH + (int)threadIdx.x / kBloomTW;
    if (x >= w || y >= h) return;
    const size_t i = (size_t)y * w + x;
    const float4 p = src[i];
    float4 o = p;   // (an invalid pixel, and every alpha: bit for bit)
    if (!bloom_invalid(p.x, p.y, p.z, p.w)) {
        const BloomSrcLevel up = {u1, bloom_half(w)};
        const Bloom3 g = bloom_up_at(up, bloom_half(w), bloom_half(h), x, y);
        o.x = bloom_mad(p.x, gain, g.x);
        o.y = bloom_mad(p.y, gain, g.y);
        o.z = bloom_mad(p.z, gain, g.z);
    }
    out[i] = o;
}

// ---- the small levels in one block -------------------------------------------------------------------
struct BloomSrcLds {
    const Bloom3* p;
    int w;
    __device__ Bloom3 operator()(int x, int y) const { return p[y * w + x]; }
};

// down of a w x h input into LDS by the whole block: per output pixel, four rows along x, then along y
template <class Src>
__device__ inline void bloom_tail_down(const Src& src, int w, int h, Bloom3* __restrict__ out) {
    const int w2 = bloom_half(w), h2 = bloom_half(h);
    for (int idx = (int)threadIdx.x; idx < w2 * h2; idx += kBloomTailThreads) {
        const int ox = idx % w2, oy = idx / w2;
        const int i = 2 * ox, xm = bloom_cl(i - 1, w), x1 = bloom_cl(i + 1, w), x2 = bloom_cl(i + 2, w);
        // (row by row in a rolled loop: sixteen taps in flight at once cost more registers than 1024 threads have)
        const Bloom3 zero = {0.0f, 0.0f, 0.0f};
        Bloom3 rm = zero, r0 = zero, r1 = zero, r2 = zero;
#pragma unroll 1
        for (int d = 0; d < 4; d++) {
            const int sy = bloom_cl(2 * oy - 1 + d, h);
            const Bloom3 v = bloom_down3(src(xm, sy), src(i, sy), src(x1, sy), src(x2, sy));
            if (d == 0) rm = v;
            else if (d == 1) r0 = v;
            else if (d == 2) r1 = v;
            else r2 = v;
        }
        out[idx] = bloom_down3(rm, r0, r1, r2);
    }
}

// the size of the level `steps` halvings below a w x h one, and the pixels of the levels before it
struct BloomTailLevel {
    int w, h, off;
};
__device__ inline BloomTailLevel bloom_tail_level(int w, int h, int steps) {
    BloomTailLevel l = {w, h, 0};
    for (int i = 0; i < steps; i++) {
        l.off += l.w * l.h;
        l.w = bloom_half(l.w);
        l.h = bloom_half(l.h);
    }
    return l;
}

__global__ __launch_bounds__(kBloomTailThreads) void k_bloom_tail(const float4* __restrict__ in, float4* __restrict__ out, BloomTail t) {
    __shared__ Bloom3 lv[kBloomTailPixels];
    const int w0 = bloom_half(t.w_in), h0 = bloom_half(t.h_in);   // level k0, at lv; level k0 + i follows the i before it
    // the downs: level k0 from memory, the rest from LDS
    if (t.from_source) {
        const BloomSrcBright s = {in, t.w_in, t.threshold, t.clamp};
        bloom_tail_down(s, t.w_in, t.h_in, lv);
    } else {
        const BloomSrcLevel s = {in, t.w_in};
        bloom_tail_down(s, t.w_in, t.h_in, lv);
    }
    __syncthreads();
    for (int i = 1; i < t.count; i++) {
        const BloomTailLevel a = bloom_tail_level(w0, h0, i - 1), b = bloom_tail_level(w0, h0, i);
        const BloomSrcLds s = {lv + a.off, a.w};
        bloom_tail_down(s, a.w, a.h, lv + b.off);
        __syncthreads();
    }
    // the ups, in place: a thread reads its own B_k and four taps of the level below it
    for (int i = t.count - 2; i >= 0; i--) {
        const BloomTailLevel a = bloom_tail_level(w0, h0, i), b = bloom_tail_level(w0, h0, i + 1);
        const BloomSrcLds up = {lv + b.off, b.w};
        Bloom3* bk = lv + a.off;
        for (int idx = (int)threadIdx.x; idx < a.w * a.h; idx += kBloomTailThreads) {
            const Bloom3 u = bloom_up_at(up, b.w, b.h, idx % a.w, idx / a.w);
            const Bloom3 v = bk[idx];
            const Bloom3 r = {bloom_mad(v.x, t.scatter, u.x), bloom_mad(v.y, t.scatter, u.y), bloom_mad(v.z, t.scatter, u.z)};
            bk[idx] = r;
        }
        __syncthreads();
    }
    for (int idx = (int)threadIdx.x; idx < w0 * h0; idx += kBloomTailThreads)
        out[idx] = make_float4(lv[idx].x, lv[idx].y, lv[idx].z, 0.0f);
}

bool bloom_tail_plan(const int* w, const int* h, int levels, int max_pixels, float threshold, float clamp, float scatter,
                     BloomTail* t) {
    if (max_pixels > kBloomTailPixels) max_pixels = kBloomTailPixels;
    // the first level from which everything down to `levels` fits; a tail of one level is a plain down
    int k0 = levels + 1;
    long long sum = 0;
    while (k0 > 1 && sum + (long long)w[k0 - 1] * h[k0 - 1] <= (long long)max_pixels) {
        k0--;
        sum += (long long)w[k0] * h[k0];
    }
    if (k0 >= levels) return false;
    *t = BloomTail{};
    t->k0 = k0;
    t->count = levels - k0 + 1;
    t->w_in = w[k0 - 1];
    t->h_in = h[k0 - 1];
    t->from_source = k0 == 1 ? 1 : 0;
    t->threshold = threshold;
    t->clamp = clamp;
    t->scatter = scatter;
    return true;
}

hipError_t launch_bloom_tail(const float4* in, float4* out, const BloomTail& t, hipStream_t s) {
    k_bloom_tail<<<dim3(1), dim3(kBloomTailThreads), 0, s>>>(in, out, t);
    return hipGetLastError();
}

namespace {
dim3 bloom_grid(int w, int h) {
    return dim3((unsigned)((w + kBloomTW - 1) / kBloomTW), (unsigned)((h + kBloomTH - 1) / kBloomTH));
}
}  // namespace

hipError_t launch_bloom_down0(const float4* src, int w, int h, float threshold, float clamp, float4* out, hipStream_t s) {
    k_bloom_down0<<<bloom_grid(bloom_half(w), bloom_half(h)), dim3(kBloomThreads), 0, s>>>(src, w, h, threshold, clamp, out);
    return hipGetLastError();
}

hipError_t launch_bloom_down(const float4* in, int w, int h, float4* out, hipStream_t s) {
    k_bloom_down<<<bloom_grid(bloom_half(w), bloom_half(h)), dim3(kBloomThreads), 0, s>>>(in, w, h, out);
    return hipGetLastError();
}

hipError_t launch_bloom_up(float4* bk, int w, int h, const float4* uk1, float scatter, hipStream_t s) {
    k_bloom_up<<<bloom_grid(w, h), dim3(kBloomThreads), 0, s>>>(bk, w, h, uk1, scatter);
    return hipGetLastError();
}

hipError_t launch_bloom_compose(const float4* src, int w, int h, const float4* u1, float gain, float4* out, hipStream_t s) {
    k_bloom_compose<<<bloom_grid(w, h), dim3(kBloomThreads), 0, s>>>(src, w, h, u1, gain, out);
    return hipGetLastError();
}

}  // namespace rmr
