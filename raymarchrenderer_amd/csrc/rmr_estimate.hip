// rmr_estimate.hip — the per-tile error estimate behind adaptive sampling: the
// running-mean fold that also keeps the half image (the mean of the odd-indexed samples), and the tile
// error kernel that compares the accumulator with it, one wave per 8x8 tile of the image's lattice.
// Every float operation is rounded on its own (-ffp-contract=off, IEEE division, correctly rounded
// sqrt), so both are checkable bit for bit: the fold against the oracle's render of the same seeds, the
// tile error against tests/adaptive_ref.py.
#include <hip/hip_runtime.h>
#include "rmr_internal.h"
#include "rmr_math.h"

namespace rmr {

// k_fold (rmr_trace.h fold_main) plus the half image: the accumulator gets the same expressions in the
// same order, the work-queue counters the same zeroing; a sample of odd global index n also goes into
// `half` with the running-mean index n >> 1 (0 overwrites). One pass over the sample planes serves both.
__global__ __launch_bounds__(256) void k_fold_half(KParams P, float4* half) {
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid < (int)(kQueueBytes / (4 * kQueueWordStride))) ((uint32_t*)P.queue)[gid * kQueueWordStride] = 0u;
    const int tile = gid >> 6, lane = gid & 63;
    if (tile >= P.n_tiles) return;
    const TileXY txy = P.tiles[tile];
    const int px = txy.x + (lane & 7), py = txy.y + (lane >> 3);
    if (px < P.x0 || py < P.y0 || px >= P.x1 || py >= P.y1) return;
    const size_t o = (size_t)py * P.W + px;
    float4 acc = P.accum[o];
    float4 hb = half[o];
    const size_t plane = (size_t)P.n_tiles * 64;
    for (uint32_t k = 0; k < P.nspp; k++) {
        const float4 c = P.samp[(size_t)k * plane + (size_t)tile * 64 + lane];
        const uint32_t n = P.first_sample + k;
        if (n != 0u) {
            const float f1 = 1.0f / (float)(n + 1u);
            const float f2 = (float)n / (float)(n + 1u);
            acc.x = c.x * f1 + acc.x * f2;
            acc.y = c.y * f1 + acc.y * f2;
            acc.z = c.z * f1 + acc.z * f2;
        } else {
            acc.x = c.x; acc.y = c.y; acc.z = c.z;
        }
        acc.w = 1.0f;
        if (n & 1u) {
            const uint32_t m = n >> 1;
            if (m != 0u) {
                const float g1 = 1.0f / (float)(m + 1u);
                const float g2 = (float)m / (float)(m + 1u);
                hb.x = c.x * g1 + hb.x * g2;
                hb.y = c.y * g1 + hb.y * g2;
                hb.z = c.z * g1 + hb.z * g2;
            } else {
                hb.x = c.x; hb.y = c.y; hb.z = c.z;
            }
            hb.w = 1.0f;
        }
    }
    P.accum[o] = acc;
    half[o] = hb;
}

hipError_t launch_fold_half(const KParams& P, float4* half, hipStream_t s) {
    const uint64_t threads = (uint64_t)P.n_tiles * 64;
    k_fold_half<<<(unsigned)((threads + 255) / 256), 256, 0, s>>>(P, half);
    return hipGetLastError();
}

__device__ __forceinline__ bool finite3(float4 a) {
    return (__float_as_uint(a.x) & 0x7f800000u) != 0x7f800000u && (__float_as_uint(a.y) & 0x7f800000u) != 0x7f800000u &&
           (__float_as_uint(a.z) & 0x7f800000u) != 0x7f800000u;
}

// One wave per tile (tx, ty) of the image's 8-pixel lattice, lane l = pixel (8 tx + (l & 7), 8 ty + (l >> 3)).
// Per pixel v = (|dr| + |dg|) + |db| over offset + sqrt(max((r + g) + b, 0)) of the accumulator, d the
// difference to the half image; 0 outside the image (not counted) and for a non-finite pixel (counted); a
// pixel with fewer than two samples (either alpha 0) makes its tile's error +inf. The sum is the xor
// butterfly over steps 1 .. 32 (every lane ends with the same bits; the pairwise tree v[0::2] + v[1::2]),
// divided by the tile's pixel count inside the image.
__global__ __launch_bounds__(256) void k_tile_error(const float4* A, const float4* B, int W, int H, int TX, int TY,
                                                    float offset, float* out) {
    const int tile = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (tile >= TX * TY) return;   // (wave-uniform)
    const int lane = (int)(threadIdx.x & 63u);
    const int px = 8 * (tile % TX) + (lane & 7), py = 8 * (tile / TX) + (lane >> 3);
    const bool inside = px < W && py < H;
    float v = 0.0f;
    bool unsampled = false;
    if (inside) {
        const size_t o = (size_t)py * (size_t)W + (size_t)px;
        const float4 a = A[o], b = B[o];
        if (a.w == 0.0f || b.w == 0.0f) {
            unsampled = true;
        } else if (finite3(a) && finite3(b)) {
            const float d = (fabsf(a.x - b.x) + fabsf(a.y - b.y)) + fabsf(a.z - b.z);
            const float s = (a.x + a.y) + a.z;
            v = d / (offset + sqrt_cr(fmaxf(s, 0.0f)));
        }
    }
#pragma unroll
    for (int step = 1; step < 64; step <<= 1) v += __shfl_xor(v, step, 64);
    const int n_t = __popcll(__ballot(inside));
    const bool any_unsampled = __ballot(unsampled) != 0ull;
    if (lane == 0) out[tile] = any_unsampled ? __builtin_inff() : v / (float)n_t;
}

// A, B: W x H float4 each; out: ceil(H / 8) x ceil(W / 8) floats.
hipError_t launch_tile_error(const float4* A, const float4* B, int W, int H, float offset, float* out, hipStream_t s) {
    const int TX = (W + 7) / 8, TY = (H + 7) / 8;
    const long long tiles = (long long)TX * TY;
    k_tile_error<<<(unsigned)((tiles + 3) / 4), 256, 0, s>>>(A, B, W, H, TX, TY, offset, out);
    return hipGetLastError();
}

}  // namespace rmr
