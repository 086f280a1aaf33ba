// rmr_tonemap.hip — tone mapping and histogram auto-exposure of the output stage (rmr_tonemap,
// DESIGN.md §4.13). The rule is rmr_tonemap_rule.h, shared with the host (tonemap.cpp).
//
//   k_lum_hist  the luminance histogram of a W x H float4 plane: 256 threads per block, each taking
//               four pixels (16-B loads) per round of a grid-stride loop, into 257 words of LDS (256
//               bins and the skipped count); each block then stores its 257 words plainly to its own
//               row of a [blocks][257] slab. No memset and no global atomic.
//   k_meter     one block: sums the slab's rows per bin; thread b works out bin b's weight from the
//               integer counts before it; one lane adds the 255 weights in bin order in double, finishes
//               the rule and writes the state {l, scale, valid}; the summed histogram beside it.
//   k_tonemap   one thread per pixel, 16 B in and 16 B out, the scale read from the state word.
#include <hip/hip_runtime.h>

#include "rmr_internal.h"
#include "rmr_tonemap_rule.h"

namespace rmr {

constexpr int kHistThreads = 256;
constexpr int kHistPerThread = 4;
constexpr int kFoldRounds = 2;   // in-wave folds before the lanes left over add on their own

// One count for `slot` (0..256, or -1: none) of every lane. FOLD: the lanes that hold the first
// pending lane's slot are counted with one LDS add of their number, kFoldRounds times (a flat image has
// all 64 lanes on one word); whoever is left adds 1 itself. Called from wave-uniform control flow.
template <bool FOLD>
__device__ inline void hist_add(uint32_t* h, int slot) {
    if constexpr (FOLD) {
        const int lane = (int)(threadIdx.x & 63u);
        unsigned long long todo = __ballot(slot >= 0);
#pragma unroll
        for (int r = 0; r < kFoldRounds; r++) {
            if (!todo) break;
            const int lead_lane = __ffsll((long long)todo) - 1;
            const int lead = __shfl(slot, lead_lane);
            const unsigned long long m = __ballot(slot == lead);
            if (lane == lead_lane) atomicAdd(&h[lead], (uint32_t)__popcll(m));
            todo &= ~m;
        }
        if ((todo >> lane) & 1ull) atomicAdd(&h[slot], 1u);
    } else {
        if (slot >= 0) atomicAdd(&h[slot], 1u);
    }
}

template <bool FOLD>
__global__ __launch_bounds__(kHistThreads) void k_lum_hist(const float4* __restrict__ in, size_t n, uint32_t* __restrict__ slab) {
    __shared__ uint32_t h[kToneWords];
    for (int i = (int)threadIdx.x; i < kToneWords; i += kHistThreads) h[i] = 0u;
    __syncthreads();
    const size_t stride = (size_t)gridDim.x * kHistThreads;
    // (the loop's bounds are the block's, so that every lane of a wave takes every round)
    for (size_t b0 = (size_t)blockIdx.x * kHistThreads; b0 < n; b0 += stride * kHistPerThread) {
        float4 p[kHistPerThread];
        bool on[kHistPerThread];
#pragma unroll
        for (int k = 0; k < kHistPerThread; k++) {
            const size_t i = b0 + (size_t)k * stride + threadIdx.x;
            on[k] = i < n;
            p[k] = on[k] ? in[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
#pragma unroll
        for (int k = 0; k < kHistPerThread; k++) {
            const int bin = lum_bin(p[k].x, p[k].y, p[k].z, p[k].w);
            hist_add<FOLD>(h, !on[k] ? -1 : (bin < 0 ? kToneSkipped : bin));
        }
    }
    __syncthreads();
    uint32_t* row = slab + (size_t)blockIdx.x * kToneWords;
    for (int i = (int)threadIdx.x; i < kToneWords; i += kHistThreads) row[i] = h[i];
}

constexpr int kMeterThreads = 1024;
constexpr int kMeterParts = kMeterThreads / kToneBins;

// run_meter 0: the histogram alone (rmr_luminance_histogram), the state's l, scale and valid untouched.
__global__ __launch_bounds__(kMeterThreads) void k_meter(const uint32_t* __restrict__ slab, int rows, ToneState* __restrict__ st,
                                                       const double* __restrict__ lc, ToneMeter M, int run_meter) {
    __shared__ uint32_t part[kMeterParts][kToneBins];
    __shared__ uint32_t part_skip[kMeterParts];
    __shared__ uint32_t total[kToneBins];
    __shared__ double bin_w[kToneBins], bin_t[kToneBins];
    const int b = (int)(threadIdx.x & (kToneBins - 1)), q = (int)(threadIdx.x / kToneBins);
    uint32_t s = 0u, sk = 0u;
    for (int r = q; r < rows; r += kMeterParts) s += slab[(size_t)r * kToneWords + b];
    if (b == 0)
        for (int r = q; r < rows; r += kMeterParts) sk += slab[(size_t)r * kToneWords + kToneSkipped];
    part[q][b] = s;
    if (b == 0) part_skip[q] = sk;
    __syncthreads();
    if (q == 0) {
        uint32_t t = 0u;
#pragma unroll
        for (int k = 0; k < kMeterParts; k++) t += part[k][b];
        total[b] = t;
        st->hist[b] = t;
    }
    __syncthreads();
    if (!run_meter) {
        if (threadIdx.x == 0) {
            unsigned long long skipped = 0ull;
#pragma unroll
            for (int k = 0; k < kMeterParts; k++) skipped += part_skip[k];
            st->skipped = skipped;
        }
        return;
    }
    // thread b: bin b's weight from the integer counts before it (meter_bin), every bin at once
    uint64_t C = 0, N = 0;
    if (q == 0) {
        for (int j = 1; j < kToneBins; j++) {
            const uint32_t n = total[j];
            if (j < b) C += n;
            N += n;
        }
        double w = 0.0, t = 0.0;
        if (b >= 1 && N != 0) meter_bin(C, total[b], N, M, lc[b - 1], w, t);
        bin_w[b] = w;
        bin_t[b] = t;
    }
    __syncthreads();
    // one lane: the sums in bin order, and the rest of the rule
    if (threadIdx.x == 0) {
        unsigned long long skipped = 0ull;
#pragma unroll
        for (int k = 0; k < kMeterParts; k++) skipped += part_skip[k];
        st->skipped = skipped;
        const bool has_prev = st->valid != 0u;
        const double l_prev = has_prev ? st->l : 0.0;
        double l;
        if (N == 0) {
            l = has_prev ? l_prev : M.ev;
        } else {
            double sw = 0.0, swl = 0.0;
            for (int j = 1; j < kToneBins; j++) {
                swl = swl + bin_t[j];
                sw = sw + bin_w[j];
            }
            l = meter_finish(swl, sw, M, has_prev, l_prev);
        }
        st->l = l;
        st->scale = (float)exp2(l);
        st->valid = 1u;
    }
}

__global__ __launch_bounds__(256) void k_tonemap(const float4* __restrict__ in, float4* __restrict__ out, size_t n,
                                                const ToneState* __restrict__ st, float scale_manual, int curve, float iw2) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float scale = st ? st->scale : scale_manual;
    const float4 p = in[i];
    out[i] = make_float4(tone_curve(curve, p.x, scale, iw2), tone_curve(curve, p.y, scale, iw2),
                         tone_curve(curve, p.z, scale, iw2), p.w);
}

int lum_hist_blocks(size_t n) {
    const size_t per_block = (size_t)kHistThreads * kHistPerThread;
    const size_t want = (n + per_block - 1) / per_block;
    return (int)(want < 1 ? 1 : (want > (size_t)kToneSlabRows ? (size_t)kToneSlabRows : want));
}

hipError_t launch_lum_hist(const float4* in, size_t n, uint32_t* slab, int blocks, bool fold, hipStream_t s) {
    if (fold) k_lum_hist<true><<<dim3((unsigned)blocks), dim3(kHistThreads), 0, s>>>(in, n, slab);
    else k_lum_hist<false><<<dim3((unsigned)blocks), dim3(kHistThreads), 0, s>>>(in, n, slab);
    return hipGetLastError();
}

hipError_t launch_meter(const uint32_t* slab, int rows, ToneState* st, const double* lc, const ToneMeter& M, bool run_meter,
                        hipStream_t s) {
    k_meter<<<dim3(1), dim3(kMeterThreads), 0, s>>>(slab, rows, st, lc, M, run_meter ? 1 : 0);
    return hipGetLastError();
}

hipError_t launch_tonemap(const float4* in, float4* out, size_t n, const ToneState* st, float scale, int curve, float iw2,
                          hipStream_t s) {
    const size_t blocks = (n + 255) / 256;
    k_tonemap<<<dim3((unsigned)blocks), dim3(256), 0, s>>>(in, out, n, st, scale, curve, iw2);
    return hipGetLastError();
}

}  // namespace rmr
