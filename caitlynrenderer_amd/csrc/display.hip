// crt_display (include/crt.h): metered auto-exposure, a tone curve and the pinned gamma over one of the scene's float
// images.  Three kernels: k_display_hist counts pixels per luminance bin, k_display_meter (one workgroup) turns the counts into the
// exposure and the state block, k_display writes the RGBA8.
//
// The arithmetic is the contract.  The float steps are one IEEE float32 operation each, in the order written, no contraction
// (-ffp-contract=off), divisions through __fdiv_rn / rcp_ieee.  The meter is integers throughout: a pixel's bin is a shift of its
// luminance's bit pattern, the counts are uint32, the trimmed mean is 64-bit integer arithmetic, and the metered luminance is put
// together from bits, so neither the order of the atomics nor the launch shape can change a bit of the result.  tests/display_ref.py
// states the same in numpy and Python integers and the tests compare bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "display.hpp"
#include "rt_math.hpp"

namespace crt {

namespace {

constexpr uint32_t kNoBin = 0xffffffffu;
constexpr uint32_t kFirstBin = 111u << 3;        // bits(0x1p-16f) >> 20

// local pixel index -> frame pixel, as rt_kernels.hip lays the packed sum out (tile-major; inside a tile 8 x 8 blocks row-major)
__device__ __forceinline__ bool pixel_of(const FrameArgs& f, uint32_t i, uint32_t& px, uint32_t& py) {
    uint32_t t, bx, by;
    const uint32_t k = i & 63u;
    if (f.tile_log2) {
        const uint32_t s2 = 2u * f.tile_log2, sb = f.tile_log2 - 3u;
        t = i >> s2;
        const uint32_t blk = (i & ((1u << s2) - 1u)) >> 6;
        bx = blk & ((1u << sb) - 1u); by = blk >> sb;
    } else {
        const uint32_t tile_px = f.tile * f.tile;
        t = i / tile_px;
        const uint32_t blk = (i - t * tile_px) >> 6, blocks_per_row = f.tile >> 3;
        by = blk / blocks_per_row; bx = blk - by * blocks_per_row;
    }
    const uint2 txy = f.tile_xy[t];
    px = txy.x * f.tile + bx * 8u + (k & 7u);
    py = txy.y * f.tile + by * 8u + (k >> 3);
    return px < f.width && py < f.height;
}

// the resolve's weights and order
__device__ __forceinline__ float luminance(float c0, float c1, float c2) { return (0.3f * c0 + 0.6f * c1) + 0.1f * c2; }

// 256 bins, 8 per octave, from 2^-16 upward; kNoBin for what does not count (NaN, +-inf, zero, negatives, anything below 2^-16)
__device__ __forceinline__ uint32_t bin_of(float L) {
    const uint32_t b = __float_as_uint(L);
    if (!(L >= 0x1p-16f) || b >= 0x7f800000u) return kNoBin;
    return min((b >> 20) - kFirstBin, 255u);
}

template <bool PACKED>
__global__ void __launch_bounds__(256) k_display_hist(FrameArgs f, const float* __restrict__ image, uint32_t n, float inv_count, uint32_t* __restrict__ bins) {
    __shared__ uint32_t lds[256];
    lds[threadIdx.x] = 0u;
    __syncthreads();
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        if (PACKED) { uint32_t px, py; if (!pixel_of(f, i, px, py)) continue; }
        float c0 = image[3 * (size_t)i], c1 = image[3 * (size_t)i + 1], c2 = image[3 * (size_t)i + 2];
        if (PACKED) { c0 = c0 * inv_count; c1 = c1 * inv_count; c2 = c2 * inv_count; }
        const uint32_t k = bin_of(luminance(c0, c1, c2));
        if (k != kNoBin) atomicAdd(&lds[k], 1u);          // one LDS atomic per counted lane: combining equal bins within the wave first lost
    }
    __syncthreads();
    const uint32_t mine = lds[threadIdx.x];
    if (mine) atomicAdd(&bins[(blockIdx.x % kDisplayBinCopies) * 256u + threadIdx.x], mine);
}

// One workgroup of 256: thread t owns bin t.
__global__ void __launch_bounds__(256) k_display_meter(DisplayMeterArgs a) {
    __shared__ uint32_t scan[256];
    __shared__ unsigned long long part[256];
    const uint32_t t = threadIdx.x;
    if (!a.metered) {
        if (t == 0u) {
            a.state[kDisplayExposure] = __float_as_uint(a.exposure);
            a.state[kDisplayMetered] = 0u; a.state[kDisplayCounted] = 0u; a.state[kDisplayQ] = 0u;
        }
        return;
    }
    uint32_t h = 0u;
    for (uint32_t c = 0u; c < kDisplayBinCopies; ++c) h += a.bins[c * 256u + t];
    scan[t] = h;
    __syncthreads();
    for (uint32_t d = 1u; d < 256u; d <<= 1) {             // inclusive prefix sum
        const uint32_t v = t >= d ? scan[t - d] : 0u;
        __syncthreads();
        scan[t] += v;
        __syncthreads();
    }
    const uint64_t N = scan[255];
    const uint64_t lo = N * a.low_permille / 1000u, hi = N * a.high_permille / 1000u;
    // with the counted pixels ordered by bin, bin t holds ranks [incl - h, incl); ranks [lo, hi) are kept
    const uint64_t incl = scan[t], excl = incl - h;
    const uint64_t first = excl > lo ? excl : lo, end = incl < hi ? incl : hi;
    part[t] = end > first ? (end - first) * t : 0ull;
    __syncthreads();
    for (uint32_t d = 128u; d != 0u; d >>= 1) {
        if (t < d) part[t] += part[t + d];
        __syncthreads();
    }
    if (t == 0u) {
        const uint64_t M = hi - lo, S = part[0];
        const uint32_t calls = a.state[kDisplayCalls];
        float E, L_avg = 0.f;
        uint32_t Q = 0u;
        if (M == 0ull) {                                   // nothing metered: the exposure keeps the value it had, or takes params.exposure
            E = calls ? __uint_as_float(a.state[kDisplayAdapted]) : a.exposure;
        } else {
            Q = (uint32_t)(S * 256ull / M) + 128u;
            L_avg = __uint_as_float((kFirstBin << 20) + (Q << 12));
            const float E_target = fminf(fmaxf(__fdiv_rn(a.key, L_avg), a.exposure_min), a.exposure_max);
            if (calls == 0u || a.adapt == 1.0f) E = E_target;
            else {
                const float E_prev = __uint_as_float(a.state[kDisplayAdapted]);
                E = E_prev + (E_target - E_prev) * a.adapt;
            }
            a.state[kDisplayAdapted] = __float_as_uint(E);
            a.state[kDisplayCalls] = calls + 1u;
        }
        a.state[kDisplayExposure] = __float_as_uint(E);
        a.state[kDisplayMetered] = __float_as_uint(L_avg);
        a.state[kDisplayCounted] = (uint32_t)N;
        a.state[kDisplayQ] = Q;
    }
    a.last[t] = h;
    for (uint32_t c = 0u; c < kDisplayBinCopies; ++c) a.bins[c * 256u + t] = 0u;
}

// the byte: thr[1..255] ascending; the largest j with y >= thr[j] (0: none; NaN and negatives: none) — the resolve kernels' eight compares
__device__ __forceinline__ uint32_t gamma_byte(float y, const float* __restrict__ thr) {
    uint32_t lo = 0u;
#pragma unroll
    for (uint32_t step = 128u; step != 0u; step >>= 1)
        if (y >= thr[lo + step]) lo += step;
    return lo;
}

template <int CURVE>
__device__ __forceinline__ uchar4 display_pixel(float c0, float c1, float c2, float E, float w2, const float* __restrict__ thr) {
    const float x0 = c0 * E, x1 = c1 * E, x2 = c2 * E;
    float y0, y1, y2;
    if (CURVE == CRT_DISPLAY_CURVE_REFERENCE) {
        const float k = rcp_ieee(1.0f + __fdiv_rn(luminance(x0, x1, x2), 2.0f));
        y0 = x0 * k; y1 = x1 * k; y2 = x2 * k;
    } else if (CURVE == CRT_DISPLAY_CURVE_REINHARD) {
        const float lum = luminance(x0, x1, x2);
        const float k = __fdiv_rn(1.0f + __fdiv_rn(lum, w2), 1.0f + lum);
        y0 = x0 * k; y1 = x1 * k; y2 = x2 * k;
    } else if (CURVE == CRT_DISPLAY_CURVE_ACES) {
        y0 = __fdiv_rn(x0 * (2.51f * x0 + 0.03f), x0 * (2.43f * x0 + 0.59f) + 0.14f);
        y1 = __fdiv_rn(x1 * (2.51f * x1 + 0.03f), x1 * (2.43f * x1 + 0.59f) + 0.14f);
        y2 = __fdiv_rn(x2 * (2.51f * x2 + 0.03f), x2 * (2.43f * x2 + 0.59f) + 0.14f);
    } else {
        y0 = x0; y1 = x1; y2 = x2;
    }
    return make_uchar4((uint8_t)gamma_byte(y0, thr), (uint8_t)gamma_byte(y1, thr), (uint8_t)gamma_byte(y2, thr), 255);
}

template <int CURVE, bool PACKED>
__global__ void __launch_bounds__(256) k_display(FrameArgs f, const float* __restrict__ image, uint32_t n, float inv_count, float w2,
                                                 const uint32_t* __restrict__ state, const float* __restrict__ thr, uint8_t* __restrict__ rgba) {
    const float E = __uint_as_float(state[kDisplayExposure]);
    // the thresholds staged in LDS: a byte is eight DEPENDENT table reads per channel, and from global memory those chains were half the
    // kernel (25.1 against 12.5 us at 1920 x 1080)
    __shared__ float thr_lds[256];
    thr_lds[threadIdx.x] = thr[threadIdx.x];
    __syncthreads();
    thr = thr_lds;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        size_t o = i;
        if (PACKED) {
            uint32_t px, py;
            if (!pixel_of(f, i, px, py)) continue;
            o = (size_t)py * f.width + px;
        }
        float c0 = image[3 * (size_t)i], c1 = image[3 * (size_t)i + 1], c2 = image[3 * (size_t)i + 2];
        if (PACKED) { c0 = c0 * inv_count; c1 = c1 * inv_count; c2 = c2 * inv_count; }
        reinterpret_cast<uchar4*>(rgba)[o] = display_pixel<CURVE>(c0, c1, c2, E, w2, thr);
    }
}

template <bool PACKED>
void launch_display_form(const DisplaySlice& sl, uint32_t n, float inv_count, uint32_t curve, float w2, const uint32_t* state, const float* thr, uint8_t* rgba,
                         hipStream_t stream) {
    const dim3 grid(sl.grid), block(256);
    switch (curve) {
    case CRT_DISPLAY_CURVE_REFERENCE: hipLaunchKernelGGL((k_display<CRT_DISPLAY_CURVE_REFERENCE, PACKED>), grid, block, 0, stream, sl.f, sl.image, n, inv_count, w2, state, thr, rgba); break;
    case CRT_DISPLAY_CURVE_REINHARD:  hipLaunchKernelGGL((k_display<CRT_DISPLAY_CURVE_REINHARD, PACKED>), grid, block, 0, stream, sl.f, sl.image, n, inv_count, w2, state, thr, rgba); break;
    case CRT_DISPLAY_CURVE_ACES:      hipLaunchKernelGGL((k_display<CRT_DISPLAY_CURVE_ACES, PACKED>), grid, block, 0, stream, sl.f, sl.image, n, inv_count, w2, state, thr, rgba); break;
    default:                          hipLaunchKernelGGL((k_display<CRT_DISPLAY_CURVE_CLAMP, PACKED>), grid, block, 0, stream, sl.f, sl.image, n, inv_count, w2, state, thr, rgba); break;
    }
}

}  // namespace

// the running sum is the packed, scaled form; the denoised and the accumulated image are linear and taken as they are
void launch_display_hist(const DisplaySlice& sl, float inv_count, uint32_t* bins, hipStream_t stream) {
    if (sl.packed) hipLaunchKernelGGL(k_display_hist<true>, dim3(sl.grid), dim3(256), 0, stream, sl.f, sl.image, sl.f.n_local_pixels, inv_count, bins);
    else hipLaunchKernelGGL(k_display_hist<false>, dim3(sl.grid), dim3(256), 0, stream, sl.f, sl.image, sl.n_pixels, inv_count, bins);
}
void launch_display_meter(const DisplayMeterArgs& a, hipStream_t stream) { hipLaunchKernelGGL(k_display_meter, dim3(1), dim3(256), 0, stream, a); }
void launch_display(const DisplaySlice& sl, float inv_count, uint32_t curve, float w2, const uint32_t* state, const float* thr, uint8_t* rgba, hipStream_t stream) {
    if (sl.packed) launch_display_form<true>(sl, sl.f.n_local_pixels, inv_count, curve, w2, state, thr, rgba, stream);
    else launch_display_form<false>(sl, sl.n_pixels, inv_count, curve, w2, state, thr, rgba, stream);
}

}  // namespace crt
