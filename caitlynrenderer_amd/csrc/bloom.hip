// crt_bloom (include/crt.h): the bright part of a float image filtered down an image pyramid, blended back up it and
// put on the image.  k_bloom_down<true> scales, bright-passes and filters to level 1, k_bloom_down<false> makes each further level,
// k_bloom_up blends a level with the one below it, k_bloom_composite is the last Up and the blend with the image.
//
// The arithmetic is the contract.  Every step is one IEEE float32 operation in the header's order, no contraction (-ffp-contract=off),
// the one division through __fdiv_rn.  Both filters are separable and defined horizontal first: a thread computes the horizontal
// results of the rows it needs and filters those vertically, which are the same operations on the same operands as two passes over
// whole levels, so no tiling can change a bit.  tests/bloom_ref.py states the same in numpy and the tests compare bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bloom.hpp"

namespace crt {

namespace {

struct Px { float x, y, z; };      // 12 bytes at 4-byte alignment: one global_load_dwordx3

__device__ __forceinline__ Px add(Px a, Px b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ Px sub(Px a, Px b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ Px mul(Px a, float k) { return {a.x * k, a.y * k, a.z * k}; }

__device__ __forceinline__ Px load_px(const float* __restrict__ p, uint32_t i) { return reinterpret_cast<const Px*>(p)[i]; }
__device__ __forceinline__ void store_px(float* __restrict__ p, uint32_t i, Px v) { reinterpret_cast<Px*>(p)[i] = v; }

// c: the image times inv_count for the running sum, the image itself otherwise
__device__ __forceinline__ Px input_px(const BloomSource& s, uint32_t i) {
    Px c = load_px(s.image, i);
    if (s.scale) c = mul(c, s.inv_count);
    return c;
}

// b = c * k, k = max(min(L, clamp) - threshold, 0) / max(L, 2^-16), 0 where not L > 0
__device__ __forceinline__ Px bright_px(const BloomSource& s, uint32_t i) {
    const Px c = input_px(s, i);
    const float L = (0.3f * c.x + 0.6f * c.y) + 0.1f * c.z;
    const float Lc = s.clamp == 0.0f ? L : fminf(L, s.clamp);
    float k = __fdiv_rn(fmaxf(Lc - s.threshold, 0.0f), fmaxf(L, 0x1p-16f));
    if (!(L > 0.0f)) k = 0.0f;
    return mul(c, k);
}

// one tap row of Down: ((a[x0-1] + a[x0+2]) + 3 * (a[x0] + a[x0+1])) * 0.125, indices clamped to the row
template <typename Load>
__device__ __forceinline__ Px down_row(Load ld, uint32_t x, uint32_t row, uint32_t w) {
    const uint32_t x0 = 2u * x, xm = x0 ? x0 - 1u : 0u, x1 = min(x0 + 1u, w - 1u), x2 = min(x0 + 2u, w - 1u);
    return mul(add(add(ld(xm, row), ld(x2, row)), mul(add(ld(x0, row), ld(x1, row)), 3.0f)), 0.125f);
}

// pixel (x, y) of Down(a), a of w x h read through ld(x, y)
template <typename Load>
__device__ __forceinline__ Px down_at(Load ld, uint32_t x, uint32_t y, uint32_t w, uint32_t h) {
    const uint32_t y0 = 2u * y, ym = y0 ? y0 - 1u : 0u, y1 = min(y0 + 1u, h - 1u), y2 = min(y0 + 2u, h - 1u);
    const Px rm = down_row(ld, x, ym, w), r0 = down_row(ld, x, y0, w), r1 = down_row(ld, x, y1, w), r2 = down_row(ld, x, y2, w);
    return mul(add(add(rm, r2), mul(add(r0, r1), 3.0f)), 0.125f);
}

// pixel (x, y) of Up(a), a of ws x hs read through ld(x, y): a[near] * 0.75 + a[far] * 0.25 along x, then along y
template <typename Load>
__device__ __forceinline__ Px up_at(Load ld, uint32_t x, uint32_t y, uint32_t ws, uint32_t hs) {
    const uint32_t nx = x >> 1, fx = (x & 1u) ? min(nx + 1u, ws - 1u) : (nx ? nx - 1u : 0u);
    const uint32_t ny = y >> 1, fy = (y & 1u) ? min(ny + 1u, hs - 1u) : (ny ? ny - 1u : 0u);
    const Px rn = add(mul(ld(nx, ny), 0.75f), mul(ld(fx, ny), 0.25f));
    const Px rf = add(mul(ld(nx, fy), 0.75f), mul(ld(fx, fy), 0.25f));
    return add(mul(rn, 0.75f), mul(rf, 0.25f));
}

constexpr uint32_t kBlockX = 32, kBlockY = 8;

dim3 grid_of(uint32_t w, uint32_t h) { return dim3((w + kBlockX - 1u) / kBlockX, (h + kBlockY - 1u) / kBlockY); }

// a thread per pixel of the child level; w x h is the parent
template <bool FIRST>
__global__ void __launch_bounds__(256) k_bloom_down(BloomSource s, const float* __restrict__ parent, uint32_t w, uint32_t h, float* __restrict__ child) {
    const uint32_t cw = (w + 1u) >> 1, ch = (h + 1u) >> 1;
    const uint32_t x = blockIdx.x * kBlockX + threadIdx.x, y = blockIdx.y * kBlockY + threadIdx.y;
    if (x >= cw || y >= ch) return;
    Px v;
    if (FIRST) v = down_at([&](uint32_t xx, uint32_t yy) { return bright_px(s, yy * w + xx); }, x, y, w, h);
    else v = down_at([&](uint32_t xx, uint32_t yy) { return load_px(parent, yy * w + xx); }, x, y, w, h);
    store_px(child, y * cw + x, v);
}

__global__ void __launch_bounds__(256) k_bloom_up(const float* __restrict__ coarse, float* __restrict__ level, uint32_t w, uint32_t h, float scatter) {
    const uint32_t ws = (w + 1u) >> 1, hs = (h + 1u) >> 1;
    const uint32_t x = blockIdx.x * kBlockX + threadIdx.x, y = blockIdx.y * kBlockY + threadIdx.y;
    if (x >= w || y >= h) return;
    const Px up = up_at([&](uint32_t xx, uint32_t yy) { return load_px(coarse, yy * ws + xx); }, x, y, ws, hs);
    const Px d = load_px(level, y * w + x);
    store_px(level, y * w + x, add(d, mul(sub(up, d), scatter)));
}

template <bool CONSERVE>
__global__ void __launch_bounds__(256) k_bloom_composite(BloomSource s, const float* __restrict__ u1, float strength, float* __restrict__ out) {
    const uint32_t w = s.width, h = s.height, ws = (w + 1u) >> 1, hs = (h + 1u) >> 1;
    const uint32_t x = blockIdx.x * kBlockX + threadIdx.x, y = blockIdx.y * kBlockY + threadIdx.y;
    if (x >= w || y >= h) return;
    const Px G = up_at([&](uint32_t xx, uint32_t yy) { return load_px(u1, yy * ws + xx); }, x, y, ws, hs);
    const Px c = input_px(s, y * w + x);
    store_px(out, y * w + x, CONSERVE ? add(c, mul(sub(G, c), strength)) : add(c, mul(G, strength)));
}

__global__ void __launch_bounds__(256) k_bloom_copy(BloomSource s, uint32_t n, float* __restrict__ out) {
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) store_px(out, i, input_px(s, i));
}

}  // namespace

void launch_bloom_down_first(const BloomSource& src, float* d1, hipStream_t stream) {
    hipLaunchKernelGGL(k_bloom_down<true>, grid_of((src.width + 1u) >> 1, (src.height + 1u) >> 1), dim3(kBlockX, kBlockY), 0, stream, src, src.image,
                       src.width, src.height, d1);
}

void launch_bloom_down(const float* parent, uint32_t w, uint32_t h, float* child, hipStream_t stream) {
    hipLaunchKernelGGL(k_bloom_down<false>, grid_of((w + 1u) >> 1, (h + 1u) >> 1), dim3(kBlockX, kBlockY), 0, stream, BloomSource{}, parent, w, h, child);
}

void launch_bloom_up(const float* coarse, float* level, uint32_t w, uint32_t h, float scatter, hipStream_t stream) {
    hipLaunchKernelGGL(k_bloom_up, grid_of(w, h), dim3(kBlockX, kBlockY), 0, stream, coarse, level, w, h, scatter);
}

void launch_bloom_composite(const BloomSource& src, const float* u1, uint32_t conserve, float strength, float* out, hipStream_t stream) {
    const dim3 grid = grid_of(src.width, src.height), block(kBlockX, kBlockY);
    if (conserve) hipLaunchKernelGGL(k_bloom_composite<true>, grid, block, 0, stream, src, u1, strength, out);
    else hipLaunchKernelGGL(k_bloom_composite<false>, grid, block, 0, stream, src, u1, strength, out);
}

void launch_bloom_copy(const BloomSource& src, float* out, hipStream_t stream) {
    const uint32_t n = src.width * src.height;
    hipLaunchKernelGGL(k_bloom_copy, dim3(min((n + 255u) / 256u, 2048u)), dim3(256), 0, stream, src, n, out);
}

}  // namespace crt
