// crt_denoise (include/crt.h): an edge-avoiding a-trous wavelet filter over the un-tiled sum, guided by the first-hit
// feature buffers.  Two kernels: k_denoise_prepare turns the sum and four AOV channels into two float4 records per pixel, G = (unit
// normal, t) and X = (x, key); k_denoise_pass runs one pass of tap spacing s = 2^i, X -> X', and the last pass writes the 3-float image.
//
// The arithmetic is the contract: every step is one IEEE float32 operation, evaluated in the order written, no contraction
// (-ffp-contract=off), divisions and roots through __fdiv_rn / rcp_ieee / sqrt_ieee.  tests/denoise_ref.py states the same in numpy and the
// tests compare bytes, so an "equivalent" rewrite of an expression here is a change of the result.
//
// The taps of spacing s never leave the pixel's residue class (px mod s, py mod s), and inside a class the filter is a dense 5 x 5.  So a
// workgroup takes a 16 x 16 block of ONE class, stages the block's (16 + 4)^2 records in LDS once and reads its 25 taps from there: the
// same kernel for every s.  A record outside the frame is staged with key 0, which no filterable pixel has, so "outside", "not filterable"
// and "another instance" are one compare.  The other form reads every tap from global memory through L1 / L2 (a 16 x 16 block of the FRAME
// per workgroup).  Both give the same bytes; which one a pass runs is a matter of speed alone: measured at 1920 x 1080 the
// staged form wins at s = 1, 2, 16, 32 and the direct one at s = 4, 8.  Option "denoise_form" 1 / 2 runs the staged / the direct form at
// every s (what the tests and tools/denoise_probe.py use); -DCRT_DENOISE_FORM=1 / 2 builds a library whose default that is.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "denoise.hpp"
#include "rt_math.hpp"

namespace crt {

namespace {

constexpr int kBlock = 16;                      // a workgroup's block of a class is kBlock x kBlock pixels, one lane each
constexpr int kHalo = kBlock + 4;
// records per staged row.  CRT_DENOISE_ROW 32 (a multiple of the 256-byte bank row) was measured against the dense 20 and is no faster: the
// staged passes are not LDS-bound
#ifndef CRT_DENOISE_ROW
#define CRT_DENOISE_ROW 20
#endif
constexpr int kRow = CRT_DENOISE_ROW;
static_assert(kRow >= kHalo, "a staged row holds the block and its halo");

__global__ __launch_bounds__(256) void k_denoise_prepare(DenoisePrepareArgs a) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= a.n_pixels) return;
    const float c0 = a.sum[3u * p + 0u] * a.inv_count, c1 = a.sum[3u * p + 1u] * a.inv_count, c2 = a.sum[3u * p + 2u] * a.inv_count;
    const float4 hit = a.hit[p];
    const int4 ids = a.ids[p];
    const float4 n = a.normal[p];
    const float nn = (n.x * n.x + n.y * n.y) + n.z * n.z;
    const bool filterable = __float_as_int(hit.w) >= 0 && hit.x >= 1e-20f && (ids.w & 2) == 0 && nn > 0.f && nn < __builtin_inff();
    if (!filterable) {
        a.g[p] = make_float4(0.f, 0.f, 0.f, 0.f);
        a.x[p] = make_float4(c0, c1, c2, 0.f);
        return;
    }
    const float r = rcp_ieee(sqrt_ieee(nn));
    float x0 = c0, x1 = c1, x2 = c2;
    if (a.demodulate) {
        const float4 al = a.albedo[p];
        x0 = __fdiv_rn(c0, fmaxf(al.x, 1e-3f));
        x1 = __fdiv_rn(c1, fmaxf(al.y, 1e-3f));
        x2 = __fdiv_rn(c2, fmaxf(al.z, 1e-3f));
    }
    a.g[p] = make_float4(n.x * r, n.y * r, n.z * r, hit.x);
    a.x[p] = make_float4(x0, x1, x2, __uint_as_float((uint32_t)ids.x + 1u));
}

// What a filterable pixel p accumulates over its 25 taps; `tap(dx, dy, g, x)` fetches the records of the pixel (dx, dy) class steps away
// (key 0 when it lies outside the frame).
template <typename Tap>
__device__ __forceinline__ float4 filter_pixel(const DenoisePassArgs& a, const float4 gp, const float4 xp, Tap tap) {
    const float kk[3] = {0.375f, 0.25f, 0.0625f};
    const float r1 = rcp_ieee((a.sigma_depth * gp.w) * (float)(1u << a.step_log2));
    const float r2 = r1 * 0.5f;
    float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f, sw = 0.f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            float4 gq, xq;
            tap(dx, dy, gq, xq);
            if (__float_as_uint(xq.w) != __float_as_uint(xp.w)) continue;
            const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy, m = ax > ay ? ax : ay;
            float w = kk[ax] * kk[ay];
            float nd = fmaxf((gp.x * gq.x + gp.y * gq.y) + gp.z * gq.z, 0.f);
            for (uint32_t k = 0; k < a.normal_squarings; ++k) nd = nd * nd;
            w = w * nd;
            if (m > 0) {
                const float z = __builtin_fabsf(gp.w - gq.w) * (m == 1 ? r1 : r2);
                const float g = fmaxf(1.0f - z * z, 0.f);
                w = w * (g * g);
            }
            if (a.use_color) {
                const float e0 = xp.x - xq.x, e1 = xp.y - xq.y, e2 = xp.z - xq.z;
                const float d2 = (e0 * e0 + e1 * e1) + e2 * e2;
                const float g = fmaxf(1.0f - d2 * a.inv_c, 0.f);
                w = w * (g * g);
            }
            acc0 = acc0 + w * xq.x; acc1 = acc1 + w * xq.y; acc2 = acc2 + w * xq.z;
            sw = sw + w;
        }
    }
    return make_float4(__fdiv_rn(acc0, sw), __fdiv_rn(acc1, sw), __fdiv_rn(acc2, sw), xp.w);
}

template <bool LAST>
__device__ __forceinline__ void write_pixel(const DenoisePassArgs& a, uint32_t p, float4 x) {
    if (!LAST) { a.x_out[p] = x; return; }
    if (a.demodulate && __float_as_uint(x.w) != 0u) {
        const float4 al = a.albedo[p];
        x.x = x.x * fmaxf(al.x, 1e-3f); x.y = x.y * fmaxf(al.y, 1e-3f); x.z = x.z * fmaxf(al.z, 1e-3f);
    }
    a.out[3u * p + 0u] = x.x; a.out[3u * p + 1u] = x.y; a.out[3u * p + 2u] = x.z;
}

// the form a pass runs when option "denoise_form" is 0: 0 = per tap spacing as measured, 1 = staged at every spacing, 2 = direct at every spacing
#ifndef CRT_DENOISE_FORM
#define CRT_DENOISE_FORM 0
#endif

// grid (blocks across the widest class, blocks down the tallest class, s * s classes).  The classes differ in size when s does not divide
// the frame: a block beyond its class returns, a lane beyond it idles behind the barrier.
template <bool LAST>
__global__ __launch_bounds__(256) void k_denoise_pass_staged(DenoisePassArgs a) {
    __shared__ float4 s_g[kHalo * kRow];
    __shared__ float4 s_x[kHalo * kRow];
    const uint32_t s = 1u << a.step_log2;
    const uint32_t cx = blockIdx.z & (s - 1u), cy = blockIdx.z >> a.step_log2;
    if (cx >= a.width || cy >= a.height) return;                                  // an empty class (s beyond the frame)
    const uint32_t cw = (a.width - cx + s - 1u) >> a.step_log2, ch = (a.height - cy + s - 1u) >> a.step_log2;   // the class's size
    const uint32_t u0 = blockIdx.x * kBlock, v0 = blockIdx.y * kBlock;
    if (u0 >= cw || v0 >= ch) return;
    for (uint32_t i = threadIdx.x; i < (uint32_t)(kHalo * kHalo); i += 256u) {
        const uint32_t hy = i / kHalo, hx = i - hy * kHalo;
        const int u = (int)(u0 + hx) - 2, v = (int)(v0 + hy) - 2;
        float4 g = make_float4(0.f, 0.f, 0.f, 0.f), x = make_float4(0.f, 0.f, 0.f, 0.f);
        if (u >= 0 && v >= 0 && (uint32_t)u < cw && (uint32_t)v < ch) {
            const uint32_t q = (cy + ((uint32_t)v << a.step_log2)) * a.width + (cx + ((uint32_t)u << a.step_log2));
            g = a.g[q];
            x = a.x_in[q];
        }
        s_g[hy * kRow + hx] = g;
        s_x[hy * kRow + hx] = x;
    }
    __syncthreads();
    const uint32_t lx = threadIdx.x & 15u, ly = threadIdx.x >> 4;
    if (u0 + lx >= cw || v0 + ly >= ch) return;
    const uint32_t p = (cy + ((v0 + ly) << a.step_log2)) * a.width + (cx + ((u0 + lx) << a.step_log2));
    const int centre = (int)((ly + 2u) * kRow + lx + 2u);
    float4 x = s_x[centre];
    if (__float_as_uint(x.w) != 0u)
        x = filter_pixel(a, s_g[centre], x, [&](int dx, int dy, float4& gq, float4& xq) {
            xq = s_x[centre + dy * kRow + dx];
            gq = s_g[centre + dy * kRow + dx];
        });
    write_pixel<LAST>(a, p, x);
}
static dim3 staged_grid(const DenoisePassArgs& a) {
    const uint32_t s = 1u << a.step_log2;
    const uint32_t cw = (a.width + s - 1u) >> a.step_log2, ch = (a.height + s - 1u) >> a.step_log2;
    return dim3((cw + kBlock - 1u) / kBlock, (ch + kBlock - 1u) / kBlock, s * s);
}

// the direct form: a 16 x 16 block of the frame per workgroup, every tap two 16-byte loads from global memory
template <bool LAST>
__global__ __launch_bounds__(256) void k_denoise_pass_direct(DenoisePassArgs a) {
    const uint32_t px = blockIdx.x * kBlock + (threadIdx.x & 15u), py = blockIdx.y * kBlock + (threadIdx.x >> 4);
    if (px >= a.width || py >= a.height) return;
    const uint32_t p = py * a.width + px;
    float4 x = a.x_in[p];
    if (__float_as_uint(x.w) != 0u)
        x = filter_pixel(a, a.g[p], x, [&](int dx, int dy, float4& gq, float4& xq) {
            const int qx = (int)px + dx * (int)(1u << a.step_log2), qy = (int)py + dy * (int)(1u << a.step_log2);
            gq = make_float4(0.f, 0.f, 0.f, 0.f); xq = make_float4(0.f, 0.f, 0.f, 0.f);
            if (qx >= 0 && qy >= 0 && (uint32_t)qx < a.width && (uint32_t)qy < a.height) {
                const uint32_t q = (uint32_t)qy * a.width + (uint32_t)qx;
                xq = a.x_in[q];
                gq = a.g[q];
            }
        });
    write_pixel<LAST>(a, p, x);
}
static dim3 direct_grid(const DenoisePassArgs& a) { return dim3((a.width + kBlock - 1u) / kBlock, (a.height + kBlock - 1u) / kBlock, 1u); }

static bool runs_direct(uint32_t form, uint32_t step_log2) {
    if (form == 0u) form = CRT_DENOISE_FORM;
    return form == 2u || (form == 0u && (step_log2 == 2u || step_log2 == 3u));
}

}  // namespace

void launch_denoise_prepare(const DenoisePrepareArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(k_denoise_prepare, dim3((a.n_pixels + 255u) / 256u), dim3(256), 0, stream, a);
}
void launch_denoise_pass(const DenoisePassArgs& a, bool last, uint32_t form, hipStream_t stream) {
    if (runs_direct(form, a.step_log2)) {
        if (last) hipLaunchKernelGGL(k_denoise_pass_direct<true>, direct_grid(a), dim3(256), 0, stream, a);
        else      hipLaunchKernelGGL(k_denoise_pass_direct<false>, direct_grid(a), dim3(256), 0, stream, a);
    } else {
        if (last) hipLaunchKernelGGL(k_denoise_pass_staged<true>, staged_grid(a), dim3(256), 0, stream, a);
        else      hipLaunchKernelGGL(k_denoise_pass_staged<false>, staged_grid(a), dim3(256), 0, stream, a);
    }
}
int warm_denoise_kernels() {
    hipFuncAttributes a;
    hipError_t e;
    if ((e = hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_denoise_prepare))) != hipSuccess) return (int)e;
    if ((e = hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_denoise_pass_staged<false>))) != hipSuccess) return (int)e;
    if ((e = hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_denoise_pass_direct<false>))) != hipSuccess) return (int)e;
    return 0;
}

}  // namespace crt
