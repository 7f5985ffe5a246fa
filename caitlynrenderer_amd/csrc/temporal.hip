// crt_temporal (include/crt.h): temporal accumulation by reprojection, one kernel per call, one lane per pixel, a 16 x 16
// pixel block per workgroup so that the four gathered taps of neighbouring lanes share cache lines.
//
// The arithmetic is the contract, as in denoise.hip: every step is one IEEE float32 operation, evaluated in the order written, no
// contraction (-ffp-contract=off), divisions and roots through __fdiv_rn / rcp_ieee / sqrt_ieee.  tests/temporal_ref.py states the same
// in numpy and the tests compare bytes, so an "equivalent" rewrite of an expression here is a change of the result.
//
// What varies per call but not per lane is decided on kernel arguments (history or none, flat or instanced, CLAMP, DEMODULATE): those
// branches are wave-uniform.  An instanced pixel compares its instance's 12 current object_to_world words with the previous ones (six
// 16-byte loads that a wave's lanes mostly share) and only a moved instance pays the two matrix products.
//
// CLAMP needs x of the eight neighbours, and x is a function of five input arrays.  Two forms: the workgroup computes the (16 + 2)^2
// values of its block once into LDS (staged), or each lane computes its neighbours' from global memory (direct).  The same bytes;
// DESIGN.md §23 has both times.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_math.hpp"
#include "temporal.hpp"

namespace crt {

namespace {

constexpr int kBlock = 16;
constexpr int kHalo = kBlock + 2;

// what the definition's step 1 gives for pixel p: x and the key (0 = not F) in .w of the result; for the centre also the divisor and the guide
struct Source {
    float4 xk;                   // (x, key as bits)
    float m0, m1, m2;            // the divisor: max(albedo, 1e-3) when F and DEMODULATE, else 1
    float4 g;                    // (unit normal, t); zeros when not F
    int inst;
};

__device__ __forceinline__ Source source_of(const TemporalArgs& a, uint32_t p) {
    Source s;
    float c0 = a.src[3u * p + 0u], c1 = a.src[3u * p + 1u], c2 = a.src[3u * p + 2u];
    if (a.scale_source) { c0 = c0 * a.inv_count; c1 = c1 * a.inv_count; c2 = c2 * a.inv_count; }
    const float4 hit = a.hit[p];
    const int4 ids = a.ids[p];
    const float4 n = a.normal[p];
    const float nn = (n.x * n.x + n.y * n.y) + n.z * n.z;
    const bool F = __float_as_int(hit.w) >= 0 && hit.x >= 1e-20f && (ids.w & 2) == 0 && nn > 0.f && nn < __builtin_inff();
    s.m0 = s.m1 = s.m2 = 1.0f;
    s.inst = ids.x;
    if (!F) {
        s.xk = make_float4(c0, c1, c2, 0.f);
        s.g = make_float4(0.f, 0.f, 0.f, 0.f);
        return s;
    }
    const float r = rcp_ieee(sqrt_ieee(nn));
    s.g = make_float4(n.x * r, n.y * r, n.z * r, hit.x);
    if (a.demodulate) {
        const float4 al = a.albedo[p];
        s.m0 = fmaxf(al.x, 1e-3f); s.m1 = fmaxf(al.y, 1e-3f); s.m2 = fmaxf(al.z, 1e-3f);
        c0 = __fdiv_rn(c0, s.m0); c1 = __fdiv_rn(c1, s.m1); c2 = __fdiv_rn(c2, s.m2);
    }
    s.xk = make_float4(c0, c1, c2, __uint_as_float((uint32_t)ids.x + 1u));
    return s;
}

// the primary-ray direction of view v at pixel (px, py): rt_kernels.hip's primary_ray, restated operation for operation
__device__ __forceinline__ vec3 view_direction(const TemporalView& v, uint32_t px, uint32_t py, float W, float H) {
    float sx = (float)px + 0.5f, sy = (float)py + 0.5f;
    float jx = 0.f, jy = 0.f;
    if (v.jitter) {
        const float r1 = 2.0f * shader_rand(sx, sy, v.rv);
        const float r2 = 2.0f * shader_rand(sx, sy, v.rv);
        jx = r1 < 1.0f ? sqrt_ieee(r1) - 1.0f : 1.0f - sqrt_ieee(2.0f - r1);
        jy = r2 < 1.0f ? sqrt_ieee(r2) - 1.0f : 1.0f - sqrt_ieee(2.0f - r2);
        jx = __fdiv_rn(jx, W * 0.5f);
        jy = __fdiv_rn(jy, H * 0.5f);
    }
    const float tx = __fdiv_rn((float)px + 0.5f, W), ty = __fdiv_rn((float)py + 0.5f, H);
    float dx = (2.0f * tx - 1.0f) + jx;
    float dy = (2.0f * ty - 1.0f) + jy;
    dx = dx * v.aspect_tan;
    dy = dy * v.tan_fov;
    const vec3 right = V3(v.right[0], v.right[1], v.right[2]);
    const vec3 up = V3(v.up[0], v.up[1], v.up[2]);
    const vec3 fwd = V3(v.fwd[0], v.fwd[1], v.fwd[2]);
    return normalize((right * dx + up * dy) + fwd);
}

// one row of a 3 x 4 matrix (12 floats, row-major) applied to a point
__device__ __forceinline__ float row_point(const float4 m, const vec3 a) { return ((m.x * a.x + m.y * a.y) + m.z * a.z) + m.w; }

__device__ __forceinline__ bool same_words(const float4 a, const float4 b) {
    return __float_as_uint(a.x) == __float_as_uint(b.x) && __float_as_uint(a.y) == __float_as_uint(b.y) &&
           __float_as_uint(a.z) == __float_as_uint(b.z) && __float_as_uint(a.w) == __float_as_uint(b.w);
}

// steps 3 - 7 of the definition for an F pixel: whether there is history, and (h, nh) if so
__device__ __forceinline__ bool gather_history(const TemporalArgs& a, uint32_t px, uint32_t py, const Source& s, float4& h) {
    const float W = (float)a.width, H = (float)a.height;
    const vec3 d = view_direction(a.cur, px, py, W, H);
    const float t = s.g.w;
    vec3 X = V3(a.cur.pos[0] + d.x * t, a.cur.pos[1] + d.y * t, a.cur.pos[2] + d.z * t);
    if (a.o2w) {
        const uint32_t i = (uint32_t)s.inst;
        if (i >= a.n_prev_instances || i >= a.n_instances) return false;
        const float4* const cur = reinterpret_cast<const float4*>(a.o2w) + 3u * i;
        const float4* const prev = reinterpret_cast<const float4*>(a.o2w_prev) + 3u * i;
        const float4 p0 = prev[0], p1 = prev[1], p2 = prev[2];
        if (!(same_words(cur[0], p0) && same_words(cur[1], p1) && same_words(cur[2], p2))) {
            const float4* const inv = reinterpret_cast<const float4*>(a.w2o) + 3u * i;
            const vec3 Y = V3(row_point(inv[0], X), row_point(inv[1], X), row_point(inv[2], X));
            X = V3(row_point(p0, Y), row_point(p1, Y), row_point(p2, Y));
        }
    }
    const vec3 v = V3(X.x - a.prev.pos[0], X.y - a.prev.pos[1], X.z - a.prev.pos[2]);
    const float cz = dot(v, V3(a.prev.fwd[0], a.prev.fwd[1], a.prev.fwd[2]));
    const float cx = dot(v, V3(a.prev.right[0], a.prev.right[1], a.prev.right[2]));
    const float cy = dot(v, V3(a.prev.up[0], a.prev.up[1], a.prev.up[2]));
    if (!(cz > 0.f)) return false;
    const float tp = sqrt_ieee(dot(v, v));
    const float fx = ((__fdiv_rn(__fdiv_rn(cx, cz), a.prev.aspect_tan) + 1.0f) * 0.5f) * W - 0.5f;
    const float fy = ((__fdiv_rn(__fdiv_rn(cy, cz), a.prev.tan_fov) + 1.0f) * 0.5f) * H - 0.5f;
    if (!(fx > -1.0f && fx < W && fy > -1.0f && fy < H)) return false;
    const float x0 = __builtin_floorf(fx), y0 = __builtin_floorf(fy);
    const float ax = fx - x0, ay = fy - y0;
    const float wx[2] = {1.0f - ax, ax}, wy[2] = {1.0f - ay, ay};
    const int ix = (int)x0, iy = (int)y0;
    const float tol = a.sigma_depth * tp;
    const uint32_t key = __float_as_uint(s.xk.w);
    float sw = 0.f, acc0 = 0.f, acc1 = 0.f, acc2 = 0.f, an = 0.f;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int qx = ix + i, qy = iy + j;
            if (qx < 0 || qy < 0 || (uint32_t)qx >= a.width || (uint32_t)qy >= a.height) continue;
            const uint32_t q = (uint32_t)qy * a.width + (uint32_t)qx;
            if (a.key_in[q] != key) continue;
            const float4 gq = a.guide_in[q];
            if (!((s.g.x * gq.x + s.g.y * gq.y) + s.g.z * gq.z >= a.normal_min)) continue;
            if (!(__builtin_fabsf(gq.w - tp) <= tol)) continue;
            const float4 hq = a.hist_in[q];
            const float b = wx[i] * wy[j];
            sw = sw + b;
            acc0 = acc0 + b * hq.x; acc1 = acc1 + b * hq.y; acc2 = acc2 + b * hq.z;
            an = an + b * hq.w;
        }
    }
    if (!(sw >= 0.01f)) return false;
    h = make_float4(__fdiv_rn(acc0, sw), __fdiv_rn(acc1, sw), __fdiv_rn(acc2, sw), __fdiv_rn(an, sw));
    return true;
}

// steps 9 - 10
__device__ __forceinline__ void blend_and_store(const TemporalArgs& a, uint32_t p, const Source& s, bool have, const float4 h) {
    float y0 = s.xk.x, y1 = s.xk.y, y2 = s.xk.z, N = 1.0f;
    if (have) {
        N = fminf(h.w + 1.0f, a.max_history);
        const float w = __fdiv_rn(1.0f, N);
        y0 = h.x + w * (s.xk.x - h.x); y1 = h.y + w * (s.xk.y - h.y); y2 = h.z + w * (s.xk.z - h.z);
    }
    a.hist_out[p] = make_float4(y0, y1, y2, N);
    a.guide_out[p] = s.g;
    a.key_out[p] = __float_as_uint(s.xk.w);
    a.out[3u * p + 0u] = y0 * s.m0; a.out[3u * p + 1u] = y1 * s.m1; a.out[3u * p + 2u] = y2 * s.m2;
}

__device__ __forceinline__ void clamp_by(float4& lo, float4& hi, const float4 xq) {
    lo.x = fminf(lo.x, xq.x); lo.y = fminf(lo.y, xq.y); lo.z = fminf(lo.z, xq.z);
    hi.x = fmaxf(hi.x, xq.x); hi.y = fmaxf(hi.y, xq.y); hi.z = fmaxf(hi.z, xq.z);
}

template <bool STAGED>
__global__ __launch_bounds__(256) void k_temporal(TemporalArgs a) {
    __shared__ float4 s_x[STAGED ? kHalo * kHalo : 1];
    const uint32_t bx = blockIdx.x * kBlock, by = blockIdx.y * kBlock;
    const uint32_t lx = threadIdx.x & 15u, ly = threadIdx.x >> 4;
    const uint32_t px = bx + lx, py = by + ly;
    const bool neighbourhood = a.clamp && a.has_history;
    if (STAGED && neighbourhood) {
        for (uint32_t i = threadIdx.x; i < (uint32_t)(kHalo * kHalo); i += 256u) {
            const uint32_t hy = i / kHalo, hx = i - hy * kHalo;
            const int qx = (int)(bx + hx) - 1, qy = (int)(by + hy) - 1;
            float4 xk = make_float4(0.f, 0.f, 0.f, 0.f);                      // key 0: outside the frame or not F, never a neighbour
            if (qx >= 0 && qy >= 0 && (uint32_t)qx < a.width && (uint32_t)qy < a.height) xk = source_of(a, (uint32_t)qy * a.width + (uint32_t)qx).xk;
            s_x[STAGED ? i : 0] = xk;
        }
        __syncthreads();
    }
    if (px >= a.width || py >= a.height) return;
    const uint32_t p = py * a.width + px;
    const Source s = source_of(a, p);
    float4 h = make_float4(0.f, 0.f, 0.f, 0.f);
    bool have = false;
    if (a.has_history && __float_as_uint(s.xk.w) != 0u) have = gather_history(a, px, py, s, h);
    if (have && a.clamp) {
        float4 lo = s.xk, hi = s.xk;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                if (dx == 0 && dy == 0) continue;
                float4 xq;
                if (STAGED) {
                    xq = s_x[STAGED ? (int)((ly + 1u) * kHalo + lx + 1u) + dy * kHalo + dx : 0];
                } else {
                    const int qx = (int)px + dx, qy = (int)py + dy;
                    if (qx < 0 || qy < 0 || (uint32_t)qx >= a.width || (uint32_t)qy >= a.height) continue;
                    xq = source_of(a, (uint32_t)qy * a.width + (uint32_t)qx).xk;
                }
                if (__float_as_uint(xq.w) == __float_as_uint(s.xk.w)) clamp_by(lo, hi, xq);
            }
        }
        h.x = fminf(fmaxf(h.x, lo.x), hi.x); h.y = fminf(fmaxf(h.y, lo.y), hi.y); h.z = fminf(fmaxf(h.z, lo.z), hi.z);
    }
    blend_and_store(a, p, s, have, h);
}

// the form a CLAMP call runs when option "temporal_form" is 0: 1 = staged, 2 = direct (DESIGN.md §23 has the measurement)
#ifndef CRT_TEMPORAL_FORM
#define CRT_TEMPORAL_FORM 1
#endif

}  // namespace

void launch_temporal(const TemporalArgs& a, uint32_t form, hipStream_t stream) {
    if (form == 0u) form = CRT_TEMPORAL_FORM;
    const dim3 grid((a.width + kBlock - 1u) / kBlock, (a.height + kBlock - 1u) / kBlock, 1u);
    if (form == 1u && a.clamp && a.has_history) hipLaunchKernelGGL(k_temporal<true>, grid, dim3(256), 0, stream, a);
    else                                        hipLaunchKernelGGL(k_temporal<false>, grid, dim3(256), 0, stream, a);
}
int warm_temporal_kernels() {
    hipFuncAttributes a;
    hipError_t e;
    if ((e = hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_temporal<true>))) != hipSuccess) return (int)e;
    if ((e = hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_temporal<false>))) != hipSuccess) return (int)e;
    return 0;
}

}  // namespace crt
