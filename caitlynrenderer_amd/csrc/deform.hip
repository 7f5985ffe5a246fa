// crt_deformer's kernel for gfx950 (deform.hpp).  One thread per output element; the elements are cut into tiles of 256,
// the vertices' tiles first, then the normals', so a workgroup never holds both kinds.  Per element the streams cost 36 B read (12 B rest
// + 8 B indices + 16 B weights, one load each) and 12 B written; the bone palette is the part every thread shares, and it is read in
// one of two forms: through the vector cache (three 16-byte loads per influence), or from LDS where a workgroup stages it once and
// then walks several tiles.  No atomics: a vertex sums its own morph deltas in target order.
#include "deform.hpp"

#include <algorithm>

#include "host/deform_math.hpp"

namespace crt {

namespace {

constexpr uint32_t kTile = 256;
// the LDS form's grid: at most this many workgroups, each staging the palette once and striding over the tiles (256 CUs x 8)
constexpr uint32_t kLdsGrid = 2048;

struct F3 { float x, y, z; };        // one 12-byte load / store

__device__ __forceinline__ void load_bone(const float4* __restrict__ pal, uint32_t b, float B[12]) {
    const float4 r0 = pal[3u * b], r1 = pal[3u * b + 1u], r2 = pal[3u * b + 2u];
    B[0] = r0.x; B[1] = r0.y; B[2] = r0.z; B[3] = r0.w;
    B[4] = r1.x; B[5] = r1.y; B[6] = r1.z; B[7] = r1.w;
    B[8] = r2.x; B[9] = r2.y; B[10] = r2.z; B[11] = r2.w;
}

// Blend: M = w_0 * B[b_0], then + w_k * B[b_k] for the k = 1..3 whose weight is not zero (their bones are not loaded otherwise)
__device__ __forceinline__ void blend(const float4* __restrict__ pal, uint2 bi, float4 w, float M[12]) {
    const uint32_t b[4] = {bi.x & 0xffffu, bi.x >> 16, bi.y & 0xffffu, bi.y >> 16};
    const float wk[4] = {w.x, w.y, w.z, w.w};
    float B[12];
    load_bone(pal, b[0], B);
    dm::blend_first(M, wk[0], B);
#pragma unroll
    for (int k = 1; k < 4; ++k)
        if (wk[k] != 0.0f) {
            load_bone(pal, b[k], B);
            dm::blend_add(M, wk[k], B);
        }
}

__device__ __forceinline__ void deform_tile(const DeformArgs& a, const float4* __restrict__ pal, uint32_t tile, uint32_t tiles_v) {
    float M[12];
    if (tile < tiles_v) {
        const uint32_t i = tile * kTile + threadIdx.x;
        if (i >= a.n_vertices) return;
        const F3 r = reinterpret_cast<const F3*>(a.rest_v)[i];
        float p[3] = {r.x, r.y, r.z};
        if (a.morph_first) {
            const uint32_t end = a.morph_first[i + 1u];
            for (uint32_t e = a.morph_first[i]; e < end; ++e) {
                const float4 m = reinterpret_cast<const float4*>(a.morph)[e];
                const float d[3] = {m.x, m.y, m.z};
                dm::morph_add(p, a.morph_weights[__float_as_uint(m.w)], d);
            }
        }
        blend(pal, a.bones_v[i], a.weights_v[i], M);
        float o[3];
        dm::skin_position(M, p, o);
        reinterpret_cast<F3*>(a.out_v)[i] = F3{o[0], o[1], o[2]};
    } else {
        const uint32_t i = (tile - tiles_v) * kTile + threadIdx.x;
        if (i >= a.n_normals) return;
        const F3 r = reinterpret_cast<const F3*>(a.rest_n)[i];
        const float n[3] = {r.x, r.y, r.z};
        blend(pal, a.bones_n[i], a.weights_n[i], M);
        float o[3];
        dm::skin_normal(M, n, o);
        reinterpret_cast<F3*>(a.out_n)[i] = F3{o[0], o[1], o[2]};
    }
}

// the palette through the vector cache: one workgroup per tile
__global__ __launch_bounds__(256) void k_deform_global(const DeformArgs a, uint32_t tiles_v) {
    deform_tile(a, a.palette, blockIdx.x, tiles_v);
}

// the palette staged in LDS (48 * n_bones bytes of dynamic LDS), then the workgroup's tiles
__global__ __launch_bounds__(256) void k_deform_lds(const DeformArgs a, uint32_t tiles_v, uint32_t tiles) {
    extern __shared__ float4 s_palette[];
    for (uint32_t k = threadIdx.x; k < 3u * a.n_bones; k += kTile) s_palette[k] = a.palette[k];
    __syncthreads();
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) deform_tile(a, s_palette, tile, tiles_v);
}

}  // namespace

void launch_deform(const DeformArgs& a, int form, hipStream_t stream) {
    const uint32_t tiles_v = (a.n_vertices + kTile - 1u) / kTile, tiles = tiles_v + (a.n_normals + kTile - 1u) / kTile;
    if (!tiles) return;
    if (form == kDeformPaletteLds && a.n_bones <= kDeformLdsBones)
        hipLaunchKernelGGL(k_deform_lds, dim3(std::min(tiles, kLdsGrid)), dim3(kTile), 48u * a.n_bones, stream, a, tiles_v, tiles);
    else
        hipLaunchKernelGGL(k_deform_global, dim3(tiles), dim3(kTile), 0, stream, a, tiles_v);
}

}  // namespace crt
