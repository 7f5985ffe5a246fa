// Device helpers of the CWBVH walks shared by the traversal kernels of rt_kernels.hip and the two-level walk of instances.hip:
// the 8-wide child-box test, the triangle test, the row addressing and the XCD-aware work distribution.  Moved here verbatim from
// rt_kernels.hip; every kernel that includes them inlines them, so the walks of both translation units share one arithmetic.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_kernels.hpp"
#include "rt_math.hpp"

namespace crt {

__device__ __forceinline__ uint32_t sign_extend_s8x4(uint32_t x) { return ((x >> 7) & 0x01010101u) * 0xffu; }   // cwbvh.fs:369-372


__device__ __forceinline__ float ubyte_f(uint32_t x, int j) { return (float)((x >> (8 * j)) & 0xffu); }          // v_cvt_f32_ubyteN

// 8-wide quantised child-box test (cwbvh.fs:376-446, corrected: far = min(min()), tmin clamped to 0,
// tmax clamped to max_t, hit iff tmin <= tmax).  ~19 VALU instructions per child (6 cvt_f32_ubyte, 6 fma, max3,
// min3, 2 clamps, compare, shift, select); pairing the near/far fmas of an axis into v_pk_fma_f32 (24 instead of
// 48) was measured twice: 0.224 vs 0.217 ms (200-frame averages) and 9 more VGPRs, so the scalar form stays.  Returns the hit mask: inner children in the top
// byte at bit (24+slot)^oct, leaf triangles as unary-count bits in the low 24.
// Round 3 measured what each instruction kind costs (profiles/r03_valu_issue_cycles.txt: only fma / mul / add / mov issue at ~2.5
// cycles per wave64 instruction, conversions, min / max, compares and integer ops at ~4.2) and tried the obvious answer — a 128-byte
// device copy of the node with the planes widened to IEEE halves, so that the conversion rides inside v_fma_mix_f32 and the ray picks
// near / far plane rows by address instead of 12 v_cndmask (55 fewer instructions per node, same arithmetic, bit-identical).  It
// lost: v_fma_mix_f32 is a 4.3-cycle instruction itself, and 8 row loads per node instead of 5 saturate the CU's vector-memory path
// (1,004,672 triangles 12,574 vs 12,365 Mray/s at 96 VGPRs but the 80-VGPR build spills in the loop, 4 segments 4,995 vs 5,047,
// the 8 M-triangle scene 6,942 vs 8,588).  The patch is kept as profiles/r03_f16_planes_experiment.patch.
// Also tried: the mask assembly (54 of the 230 instructions, all of the 4.2-cycle kind) with the byte extractions folded into SDWA
// operand selects by inline assembly (v_lshlrev_b32_sdwa: child_bits << bit_index in one instruction per child, the exponent bytes
// likewise): 223 instructions per visit instead of 230 and SLOWER — 13,120 vs 13,660 Mray/s, 4 segments 5,357 vs 5,402, Cornell
// 45,250 vs 44,640: an SDWA instruction costs more issue time than the two plain ones it replaces.
// keep: bit i clear = meta slot i is culled whatever its box (the masked instanced walk's TLAS steps); every other caller
// leaves the default 0xff, which folds away and leaves their code as it was.
__device__ __forceinline__ uint32_t node8_intersect(const uint4 n0, const uint4 n1, const uint4 n2, const uint4 n3,
                                                    const uint4 n4, vec3 o, vec3 inv, bool negx, bool negy, bool negz,
                                                    uint32_t oct4, float max_t, uint32_t keep = 0xffu) {
    const vec3 p = V3(__uint_as_float(n0.x), __uint_as_float(n0.y), __uint_as_float(n0.z));
    const uint32_t e_imask = n0.w;
    const vec3 adj_inv = V3(__uint_as_float((e_imask & 0xffu) << 23) * inv.x,
                            __uint_as_float(((e_imask >> 8) & 0xffu) << 23) * inv.y,
                            __uint_as_float(((e_imask >> 16) & 0xffu) << 23) * inv.z);
    const vec3 adj_o = (p - o) * inv;
    uint32_t hit_mask = 0;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const uint32_t meta4 = i == 0 ? n1.z : n1.w;
        const uint32_t is_inner4 = (meta4 & (meta4 << 1)) & 0x10101010u;
        const uint32_t inner_mask4 = sign_extend_s8x4(is_inner4 << 3);
        const uint32_t bit_index4 = (meta4 ^ (oct4 & inner_mask4)) & 0x1F1F1F1Fu;
        const uint32_t child_bits4 = (meta4 >> 5) & 0x07070707u;
        const uint32_t qlox = i == 0 ? n2.x : n2.y, qhix = i == 0 ? n2.z : n2.w;
        const uint32_t qloy = i == 0 ? n3.x : n3.y, qhiy = i == 0 ? n3.z : n3.w;
        const uint32_t qloz = i == 0 ? n4.x : n4.y, qhiz = i == 0 ? n4.z : n4.w;
        const uint32_t xmin = negx ? qhix : qlox, xmax = negx ? qlox : qhix;
        const uint32_t ymin = negy ? qhiy : qloy, ymax = negy ? qloy : qhiy;
        const uint32_t zmin = negz ? qhiz : qloz, zmax = negz ? qloz : qhiz;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float tminx = __builtin_fmaf(ubyte_f(xmin, j), adj_inv.x, adj_o.x);
            const float tminy = __builtin_fmaf(ubyte_f(ymin, j), adj_inv.y, adj_o.y);
            const float tminz = __builtin_fmaf(ubyte_f(zmin, j), adj_inv.z, adj_o.z);
            const float tmaxx = __builtin_fmaf(ubyte_f(xmax, j), adj_inv.x, adj_o.x);
            const float tmaxy = __builtin_fmaf(ubyte_f(ymax, j), adj_inv.y, adj_o.y);
            const float tmaxz = __builtin_fmaf(ubyte_f(zmax, j), adj_inv.z, adj_o.z);
            const float tmin = __builtin_fmaxf(__builtin_fmaxf(tminx, tminy), __builtin_fmaxf(tminz, 0.0f));
            const float tmax = __builtin_fminf(__builtin_fminf(tmaxx, tmaxy), __builtin_fminf(tmaxz, max_t));
            if (tmin <= tmax && ((keep >> (4 * i + j)) & 1u)) {
                const uint32_t child_bits = (child_bits4 >> (8 * j)) & 0xffu;
                const uint32_t bit_index = (bit_index4 >> (8 * j)) & 0xffu;
                hit_mask |= child_bits << bit_index;
            }
        }
    }
    return hit_mask;
}

__device__ __forceinline__ float clamp_dir(float d) {
    const float eps = 0x1p-80f;
    return __builtin_fabsf(d) > eps ? d : __builtin_copysignf(eps, d);
}

// Moller-Trumbore, operation order of path_trace.fs:337-360, on the pre-gathered record
// (v0, e1 = v1 - v0, e2 = v2 - v0): the two subtractions are the same fp32 operations the shader
// performs per test, done once at upload.
__device__ __forceinline__ bool mt_test(const float4 a, const float4 b, const float4 c, vec3 o, vec3 d, float& u,
                                        float& v, float& t) {
    const vec3 v0 = V3(a.x, a.y, a.z), e1 = V3(b.x, b.y, b.z), e2 = V3(c.x, c.y, c.z);
    const vec3 pv = cross(d, e2);
    const vec3 tv = o - v0;
    const vec3 qv = cross(tv, e1);
    float uu = dot(tv, pv);
    float vv = dot(d, qv);
    float tt = dot(e2, qv);
    const float inv_det = rcp_ieee(dot(e1, pv));
    uu = uu * inv_det;
    vv = vv * inv_det;
    tt = tt * inv_det;
    const float w = 1.0f - uu - vv;
    u = uu; v = vv; t = tt;
    return (uu >= 0.0f) & (vv >= 0.0f) & (tt >= 0.0f) & (w >= 0.0f);
}

// Row address of a node / triangle record as uniform base + a 32-bit byte offset: the load then takes the base from an SGPR pair and the
// offset from one VGPR (global_load ... v_off, s[base]) instead of a 64-bit v_mad_u64_u32 per visit — an instruction that costs 8.9
// issue cycles against 4.4 for the 32-bit multiply (profiles/r03_valu_issue_cycles.txt).  crt_scene_create refuses arrays beyond 4 GiB.
__device__ __forceinline__ const uint4* node_rows(const uint4* nodes, uint32_t idx) {
    return reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(nodes) + (size_t)(idx * (uint32_t)(CRT_NODE_ROWS * 16)));
}
__device__ __forceinline__ const float4* tri_rows(const float4* tris, uint32_t idx) {
    return reinterpret_cast<const float4*>(reinterpret_cast<const char*>(tris) + (size_t)(idx * (uint32_t)(CRT_TRI_ROWS * 16)));
}

#define CRT_COUNTER_STRIDE 32u   // uint32 slots between two per-group counters (128 B)

// ------------------------------------------------------------------ scheduling -------

// XCD-aware work distribution shared by all traversal kernels.  By default the host launches one (single-wave)
// workgroup per batch, so `it` below only ever takes the value 0 and the hardware dispatcher balances the load; with a
// smaller, persistent grid (option "oversubscribe" >= 1) the same mapping is a static round-robin schedule.
//
// Work is cut into 64-ray batches (one wave; one 8x8 pixel block for primary rays) and chunks of 4
// batches (one workgroup pass, a 16x16 pixel patch).  Every chunk belongs to one of 8 *groups*:
//   - dense index spaces (pixels, explicit ray buffers): 64 consecutive batches form a unit (one 64x64
//     tile) and unit u belongs to group u & 7;
//   - device-written queues (path rays, shadow rays) are 8 sub-queues, one per group: a group appends to
//     and later consumes its own sub-queue, so a ray stays with the group (and normally the L2) that
//     already holds its neighbourhood, and the append atomics are spread over 8 counters on separate
//     cache lines (a single counter saturates near 90 returning atomics per microsecond: at one atomic
//     per 64-ray wave that capped a whole 1080p frame at ~0.18 ms; measured 0.183 -> 0.074 ms).
// Workgroups are dealt round-robin to the 8 XCDs by the dispatcher, so blockIdx & 7 labels workgroups
// that share an L2 (a speed heuristic only; correctness never depends on placement).  Workgroup j of a
// group takes that group's chunks j, j + groups_size, ...  A dynamic variant (one returning atomic per
// chunk on a per-group counter, stealing from other groups when drained) was measured and dropped: equal
// on the 1 M-triangle scenes (0.404 vs 0.396 ms) and 1.8x slower on Cornell (0.132 vs 0.074 ms), where the
// per-chunk atomic + two barriers sit on the critical path of very short rays.
// The pass loop of a workgroup over its chunks.  The default build launches one workgroup per chunk (the hardware dispatcher is the
// scheduler), so the loop body runs once — and is written as a loop the compiler can see runs once: around a real loop it hoists
// every wave-uniform value and constant of the body into SGPRs that then live (or spill into VGPR lanes) across the whole kernel.
#ifdef CRT_EXPERIMENTS
#define CRT_CHUNK_LOOP(it) for (uint32_t it = 0;; ++it)          // persistent grids (option "oversubscribe")
#else
#define CRT_CHUNK_LOOP(it) for (uint32_t it = 0; it < 1u; ++it)
#endif
#define CRT_NO_WORK 0xffffffffu

__device__ __forceinline__ uint32_t dense_chunks_of_group(uint32_t n_items, uint32_t g) {
    const uint32_t n_units = (((n_items + 63u) >> 6) + 63u) >> 6;
    return n_units > g ? ((n_units - g + 7u) >> 3) * 16u : 0u;
}
__device__ __forceinline__ uint32_t queue_chunks(uint32_t n) { return (((n + 63u) >> 6) + 3u) >> 2; }

// (group << 28 | chunk) for iteration `it` of this workgroup, or CRT_NO_WORK; uniform over the workgroup.
// A workgroup is 4 waves (256 threads), 2 waves or a single wave: with fewer than 4 waves per workgroup, 4 / W
// consecutive workgroups of the same XCD stand for one chunk, so the dispatcher refills CUs (half-)wave-pair by wave.
struct WaveId { uint32_t lane, wave, lds_wave, vblock, vgrid, quadrant, sub; };
// four_per_batch (lane_samples): four consecutive single-wave workgroups of an XCD slice stand for ONE batch, one 4 x 4 pixel quadrant each
// sub_log2 (k_trace, single-wave workgroups): 1 << sub_log2 consecutive workgroups of an XCD slice stand for ONE wave of the mapping
// below, `sub` says which of them this is
__device__ __forceinline__ WaveId wave_id(bool one_batch_per_workgroup = false, bool four_per_batch = false, uint32_t sub_log2 = 0u) {
    WaveId w;
    w.lane = threadIdx.x & 63u;
    w.lds_wave = threadIdx.x >> 6;
    w.sub = 0u;
    if (four_per_batch) {
        const uint32_t qq = blockIdx.x >> 3;
        w.quadrant = qq & 3u;
        const uint32_t q = qq >> 2;
        w.wave = q & 3u;
        w.vblock = ((q >> 2) << 3) | (blockIdx.x & 7u);
        w.vgrid = gridDim.x >> 4;
        return w;
    }
    w.quadrant = 0u;
    // W = 1, 2 or 4 waves per workgroup: 4 / W consecutive workgroups of the same XCD slice stand for one 4-batch chunk.
    // one_batch_per_workgroup (wave_samples): the workgroup's waves all work on ONE batch, so it maps like a single wave.
    const uint32_t W = one_batch_per_workgroup ? 1u : blockDim.x >> 6, per_log2 = W == 1u ? 2u : W == 2u ? 1u : 0u;
    w.sub = (blockIdx.x >> 3) & ((1u << sub_log2) - 1u);
    const uint32_t q = blockIdx.x >> (3u + sub_log2);
    w.wave = (q & ((1u << per_log2) - 1u)) * W + (one_batch_per_workgroup ? 0u : w.lds_wave);
    w.vblock = ((q >> per_log2) << 3) | (blockIdx.x & 7u);
    w.vgrid = gridDim.x >> (per_log2 + sub_log2);
    return w;
}

template <bool DENSE>
__device__ __forceinline__ uint32_t static_chunk(const WaveId& w, const uint32_t* counts, uint32_t n_dense, uint32_t it) {
    const uint32_t g = w.vblock & 7u;
    const uint32_t nch = DENSE ? dense_chunks_of_group(n_dense, g) : queue_chunks(counts[g * CRT_COUNTER_STRIDE]);
    const uint32_t c = (w.vblock >> 3) + it * (w.vgrid >> 3);     // the host launches a multiple of 8 workgroups
    return c < nch ? (g << 28) | c : CRT_NO_WORK;
}

// Pool-based kernels: a workgroup chunk is 1024 items, 256 consecutive items per wave (its refill pool).
__device__ __forceinline__ uint32_t dense_pool_chunks_of_group(uint32_t n_items, uint32_t g) {
    const uint32_t n_units = (n_items + 4095u) >> 12;
    return n_units > g ? ((n_units - g + 7u) >> 3) * 4u : 0u;
}
__device__ __forceinline__ uint32_t queue_pool_chunks(uint32_t n) { return (n + 1023u) >> 10; }
template <bool DENSE>
__device__ __forceinline__ uint32_t static_pool_chunk(const WaveId& w, const uint32_t* counts, uint32_t n_dense, uint32_t it) {
    const uint32_t g = w.vblock & 7u;
    const uint32_t nch = DENSE ? dense_pool_chunks_of_group(n_dense, g) : queue_pool_chunks(counts[g * CRT_COUNTER_STRIDE]);
    const uint32_t c = (w.vblock >> 3) + it * (w.vgrid >> 3);
    return c < nch ? (g << 28) | c : CRT_NO_WORK;
}
// first item of this wave's pool for a dense pool chunk
__device__ __forceinline__ uint32_t dense_pool_first(uint32_t v, uint32_t wave) {
    const uint32_t g = v >> 28, c = v & 0x0fffffffu;
    const uint32_t unit = (c >> 2) * 8u + g;
    return unit * 4096u + (c & 3u) * 1024u + wave * 256u;
}

// index of this lane's item for a dense chunk (>= n_items when past the end)
__device__ __forceinline__ uint32_t dense_item(uint32_t v, uint32_t wave, uint32_t lane) {
    const uint32_t g = v >> 28, c = v & 0x0fffffffu;
    const uint32_t unit = (c >> 4) * 8u + g;
    return (unit * 64u + (c & 15u) * 4u + wave) * 64u + lane;
}

}  // namespace crt
