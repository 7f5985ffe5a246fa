// Ambient occlusion (include/crt.h at crt_render_ao): the entries, their buffers and the chain of launches.  Both modes end in
// the same three steps over a buffer of AO points — visibility words cleared, the any-hit walk that builds its rays where it loads them
// (k_ao_walk, k_ao_walk_instances), the fold (k_ao_fold) — and view mode puts two in front: the first hits of the view through the feature
// buffers' own kernels into HIT and NORMAL buffers that belong to the AO state (first_hits.hpp), and k_ao_view_points.  Nothing a frame or crt_render_aov
// reads or reports is written, beyond what crt_render_aov itself borrows of an instanced scene's frame (segment 0's queue, its hits, the path state).
#include <cmath>
#include <exception>
#include <new>

#include "ao.hpp"
#include "crt_scene.hpp"
#include "first_hits.hpp"
#include "instances.hpp"

using crt::dev_alloc;
using crt::fail;
using crt::grow;

namespace {

struct AoCall { uint32_t K; float radius, offset; };

int check_params(const crt_ao_params* p, const char* who, AoCall* c) {
    const crt_ao_params def = {16u, 0u, 1e9f, 0.0002f, {0u, 0u, 0u, 0u}};
    if (!p) p = &def;
    const std::string w(who);
    if (p->samples < 1u || p->samples > 256u) return fail(CRT_ERR_INVALID, w + ": samples must be in 1..256");
    if (!(std::isfinite(p->radius) && p->radius > 0.0f)) return fail(CRT_ERR_INVALID, w + ": radius must be finite and > 0 (1e9f = unbounded)");
    if (!(std::isfinite(p->offset) && p->offset >= 0.0f)) return fail(CRT_ERR_INVALID, w + ": offset must be finite and >= 0");
    if (p->flags != 0u) return fail(CRT_ERR_INVALID, w + ": flags must be 0");
    for (uint32_t r : p->reserved) if (r != 0u) return fail(CRT_ERR_INVALID, w + ": reserved must be 0");
    c->K = p->samples; c->radius = p->radius; c->offset = p->offset;
    return CRT_OK;
}

// what every entry refuses of the scene, before anything is written
int check_scene(const crt_scene* s, const char* who) {
    const std::string w(who);
    if (s->accel != 0u) return fail(CRT_ERR_INVALID, w + ": the occlusion rays take the CWBVH walk (option accel is 0)");
    if (s->primary || !s->peers.empty()) return fail(CRT_ERR_INVALID, w + ": a scene on one device and one stream only (crt_set_devices / option streams have dealt this one's tiles)");
    if (s->shard_world > 1u) return fail(CRT_ERR_INVALID, w + ": a whole frame only (crt_set_shard has world > 1)");
    return CRT_OK;
}

int ensure_state(crt_scene* s, const char* who) {
    if (s->ao) return CRT_OK;
    s->ao = new (std::nothrow) AoState;
    return s->ao ? CRT_OK : fail(CRT_ERR_NOMEM, std::string(who) + ": out of host memory");
}

// visibility words cleared, the walk, the fold: n points at d_points -> n results at d_out, on the scene's stream
int enqueue_points(crt_scene* s, const float4* d_points, uint32_t n, float rv, const AoCall& c, float4* d_out) {
    AoState* const ao = s->ao;
    crt::AoGen g{};
    g.points = d_points; g.n = n; g.K = c.K; g.words = (c.K + 31u) / 32u;
    g.rv = rv; g.radius = c.radius; g.offset = c.offset;
    int rc = grow(s, &ao->d_vis, &ao->vis_cap, (size_t)n * g.words);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(ao->d_vis, 0, (size_t)n * g.words * sizeof(uint32_t), s->stream));
    if (s->inst) {
        crt::InstancesView v{};
        crt::instances_view(s->inst, &v);
        const bool masked = s->instance_masks != 0u;
        if (masked && (rc = crt::instances_child_masks_for(s->inst, s->stream, &s->cmask_seen))) return rc;
        crt::InstMaskAoArgs a{};
        a.nodes = v.nodes; a.tris = v.tris; a.inst = v.inst;
        if (masked) { a.child_masks = v.child_masks; a.n_tlas8 = v.tlas_nodes8; a.ray_mask = s->mask_shadow; }
        a.g = g; a.vis = ao->d_vis;
        a.n_instances = v.n_instances; a.stack_entries = v.stack_entries;
        a.refill_min = 8; a.tri_min = 2;            // crt_instances_trace's
        a.overflow = s->d_overflow;
        crt::launch_ao_walk_instances(a, masked, s->stream);
    } else {
        crt::AoWalkArgs a{};
        a.nodes = s->d_nodes; a.tris = s->d_tris;
        a.g = g; a.vis = ao->d_vis;
        a.stack_entries = s->stack_entries;
        a.pool = s->shadow_pool; a.refill_min = s->shadow_refill_min; a.tri_min = s->tri_min ? s->tri_min : 1u;       // k_shadow_deferred's
        a.lanes_log2 = s->lanes_per_ray >= 8u ? 3u : 0u;
        a.overflow = s->d_overflow;
        crt::launch_ao_walk(a, s->stream);
    }
    crt::launch_ao_fold(g, ao->d_vis, d_out, s->stream);
    HIPCHK(hipGetLastError());
    return CRT_OK;
}

}  // namespace

extern "C" {

int crt_render_ao(crt_scene* s, float rx, float ry, const crt_ao_params* params, int sync) {
    if (!s) return fail(CRT_ERR_INVALID, "crt_render_ao: null scene");
    if (s->camera_rays()) return fail(CRT_ERR_INVALID, "crt_render_ao: the scene is seen along the caller's camera rays, which this call cannot follow (it looks through the pinhole): crt_clear_camera_rays first");
    AoCall c{};
    int rc = check_params(params, "crt_render_ao", &c);
    if (rc || (rc = check_scene(s, "crt_render_ao"))) return rc;
    if (!s->have_camera) return fail(CRT_ERR_INVALID, "crt_render_ao: crt_set_camera was never called");
    const size_t n_pixels = (size_t)s->width * s->height;
    if ((uint64_t)n_pixels * c.K >= (1ull << 32)) return fail(CRT_ERR_INVALID, "crt_render_ao: width*height*samples must be below 2^32");
    if ((rc = crt::require_device())) return rc;
    HIPCHK(hipSetDevice(s->device));
    if ((rc = ensure_state(s, "crt_render_ao"))) return rc;
    AoState* const ao = s->ao;
    if (!ao->d_hit && (rc = dev_alloc(&ao->d_hit, n_pixels))) return rc;
    if (!ao->d_normal && (rc = dev_alloc(&ao->d_normal, n_pixels))) return rc;
    if (!ao->d_view_points && (rc = dev_alloc(&ao->d_view_points, 2 * n_pixels))) return rc;
    if (!ao->d_image && (rc = dev_alloc(&ao->d_image, n_pixels))) return rc;
    crt::AovOut out{};
    out.hit = ao->d_hit; out.normal = ao->d_normal;
    if ((rc = crt::enqueue_first_hits(s, out, CRT_AOV_HIT | CRT_AOV_NORMAL, &ao->first_hits, "crt_render_ao", rx, ry, (uint32_t)n_pixels))) return rc;
    crt::AoViewArgs va{};
    va.f = crt::frame_args(s, rx, ry);
    va.hit = ao->d_hit; va.normal = ao->d_normal; va.points = ao->d_view_points; va.n_pixels = (uint32_t)n_pixels;
    crt::launch_ao_view_points(va, s->stream);
    if ((rc = enqueue_points(s, ao->d_view_points, (uint32_t)n_pixels, va.f.rv, c, ao->d_image))) return rc;
    ao->rendered = true;
    if (sync) HIPCHK(hipStreamSynchronize(s->stream));
    return CRT_OK;
}

int crt_ao_points_device(crt_scene* s, const void* d_points, size_t n, float rx, float ry, const crt_ao_params* params, void* d_out, int sync) {
    if (!s) return fail(CRT_ERR_INVALID, "crt_ao_points_device: null scene");
    if (n && (!d_points || !d_out)) return fail(CRT_ERR_INVALID, "crt_ao_points_device: null points or out with n > 0");
    AoCall c{};
    int rc = check_params(params, "crt_ao_points_device", &c);
    if (rc || (rc = check_scene(s, "crt_ao_points_device"))) return rc;
    if ((uint64_t)n * c.K >= (1ull << 32)) return fail(CRT_ERR_INVALID, "crt_ao_points_device: n*samples must be below 2^32");
    if ((rc = crt::require_device())) return rc;
    HIPCHK(hipSetDevice(s->device));
    if (n == 0) return CRT_OK;
    if ((rc = ensure_state(s, "crt_ao_points_device"))) return rc;
    if ((rc = enqueue_points(s, static_cast<const float4*>(d_points), (uint32_t)n, rx * ry, c, static_cast<float4*>(d_out)))) return rc;
    if (sync) HIPCHK(hipStreamSynchronize(s->stream));
    return CRT_OK;
}

int crt_ao_points(crt_scene* s, const crt_ao_point* points, size_t n, float rx, float ry, const crt_ao_params* params, float* out) {
    if (!s) return fail(CRT_ERR_INVALID, "crt_ao_points: null scene");
    if (n && (!points || !out)) return fail(CRT_ERR_INVALID, "crt_ao_points: null points or out with n > 0");
    AoCall c{};
    int rc = check_params(params, "crt_ao_points", &c);
    if (rc || (rc = check_scene(s, "crt_ao_points"))) return rc;
    if ((uint64_t)n * c.K >= (1ull << 32)) return fail(CRT_ERR_INVALID, "crt_ao_points: n*samples must be below 2^32");
    if ((rc = crt::require_device())) return rc;
    HIPCHK(hipSetDevice(s->device));
    if (n == 0) return CRT_OK;
    if ((rc = ensure_state(s, "crt_ao_points"))) return rc;
    AoState* const ao = s->ao;
    static_assert(sizeof(crt_ao_point) == 32 && sizeof(crt_ao_params) == 32, "AO layouts");
    if ((rc = grow(s, &ao->d_points, &ao->points_cap, 2 * n))) return rc;
    if ((rc = grow(s, &ao->d_out, &ao->out_cap, n))) return rc;
    HIPCHK(hipMemcpyAsync(ao->d_points, points, n * sizeof(crt_ao_point), hipMemcpyHostToDevice, s->stream));
    if ((rc = enqueue_points(s, ao->d_points, (uint32_t)n, rx * ry, c, ao->d_out))) return rc;
    HIPCHK(hipMemcpyAsync(out, ao->d_out, n * 4 * sizeof(float), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return CRT_OK;
}

int crt_read_ao(crt_scene* s, float* dst, size_t n_floats) {
    if (!s || !dst) return fail(CRT_ERR_INVALID, "crt_read_ao: null argument");
    if (!s->ao || !s->ao->rendered) return fail(CRT_ERR_INVALID, "crt_read_ao: no crt_render_ao call has succeeded on this scene");
    if (n_floats != (size_t)s->width * s->height * 4u) return fail(CRT_ERR_INVALID, "crt_read_ao: n_floats must be width*height*4");
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipMemcpyAsync(dst, s->ao->d_image, n_floats * sizeof(float), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return CRT_OK;
}

int crt_ao_device(crt_scene* s, const float** d_ptr) {
    if (!s || !d_ptr) return fail(CRT_ERR_INVALID, "crt_ao_device: null argument");
    *d_ptr = nullptr;
    if (!s->ao || !s->ao->rendered) return fail(CRT_ERR_INVALID, "crt_ao_device: no crt_render_ao call has succeeded on this scene");
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipStreamSynchronize(s->stream));
    *d_ptr = reinterpret_cast<const float*>(s->ao->d_image);
    return CRT_OK;
}

}  // extern "C"
