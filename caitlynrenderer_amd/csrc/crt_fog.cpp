// Fog with light shafts (include/crt.h at crt_render_fog): the entries, their buffers and the chain of launches.  Both modes
// end in the same three steps over a buffer of fog segments — visibility words cleared, the any-hit walk that builds its rays where it
// loads them (k_fog_walk, k_fog_walk_instances), the fold (k_fog_fold) — and view mode puts two in front: the first hits of the view
// through the feature buffers' own kernels into a HIT buffer that belongs to the fog state (first_hits.hpp), and k_fog_view_segments.
// Nothing a frame, crt_render_aov or crt_render_ao reads or reports is written, beyond what crt_render_aov itself borrows of an instanced
// scene's frame.  The composite and the fogged image's accessors are with the other float images, in crt_outputs.cpp.
#include <cmath>
#include <exception>
#include <new>

#include "crt_scene.hpp"
#include "first_hits.hpp"
#include "fog.hpp"
#include "instances.hpp"

using crt::dev_alloc;
using crt::fail;
using crt::grow;

namespace {

struct FogCall { uint32_t K; float sigma, g, max_distance, albedo[3], ambient[3]; };

bool finite_in(float v, float lo, float hi) { return std::isfinite(v) && v >= lo && v <= hi; }

int check_params(const crt_fog_params* p, const char* who, FogCall* c) {
    const crt_fog_params def = {16u, 0u, 0.05f, {1.0f, 1.0f, 1.0f}, 0.0f, 100.0f, {0.0f, 0.0f, 0.0f}, {0u, 0u, 0u, 0u, 0u}};
    if (!p) p = &def;
    const std::string w(who);
    if (p->samples < 1u || p->samples > 256u) return fail(CRT_ERR_INVALID, w + ": samples must be in 1..256");
    if (p->flags != 0u) return fail(CRT_ERR_INVALID, w + ": flags must be 0");
    if (!finite_in(p->density, 0.0f, 1e6f)) return fail(CRT_ERR_INVALID, w + ": density must be finite and in [0, 1e6]");
    for (float a : p->albedo) if (!finite_in(a, 0.0f, 1.0f)) return fail(CRT_ERR_INVALID, w + ": albedo must be finite and in [0, 1]");
    if (!finite_in(p->anisotropy, -0.99f, 0.99f)) return fail(CRT_ERR_INVALID, w + ": anisotropy must be finite and in [-0.99, 0.99]");
    if (!(std::isfinite(p->max_distance) && p->max_distance > 0.0f)) return fail(CRT_ERR_INVALID, w + ": max_distance must be finite and > 0");
    for (float a : p->ambient) if (!(std::isfinite(a) && a >= 0.0f)) return fail(CRT_ERR_INVALID, w + ": ambient must be finite and >= 0");
    for (uint32_t r : p->reserved) if (r != 0u) return fail(CRT_ERR_INVALID, w + ": reserved must be 0");
    c->K = p->samples; c->sigma = p->density; c->g = p->anisotropy; c->max_distance = p->max_distance;
    for (int k = 0; k < 3; ++k) { c->albedo[k] = p->albedo[k]; c->ambient[k] = p->ambient[k]; }
    return CRT_OK;
}

// what every entry refuses of the scene, before anything is written
int check_scene(const crt_scene* s, const char* who) {
    const std::string w(who);
    if (s->accel != 0u) return fail(CRT_ERR_INVALID, w + ": the shadow rays take the CWBVH walk (option accel is 0)");
    if (s->primary || !s->peers.empty()) return fail(CRT_ERR_INVALID, w + ": a scene on one device and one stream only (crt_set_devices / option streams have dealt this one's tiles)");
    if (s->shard_world > 1u) return fail(CRT_ERR_INVALID, w + ": a whole frame only (crt_set_shard has world > 1)");
    return CRT_OK;
}

int ensure_state(crt_scene* s, const char* who) {
    if (s->fog) return CRT_OK;
    s->fog = new (std::nothrow) FogState;
    return s->fog ? CRT_OK : fail(CRT_ERR_NOMEM, std::string(who) + ": out of host memory");
}

// visibility words cleared, the walk, the fold: n segments at d_segments -> n results at d_out, on the scene's stream
int enqueue_segments(crt_scene* s, const float4* d_segments, uint32_t n, float rv, const FogCall& c, float4* d_out) {
    FogState* const fg = s->fog;
    int rc = crt::ensure_light_table(s);                                  // lights that follow the instances, as a frame has them
    if (rc) return rc;
    crt::FogGen g{};
    g.segments = d_segments; g.lights = s->d_lights; g.n_lights = (int32_t)s->n_lights;
    g.n = n; g.K = c.K; g.words = (c.K + 31u) / 32u;
    g.rv = rv; g.sigma = c.sigma; g.g = c.g;
    for (int k = 0; k < 3; ++k) { g.albedo[k] = c.albedo[k]; g.ambient[k] = c.ambient[k]; }
    if ((rc = grow(s, &fg->d_vis, &fg->vis_cap, (size_t)n * g.words))) return rc;
    HIPCHK(hipMemsetAsync(fg->d_vis, 0, (size_t)n * g.words * sizeof(uint32_t), s->stream));
    if (s->inst) {
        crt::InstancesView v{};
        crt::instances_view(s->inst, &v);
        const bool masked = s->instance_masks != 0u;
        if (masked && (rc = crt::instances_child_masks_for(s->inst, s->stream, &s->cmask_seen))) return rc;
        crt::InstMaskFogArgs a{};
        a.nodes = v.nodes; a.tris = v.tris; a.inst = v.inst;
        if (masked) { a.child_masks = v.child_masks; a.n_tlas8 = v.tlas_nodes8; a.ray_mask = s->mask_shadow; }
        a.g = g; a.vis = fg->d_vis;
        a.n_instances = v.n_instances; a.stack_entries = v.stack_entries;
        a.refill_min = 8; a.tri_min = 2;            // crt_instances_trace's
        a.overflow = s->d_overflow;
        crt::launch_fog_walk_instances(a, masked, s->stream);
    } else {
        crt::FogWalkArgs a{};
        a.nodes = s->d_nodes; a.tris = s->d_tris;
        a.g = g; a.vis = fg->d_vis;
        a.stack_entries = s->stack_entries;
        a.pool = s->shadow_pool; a.refill_min = s->shadow_refill_min; a.tri_min = s->tri_min ? s->tri_min : 1u;       // k_shadow_deferred's
        a.lanes_log2 = s->lanes_per_ray >= 8u ? 3u : 0u;
        a.overflow = s->d_overflow;
        crt::launch_fog_walk(a, s->stream);
    }
    crt::launch_fog_fold(g, fg->d_vis, d_out, s->stream);
    HIPCHK(hipGetLastError());
    return CRT_OK;
}

// what the two segments entries share in front of their own work; *go = false: refused, or n = 0
int begin_segments(crt_scene* s, const char* who, const void* segments, size_t n, const void* out, const crt_fog_params* params, FogCall* c, bool* go) {
    *go = false;
    const std::string w(who);
    if (!s) return fail(CRT_ERR_INVALID, w + ": null scene");
    if (n && (!segments || !out)) return fail(CRT_ERR_INVALID, w + ": null segments or out with n > 0");
    int rc = check_params(params, who, c);
    if (rc || (rc = check_scene(s, who))) return rc;
    if ((uint64_t)n * c->K >= (1ull << 32)) return fail(CRT_ERR_INVALID, w + ": n*samples must be below 2^32");
    if ((rc = crt::require_device())) return rc;
    HIPCHK(hipSetDevice(s->device));
    if (n == 0) return CRT_OK;
    if ((rc = ensure_state(s, who))) return rc;
    *go = true;
    return CRT_OK;
}

}  // namespace

extern "C" {

int crt_render_fog(crt_scene* s, float rx, float ry, const crt_fog_params* params, int sync) {
    if (!s) return fail(CRT_ERR_INVALID, "crt_render_fog: null scene");
    if (s->camera_rays()) return fail(CRT_ERR_INVALID, "crt_render_fog: the scene is seen along the caller's camera rays, which this call cannot follow (it looks through the pinhole): crt_clear_camera_rays first");
    FogCall c{};
    int rc = check_params(params, "crt_render_fog", &c);
    if (rc || (rc = check_scene(s, "crt_render_fog"))) return rc;
    if (!s->have_camera) return fail(CRT_ERR_INVALID, "crt_render_fog: crt_set_camera was never called");
    const size_t n_pixels = (size_t)s->width * s->height;
    if ((uint64_t)n_pixels * c.K >= (1ull << 32)) return fail(CRT_ERR_INVALID, "crt_render_fog: width*height*samples must be below 2^32");
    if ((rc = crt::require_device())) return rc;
    HIPCHK(hipSetDevice(s->device));
    if ((rc = ensure_state(s, "crt_render_fog"))) return rc;
    FogState* const fg = s->fog;
    if (!fg->d_hit && (rc = dev_alloc(&fg->d_hit, n_pixels))) return rc;
    if (!fg->d_view_segments && (rc = dev_alloc(&fg->d_view_segments, 2 * n_pixels))) return rc;
    if (!fg->d_image && (rc = dev_alloc(&fg->d_image, n_pixels))) return rc;
    crt::AovOut out{};
    out.hit = fg->d_hit;
    if ((rc = crt::enqueue_first_hits(s, out, CRT_AOV_HIT, &fg->first_hits, "crt_render_fog", rx, ry, (uint32_t)n_pixels))) return rc;
    crt::FogViewArgs va{};
    va.f = crt::frame_args(s, rx, ry);
    va.hit = fg->d_hit; va.segments = fg->d_view_segments; va.n_pixels = (uint32_t)n_pixels; va.max_distance = c.max_distance;
    crt::launch_fog_view_segments(va, s->stream);
    if ((rc = enqueue_segments(s, fg->d_view_segments, (uint32_t)n_pixels, va.f.rv, c, fg->d_image))) return rc;
    fg->rendered = true;
    if (sync) HIPCHK(hipStreamSynchronize(s->stream));
    return CRT_OK;
}

int crt_fog_segments_device(crt_scene* s, const void* d_segments, size_t n, float rx, float ry, const crt_fog_params* params, void* d_out, int sync) {
    FogCall c{};
    bool go;
    int rc = begin_segments(s, "crt_fog_segments_device", d_segments, n, d_out, params, &c, &go);
    if (rc || !go) return rc;
    if ((rc = enqueue_segments(s, static_cast<const float4*>(d_segments), (uint32_t)n, rx * ry, c, static_cast<float4*>(d_out)))) return rc;
    if (sync) HIPCHK(hipStreamSynchronize(s->stream));
    return CRT_OK;
}

int crt_fog_segments(crt_scene* s, const crt_fog_segment* segments, size_t n, float rx, float ry, const crt_fog_params* params, float* out) {
    FogCall c{};
    bool go;
    int rc = begin_segments(s, "crt_fog_segments", segments, n, out, params, &c, &go);
    if (rc || !go) return rc;
    FogState* const fg = s->fog;
    static_assert(sizeof(crt_fog_segment) == 32 && sizeof(crt_fog_params) == 64, "fog layouts");
    if ((rc = grow(s, &fg->d_segments, &fg->segments_cap, 2 * n))) return rc;
    if ((rc = grow(s, &fg->d_out, &fg->out_cap, n))) return rc;
    HIPCHK(hipMemcpyAsync(fg->d_segments, segments, n * sizeof(crt_fog_segment), hipMemcpyHostToDevice, s->stream));
    if ((rc = enqueue_segments(s, fg->d_segments, (uint32_t)n, rx * ry, c, fg->d_out))) return rc;
    HIPCHK(hipMemcpyAsync(out, fg->d_out, n * 4 * sizeof(float), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return CRT_OK;
}

int crt_read_fog(crt_scene* s, float* dst, size_t n_floats) {
    if (!s || !dst) return fail(CRT_ERR_INVALID, "crt_read_fog: null argument");
    if (!s->fog || !s->fog->rendered) return fail(CRT_ERR_INVALID, "crt_read_fog: no crt_render_fog call has succeeded on this scene");
    if (n_floats != (size_t)s->width * s->height * 4u) return fail(CRT_ERR_INVALID, "crt_read_fog: n_floats must be width*height*4");
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipMemcpyAsync(dst, s->fog->d_image, n_floats * sizeof(float), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return CRT_OK;
}

int crt_fog_device(crt_scene* s, const float** d_ptr) {
    if (!s || !d_ptr) return fail(CRT_ERR_INVALID, "crt_fog_device: null argument");
    *d_ptr = nullptr;
    if (!s->fog || !s->fog->rendered) return fail(CRT_ERR_INVALID, "crt_fog_device: no crt_render_fog call has succeeded on this scene");
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipStreamSynchronize(s->stream));
    *d_ptr = reinterpret_cast<const float*>(s->fog->d_image);
    return CRT_OK;
}

}  // extern "C"
