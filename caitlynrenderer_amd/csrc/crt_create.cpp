// Where a scene is made (DESIGN.md "Where a scene is made"): crt_scene_create for a host-built and for a device-built tree,
// crt_scene_create_instanced / _lit, crt_scene_destroy, and what a replica and a rebuild share with them (finish_scene_setup, adopt_tree).
// The three creators differ in where their tree comes from; what they check of a descriptor, how an array reaches the device and how its
// size reaches the replica table (crt_scene.hpp SharedBuf) is here once.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/crt.h"
#include "crt_error.hpp"
#include "crt_scene.hpp"
#include "device_build.hpp"
#include "host/cwbvh.hpp"
#include "host/flatnode_link.hpp"
#include "instances.hpp"
#include "instances_bind.hpp"
#include "rt_kernels.hpp"

using crt::dev_alloc;
using crt::fail;
using crt::require_device;

namespace {

constexpr int kMaxEvents = 8 + 8 * 16;

static_assert(sizeof(crt_node8) == 80, "node8 must be 80 bytes (cwbvh.h:11-25)");
static_assert(sizeof(crt_triangle) == 48 && sizeof(crt_flatnode) == 32 && sizeof(crt_material) == 64 && sizeof(crt_light) == 72, "layout");

// *dst = a device array of `count` elements filled from the host array `src`: behind what `st` holds (the source must outlive that), or,
// with a null stream, copied when this returns
template <typename T>
int upload(T** dst, const void* src, size_t count, hipStream_t st = nullptr) {
    const int rc = dev_alloc(dst, count);
    if (rc) return rc;
    if (!count) return CRT_OK;
    const hipError_t e = st ? hipMemcpyAsync(*dst, src, count * sizeof(T), hipMemcpyHostToDevice, st) : hipMemcpy(*dst, src, count * sizeof(T), hipMemcpyHostToDevice);
    return e == hipSuccess ? CRT_OK : fail(CRT_ERR_HIP, "hipMemcpy H2D failed");
}

// the same into a buffer replicas share or copy: the size the table holds is the size allocated here
template <typename T>
int upload_shared(crt_scene* s, SharedBuf k, const void* src, size_t count, hipStream_t st = nullptr) {
    s->shared_bytes[k] = count * sizeof(T);
    return upload(reinterpret_cast<T**>(s->shared_slot(k)), src, count, st);
}

// What both descriptors ask of a frame, of the textures and of the materials.  `who` is the entry's prefix; texcoords_missing: the entry
// refuses a textured material when the descriptor has no texcoords; light_bound: the lights an emissive material may name.
template <typename Desc>
int check_descriptor(const std::string& who, const Desc& d, bool texcoords_missing, size_t light_bound) {
    if (d.width == 0 || d.height == 0 || d.width > 65535u * 8u || d.height > 65535u * 8u) return fail(CRT_ERR_INVALID, who + "bad resolution");
    if (d.max_depth == 0 || d.max_depth > 16) return fail(CRT_ERR_INVALID, who + "max_depth must be 1..16");
    const bool have_tex = d.albedo_textures && d.n_textures > 0;
    if (have_tex && (d.tex_width == 0 || d.tex_height == 0 || d.tex_width > 16384 || d.tex_height > 16384)) return fail(CRT_ERR_INVALID, who + "bad texture size");
    for (size_t m = 0; m < d.n_materials; ++m) {
        const float tx = d.materials[m].tex_ind[0];
        if (have_tex && tx != -1.0f) {
            if (!(tx >= 0.0f && tx < (float)d.n_textures)) return fail(CRT_ERR_INVALID, who + "material texture index out of range");
            if (texcoords_missing) return fail(CRT_ERR_INVALID, who + "textured material but no texcoords");
        }
    }
    for (size_t m = 0; m < d.n_materials; ++m) {
        const float ew = d.materials[m].emission[3];
        if (ew != -1.0f && !(ew >= 0.0f && (size_t)ew < light_bound)) return fail(CRT_ERR_INVALID, who + "emissive material refers to a light that does not exist");
    }
    return CRT_OK;
}

// The shading arrays a creator has in hand: normals, materials, lights and, with textures, texcoords and the albedo array as RGB32F.
// The arrays go up behind `st` (null: synchronously); the textures always synchronously, from the converted copy made here.
template <typename Desc>
int upload_shading(crt_scene* s, const Desc& d, const float* normals, size_t n_normals, const float* texcoords, size_t n_texcoords, hipStream_t st) {
    int rc;
    if ((rc = upload_shared<float>(s, kSharedNormals, normals, n_normals * 3, st)) || (rc = upload_shared<float4>(s, kSharedMaterials, d.materials, d.n_materials * 4, st)) ||
        (rc = upload_shared<float>(s, kSharedLights, d.lights, d.n_lights * 18, st)))
        return rc;
    if (d.albedo_textures && d.n_textures > 0) {
        const size_t n_tex = (size_t)d.tex_width * d.tex_height * d.n_textures * 3;
        std::vector<float> texf(n_tex);
        for (size_t i = 0; i < n_tex; ++i) texf[i] = (float)d.albedo_textures[i] / 255.0f;   // UNORM8 -> float, as the oracle does per fetch
        if ((rc = upload_shared<float2>(s, kSharedTexcoords, texcoords, n_texcoords, st)) || (rc = upload_shared<float>(s, kSharedTextures, texf.data(), n_tex))) return rc;
        s->tex_width = (int32_t)d.tex_width; s->tex_height = (int32_t)d.tex_height; s->n_textures = (int32_t)d.n_textures;
    }
    return CRT_OK;
}

// Pre-gathered intersection records (v0 | original id) (e1 | slot) (e2 | material) of the n listed slots of the triangle array (`slots`
// null: slots 0 .. n - 1 in order).  e1 = v1 - v0, e2 = v2 - v0 are the subtractions of path_trace.fs:337-338, done once here;
// scene_build.hip make_record gives the same bits on the device.
std::vector<float4> intersection_records(const float* vertices, const crt_triangle* triangles, const int32_t* orig_ids, const int32_t* slots, size_t n) {
    std::vector<float4> recs(3 * n);
    for (size_t i = 0; i < n; ++i) {
        const int32_t slot = slots ? slots[i] : (int32_t)i;
        const crt_triangle& t = triangles[slot];
        const float* v0 = vertices + 3 * (size_t)t.v[0];
        const float* v1 = vertices + 3 * (size_t)t.v[1];
        const float* v2 = vertices + 3 * (size_t)t.v[2];
        const int32_t id = orig_ids ? orig_ids[slot] : slot;
        float4 a, b, c;
        a.x = v0[0]; a.y = v0[1]; a.z = v0[2]; std::memcpy(&a.w, &id, 4);
        b.x = v1[0] - v0[0]; b.y = v1[1] - v0[1]; b.z = v1[2] - v0[2]; std::memcpy(&b.w, &slot, 4);
        c.x = v2[0] - v0[0]; c.y = v2[1] - v0[1]; c.z = v2[2] - v0[2]; std::memcpy(&c.w, &t.v[3], 4);
        recs[3 * i] = a; recs[3 * i + 1] = b; recs[3 * i + 2] = c;
    }
    return recs;
}

// device, stream, environment overrides and the descriptor's scalars: shared by every way of creating a scene
int init_scene_common(crt_scene* s, const crt_scene_desc* d) {
    if (hipGetDevice(&s->device) != hipSuccess) return (fail(CRT_ERR_HIP, "hipGetDevice failed"));
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, s->device) == hipSuccess) s->n_cu = prop.multiProcessorCount;
    if (const char* e = std::getenv("CRT_TIMING")) s->timing = (uint32_t)std::max(0, std::atoi(e));
    if (hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess) return (fail(CRT_ERR_HIP, "hipStreamCreate failed"));
    s->width = d->width; s->height = d->height; s->max_depth = d->max_depth; s->n_lights = (uint32_t)d->n_lights;
    s->n_vertices = d->n_vertices; s->n_normals = d->n_normals; s->n_slots = d->n_triangles;
    if (d->n_vertices) {
        for (int k = 0; k < 3; ++k) s->bounds_lo[k] = s->bounds_hi[k] = d->vertices[k];
        for (size_t i = 1; i < d->n_vertices; ++i)
            for (int k = 0; k < 3; ++k) {
                s->bounds_lo[k] = std::min(s->bounds_lo[k], d->vertices[3 * i + k]);
                s->bounds_hi[k] = std::max(s->bounds_hi[k], d->vertices[3 * i + k]);
            }
    }
    for (size_t m = 0; m < d->n_materials; ++m)
        s->special_materials = s->special_materials || d->materials[m].albedo[3] == 1.0f || d->materials[m].albedo[3] == 17.0f;
    return CRT_OK;
}

}  // namespace

// every field of a light (p, u, v, n, e, area_pdf: 18 floats) is finite
bool crt::light_finite(const crt_light& l) {
    const float* f = l.p;
    for (int k = 0; k < 18; ++k) if (!std::isfinite(f[k])) return false;
    return true;
}

int crt::finish_scene_setup(crt_scene* s) {
    int rc;
    if (!s->rows_padded) {           // a replica's buffers arrive padded (crt_set_devices copies them as they are)
        if ((rc = pad_rows(s->stream, "crt_scene_create: ", &s->d_nodes, 5u, (uint32_t)CRT_NODE_ROWS, (size_t)s->info.n_nodes8))) return rc;
        if ((rc = pad_rows(s->stream, "crt_scene_create: ", &s->d_tris, 3u, (uint32_t)CRT_TRI_ROWS, (size_t)s->info.n_tris8))) return rc;
        s->rows_padded = true;
    }
    // (the float planes of the uniform node steps: ensure_planes, at the first frame that walks the CWBVH)
    if ((rc = dev_alloc(&s->d_overflow, 1))) return rc;
    if (hipMemset(s->d_overflow, 0, sizeof(uint32_t)) != hipSuccess) return fail(CRT_ERR_HIP, "hipMemset failed");
    if ((rc = dev_alloc(&s->d_counts, 2 * kCounters))) return rc;
    s->spans.resize(kMaxEvents);                 // events themselves: created by new_span when a timing option first needs them
    return CRT_OK;
}

// Publishes a built tree into the scene: its arrays, counts, depths, stack bounds, build times, and the replica table's sizes at the
// traversal's strides (a create pads its arrays right after, finish_scene_setup; a rebuild has padded them).  The scene's previous arrays,
// if any, are left in `t`, which frees them.  The stream has drained: a BVH2 too deep to walk is freed here.  Cannot fail.
void crt::adopt_tree(crt_scene* s, crt::DeviceTree& t) {
    if (!t.keep_bvh2() && t.bvh2) { (void)hipFree(t.bvh2); t.bvh2 = nullptr; }
    std::swap(s->d_bvh2, t.bvh2); std::swap(s->d_nodes, t.nodes); std::swap(s->d_tris, t.tris);
    std::swap(s->d_triangles, t.triangles); std::swap(s->d_tris2, t.tris2);
    const size_t n2 = 2 * (size_t)t.n - 1;
    s->bvh2_stack = crt::bvh2_stack_entries(t.depth2);
    s->stack_entries = t.stack_entries();
    s->tree_validated = false;                    // the device builders' own tree never went through validate_cwbvh: the checked pushes
    s->info.n_nodes8 = t.n8; s->info.n_tris8 = t.n; s->info.n_bvh2_nodes = n2; s->info.max_depth8 = t.depth8; s->info.bvh2_depth = t.depth2;
    s->info.build_lbvh_device_ms = t.lbvh_ms; s->info.build_convert_device_ms = t.conv_ms;
    s->shared_bytes[kSharedNodes] = (size_t)t.n8 * CRT_NODE_ROWS * 16;
    s->shared_bytes[kSharedTris] = (size_t)t.n * CRT_TRI_ROWS * 16;
    s->shared_bytes[kSharedTriangles] = (size_t)t.n * sizeof(crt_triangle);
    s->shared_bytes[kSharedBvh2] = s->d_bvh2 ? n2 * sizeof(crt_flatnode) : 0;
    s->shared_bytes[kSharedTris2] = s->d_bvh2 ? (size_t)t.n * 3 * sizeof(float4) : 0;
    if (t.planes) {                               // a scene without planes still builds them at its first CWBVH frame (ensure_planes)
        std::swap(s->d_planes, t.planes);
        s->shared_bytes[kSharedPlanes] = (size_t)t.n8 * 12 * sizeof(float4);
    }
}

// CRT_BUILD_LBVH_ON_DEVICE: upload the seven input arrays once, then LBVH -> CWBVH -> leaf-order triangles and intersection
// records without anything leaving HBM (the host-array entry points crt_lbvh_build / crt_cwbvh_convert_device moved 64 MB
// of FlatNodes over PCIe twice at 1 M triangles).  Temporaries of both builders come from one arena allocation.
static int scene_create_device_built(const crt_scene_desc* d, crt_scene** out) {
    const auto t_begin = std::chrono::steady_clock::now();
    // (the FlatNode array of a scene built here never leaves the device: links of 2^24 or more are kept as bit patterns, host/flatnode_link.hpp)
    if (2ull * d->n_triangles >= crt::kMaxLinkBits) return fail(CRT_ERR_LIMIT, "crt_scene_create: more than 2^29 triangles");
    const bool have_tex = d->albedo_textures && d->n_textures > 0;
    std::unique_ptr<crt_scene> owner(new (std::nothrow) crt_scene);
    crt_scene* s = owner.get();
    if (!s) return fail(CRT_ERR_NOMEM, "crt_scene_create: out of memory");
    int rc = init_scene_common(s, d);
    if (rc) return rc;
    const uint32_t n = (uint32_t)d->n_triangles;
    hipStream_t st = s->stream;

    crt::DeviceArena arena;                       // input-order triangles + both builders' temporaries; gone when this returns
    auto P = crt::DeviceArena::padded;
    s->gpu_build_flags = crt::gpu_flags_of(d->build_flags);
    hipError_t he = arena.reserve(P((size_t)n * sizeof(crt_triangle)) + P(4) + crt::device_tree_tmp_bytes(n, s->gpu_build_flags));
    if (he != hipSuccess) return fail(CRT_ERR_NOMEM, std::string("crt_scene_create: hipMalloc: ") + hipGetErrorString(he));
    crt_triangle* d_in = arena.take<crt_triangle>(n);
    uint32_t* d_flag = arena.take<uint32_t>(1);

    // everything the caller owns goes up asynchronously, on the scene's stream
    float* d_verts = nullptr;
    struct Guard { void* p = nullptr; ~Guard() { if (p) (void)hipFree(p); } } verts_guard;
    if ((rc = upload(&d_verts, d->vertices, d->n_vertices * 3, st))) return rc;
    verts_guard.p = d_verts;                      // only the builders and the gather kernels read the vertices
    if (hipMemcpyAsync(d_in, d->triangles, (size_t)n * sizeof(crt_triangle), hipMemcpyHostToDevice, st) != hipSuccess)
        return fail(CRT_ERR_HIP, "hipMemcpy H2D failed");
    if ((rc = upload_shading(s, *d, d->normals, d->n_normals, d->texcoords, d->n_texcoords, st))) return rc;
    if (hipMemsetAsync(d_flag, 0, 4, st) != hipSuccess) return fail(CRT_ERR_HIP, "hipMemset failed");
    crt::launch_validate_triangles(d_in, n, (uint32_t)d->n_vertices, (uint32_t)d->n_materials, d->normals ? (uint32_t)d->n_normals : 0u,
                                   (uint32_t)d->n_texcoords, reinterpret_cast<const float*>(s->d_materials), have_tex ? 1 : 0, d_flag, st);
    uint32_t flag = 0;
    if (hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return fail(CRT_ERR_HIP, "crt_scene_create: triangle validation failed to run");
    const float upload_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    if (flag)
        return fail(CRT_ERR_INVALID, std::string("crt_scene_create: ") + ((flag & 1u) ? "vertex" : (flag & 2u) ? "material" : (flag & 4u) ? "normal" : "texcoord") +
                                         " index out of range");

    // BVH2 (kept: it is the FlatNode array the BVH2 frame mode and CRT_TRACE_BVH2 walk) -> CWBVH
    crt::warm_wait();                             // the builders' code objects: loaded by now, or being loaded by that thread
    crt::DeviceTree tree;
    if ((rc = dev_alloc(&tree.bvh2, (2 * (size_t)n - 1) * 2))) return rc;
    if ((rc = crt::build_device_tree(d_in, d_verts, n, s->gpu_build_flags, arena, reinterpret_cast<crt_flatnode*>(tree.bvh2), crt::kSceneTree, st,
                                     "crt_scene_create: ", &tree))) return rc;
    if (hipStreamSynchronize(st) != hipSuccess || hipGetLastError() != hipSuccess) return fail(CRT_ERR_HIP, "crt_scene_create: scene assembly kernels failed");
    crt::adopt_tree(s, tree);                     // packed: finish_scene_setup pads to the traversal's strides
    s->info.built_on_device = 1u;
    s->info.build_upload_ms = upload_ms;
    if ((rc = crt::finish_scene_setup(s))) return rc;
    s->info.build_wall_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    *out = owner.release();
    return CRT_OK;
}

static int scene_create_impl(const crt_scene_desc* d, crt_scene** out) {
    const std::string who = "crt_scene_create: ";
    if (!out) return fail(CRT_ERR_INVALID, who + "null out");
    *out = nullptr;
    if (!d) return fail(CRT_ERR_INVALID, who + "null desc");
    if (d->abi_version != CRT_ABI_VERSION) return fail(CRT_ERR_INVALID, who + "abi_version mismatch");
    if (!d->vertices || !d->triangles || d->n_triangles == 0 || d->n_vertices == 0) return fail(CRT_ERR_INVALID, who + "vertices/triangles missing");
    if (!d->materials || d->n_materials == 0) return fail(CRT_ERR_INVALID, who + "materials missing");
    if (d->n_lights && !d->lights) return fail(CRT_ERR_INVALID, who + "lights missing");
    if (!d->bvh && !d->bvh8 && !(d->build_flags & CRT_BUILD_LBVH_ON_DEVICE))
        return fail(CRT_ERR_INVALID, who + "neither bvh nor bvh8 given (and build_flags does not ask for a build on the device)");
    if ((d->build_flags & CRT_BUILD_LBVH_ON_DEVICE) && (d->bvh || d->bvh8 || d->tri_orig_ids))
        return fail(CRT_ERR_INVALID, who + "CRT_BUILD_LBVH_ON_DEVICE takes the triangles in source order, without bvh / bvh8 / tri_orig_ids");
    if (d->build_flags & ~(uint32_t)(CRT_BUILD_LBVH_ON_DEVICE | CRT_BUILD_PLOC | CRT_BUILD_SAH | 0xff00u)) return fail(CRT_ERR_INVALID, who + "unknown build_flags");
    if ((d->build_flags & (CRT_BUILD_PLOC | CRT_BUILD_SAH | 0xff00u)) && !(d->build_flags & CRT_BUILD_LBVH_ON_DEVICE))
        return fail(CRT_ERR_INVALID, who + "CRT_BUILD_PLOC / CRT_BUILD_SAH only qualify CRT_BUILD_LBVH_ON_DEVICE");
    int rc = check_descriptor(who, *d, !d->texcoords, d->n_lights);
    if (rc) return rc;
    if (d->n_triangles >= (1ull << 31) || d->n_vertices >= (1ull << 31)) return fail(CRT_ERR_LIMIT, who + "too many elements");

    // index validation: a bad index would be an out-of-bounds device access (build-on-device scenes run the same checks
    // as a kernel over the uploaded array, scene_create_device_built)
    const bool host_checks = !(d->build_flags & CRT_BUILD_LBVH_ON_DEVICE);
    for (size_t i = 0; host_checks && i < d->n_triangles; ++i) {
        const crt_triangle& t = d->triangles[i];
        for (int j = 0; j < 3; ++j)
            if (t.v[j] < 0 || (size_t)t.v[j] >= d->n_vertices) return fail(CRT_ERR_INVALID, who + "vertex index out of range");
        if (t.v[3] < 0 || (size_t)t.v[3] >= d->n_materials) return fail(CRT_ERR_INVALID, who + "material index out of range");
        if (t.vn[3] != 0)
            for (int j = 0; j < 3; ++j)
                if (t.vn[j] < 0 || (size_t)t.vn[j] >= d->n_normals || !d->normals) return fail(CRT_ERR_INVALID, who + "normal index out of range");
    }
    // a non-finite vertex turns boxes and areas into NaN (the GPU builders check the same on the device)
    for (size_t i = 0; i < 3 * d->n_vertices; ++i)
        if (!(std::fabs(d->vertices[i]) <= 1.0e18f)) return fail(CRT_ERR_INVALID, who + "a vertex coordinate is not finite or exceeds 1e18");
    if (d->albedo_textures && d->n_textures > 0 && host_checks)
        for (size_t i = 0; i < d->n_triangles; ++i) {
            const crt_triangle& t = d->triangles[i];
            if (d->materials[t.v[3]].tex_ind[0] == -1.0f) continue;
            for (int j = 0; j < 3; ++j)
                if (t.vt[j] < 0 || (size_t)t.vt[j] >= d->n_texcoords) return fail(CRT_ERR_INVALID, who + "texcoord index out of range");
        }
    if ((rc = require_device())) return rc;
    {   // the library's other code objects load in the background while this scene is uploaded (crt_device.cpp Warmer)
        int dev = 0;
        if (hipGetDevice(&dev) == hipSuccess) crt::warm_start(dev);
    }
    if (d->build_flags & CRT_BUILD_LBVH_ON_DEVICE) return scene_create_device_built(d, out);

    // CWBVH: take the caller's, or convert the BVH2 (cwbvh.h:58)
    crt::CWBVH conv;
    const crt_node8* nodes8 = d->bvh8;
    size_t n_nodes8 = d->n_bvh8;
    const int32_t* tri_slots = d->bvh8_tri_slots;
    size_t n_tris8 = d->n_bvh8_tris;
    uint32_t depth8 = 0;
    struct HandleGuard { crt_cwbvh* h = nullptr; ~HandleGuard() { if (h) crt_cwbvh_free(h); } } dev_conv;
    if (!nodes8 && d->n_bvh >= 4096) {
        // big trees: the device converter (same bytes as the host one, ~20x faster at 1 M triangles)
        rc = crt_cwbvh_convert_device(d->bvh, d->n_bvh, d->n_triangles, &dev_conv.h);
        if (rc) return fail(rc, who + "BVH2 -> CWBVH failed: " + crt_last_error());
        nodes8 = crt_cwbvh_nodes(dev_conv.h); n_nodes8 = crt_cwbvh_num_nodes(dev_conv.h);
        tri_slots = crt_cwbvh_tri_slots(dev_conv.h); n_tris8 = crt_cwbvh_num_tris(dev_conv.h);
    } else if (!nodes8) {
        if (!conv.convert(d->bvh, d->n_bvh, d->n_triangles, d->tri_orig_ids)) return fail(CRT_ERR_INVALID, who + "BVH2 -> CWBVH failed: " + conv.error);
        nodes8 = conv.nodes.data(); n_nodes8 = conv.nodes.size();
        tri_slots = conv.tri_slots.data(); n_tris8 = conv.tri_slots.size();
    } else if (!tri_slots) {
        return fail(CRT_ERR_INVALID, who + "bvh8 given without bvh8_tri_slots");
    }
    {
        std::string why = crt::validate_cwbvh(nodes8, n_nodes8, n_tris8, CRT_STACK_ENTRIES, &depth8);
        if (!why.empty()) return fail(why.find("deeper") != std::string::npos ? CRT_ERR_LIMIT : CRT_ERR_INVALID, who + "CWBVH rejected: " + why);
        for (size_t i = 0; i < n_tris8; ++i)
            if (tri_slots[i] < 0 || (size_t)tri_slots[i] >= d->n_triangles) return fail(CRT_ERR_INVALID, who + "bvh8_tri_slots entry out of range");
    }

    // the traversal loops address node and record rows as base + a 32-bit byte offset (rt_kernels.hip node_rows / tri_rows)
    if (n_nodes8 * (uint64_t)(CRT_NODE_ROWS * 16) >= (1ull << 32) || n_tris8 * (uint64_t)(CRT_TRI_ROWS * 16) >= (1ull << 32))
        return fail(CRT_ERR_LIMIT, who + "CWBVH node or triangle-record array of 4 GiB or more (53 M nodes / 89 M records)");
    std::unique_ptr<crt_scene> owner(new (std::nothrow) crt_scene);   // freed on every early return and on a throw
    crt_scene* s = owner.get();
    if (!s) return fail(CRT_ERR_NOMEM, who + "out of memory");
    if ((rc = init_scene_common(s, d))) return rc;
    s->stack_entries = crt::cwbvh_stack_entries(depth8);
    s->tree_validated = true;                     // validate_cwbvh above walked every node and reported this depth
    s->info.n_nodes8 = n_nodes8; s->info.n_tris8 = n_tris8; s->info.n_bvh2_nodes = d->n_bvh; s->info.max_depth8 = depth8;

    // nodes and records (CWBVH triangle order) go up packed; finish_scene_setup pads them to the traversal's strides, and a replica copies those
    const std::vector<float4> recs = intersection_records(d->vertices, d->triangles, d->tri_orig_ids, tri_slots, n_tris8);
    if ((rc = upload(&s->d_nodes, nodes8, n_nodes8 * 5)) || (rc = upload(&s->d_tris, recs.data(), recs.size()))) return rc;
    s->shared_bytes[kSharedNodes] = n_nodes8 * (size_t)CRT_NODE_ROWS * 16;
    s->shared_bytes[kSharedTris] = n_tris8 * (size_t)CRT_TRI_ROWS * 16;
    if ((rc = upload_shared<int4>(s, kSharedTriangles, d->triangles, d->n_triangles * 3)) ||
        (rc = upload_shading(s, *d, d->normals, d->n_normals, d->texcoords, d->n_texcoords, nullptr)))
        return rc;
    if (d->bvh) {
        // the BVH2 itself, for the reference-order walk (crt_trace with CRT_TRACE_BVH2): nodes as uploaded, one
        // intersection record per leaf slot, and the stack bound from the tree's depth
        std::vector<uint32_t> level(d->n_bvh, 0);
        uint32_t depth2 = 0;
        for (size_t i = 0; i < d->n_bvh; ++i) {
            if (d->bvh[i].bmax[3] != 0.0f) {
                // leaf: traverse_bvh2 loops over [start, start + range) of the slot-ordered records, so the range must lie
                // inside the triangle array (range <= 255 is the builder's own bit-field cap, FlatNode.h:24-25)
                const float fs = d->bvh[i].bmin[3], fr = d->bvh[i].bmax[3];
                if (!(fr >= 1.0f && fr <= 255.0f) || !(fs >= 0.0f && fs < 16777216.0f) || (size_t)fs + (size_t)fr > d->n_triangles)
                    return fail(CRT_ERR_INVALID, who + "BVH2 leaf range outside the triangle array");
                depth2 = std::max(depth2, level[i]);
                continue;
            }
            const float fl = d->bvh[i].bmin[3];
            if (!(fl >= 0.0f && fl < 16777216.0f)) return fail(CRT_ERR_INVALID, who + "BVH2 child link out of order");
            const size_t l = (size_t)fl;
            if (l <= i || l + 1 >= d->n_bvh) return fail(CRT_ERR_INVALID, who + "BVH2 child link out of order");
            level[l] = level[l + 1] = level[i] + 1;
        }
        s->bvh2_stack = crt::bvh2_stack_entries(depth2);
        if (!s->bvh2_stack) return fail(CRT_ERR_LIMIT, who + "BVH2 deeper than 94 levels");
        s->info.bvh2_depth = depth2;              // a scene built on the device reports its own (adopt_tree)
        const std::vector<float4> rec2 = intersection_records(d->vertices, d->triangles, d->tri_orig_ids, nullptr, d->n_triangles);
        if ((rc = upload_shared<float4>(s, kSharedBvh2, d->bvh, d->n_bvh * 2)) || (rc = upload_shared<float4>(s, kSharedTris2, rec2.data(), rec2.size()))) return rc;
    }
    if ((rc = crt::finish_scene_setup(s))) return rc;
    *out = owner.release();
    return CRT_OK;
}

// A scene whose geometry is a live crt_instances handle: the shading's copies of every mesh's triangles, normals and
// texcoords, one mesh after the other with a per-mesh table of where each starts, and the binding.  Checks are crt_scene_create's, per mesh.
static int scene_create_instanced_impl(const crt_instanced_scene_desc* d, const struct crt_mesh_lights* mesh_lights, crt_scene** out) {
    const std::string who = mesh_lights ? "crt_scene_create_instanced_lit: " : "crt_scene_create_instanced: ";
    if (!out) return fail(CRT_ERR_INVALID, who + "null out");
    *out = nullptr;
    if (!d) return fail(CRT_ERR_INVALID, who + "null desc");
    if (d->abi_version != CRT_ABI_VERSION) return fail(CRT_ERR_INVALID, who + "abi_version mismatch");
    if (!d->instances) return fail(CRT_ERR_INVALID, who + "null instances handle");
    if (!d->meshes || d->n_meshes == 0) return fail(CRT_ERR_INVALID, who + "meshes missing");
    if (!d->materials || d->n_materials == 0) return fail(CRT_ERR_INVALID, who + "materials missing");
    if (d->n_lights && !d->lights) return fail(CRT_ERR_INVALID, who + "lights missing");
    int rc = require_device();
    if (rc) return rc;
    crt::InstancesView v{};
    crt::instances_view(d->instances, &v);
    if (d->n_meshes != v.n_meshes)
        return fail(CRT_ERR_INVALID, who + "n_meshes (" + std::to_string(d->n_meshes) + ") differs from the handle's mesh count (" + std::to_string(v.n_meshes) + ")");
    // lights that follow the instances: a scene has them when some mesh carries one
    size_t max_nl = 0, n_obj = 0;
    if (mesh_lights)
        for (uint32_t k = 0; k < d->n_meshes; ++k) {
            if (mesh_lights[k].n_lights && !mesh_lights[k].lights) return fail(CRT_ERR_INVALID, who + "mesh " + std::to_string(k) + ": null lights");
            max_nl = std::max(max_nl, mesh_lights[k].n_lights); n_obj += mesh_lights[k].n_lights;
        }
    const bool lit = max_nl > 0;
    if (lit) {
        if ((uint64_t)d->n_lights + (uint64_t)std::max(v.capacity, 1u) * max_nl >= (1ull << 31)) return fail(CRT_ERR_LIMIT, who + "the world light table could exceed 2^31 lights");
        for (size_t i = 0; i < d->n_lights; ++i)
            if (!crt::light_finite(d->lights[i])) return fail(CRT_ERR_INVALID, who + "a field of light " + std::to_string(i) + " is not finite");
        for (uint32_t k = 0; k < d->n_meshes; ++k)
            for (size_t i = 0; i < mesh_lights[k].n_lights; ++i)
                if (!crt::light_finite(mesh_lights[k].lights[i])) return fail(CRT_ERR_INVALID, who + "mesh " + std::to_string(k) + ": a field of light " + std::to_string(i) + " is not finite");
    }
    // an emissive material names a static light or, on a light-bearing mesh, one of the mesh's own: per triangle below
    if ((rc = check_descriptor(who, *d, false, lit ? std::max(d->n_lights, max_nl) : d->n_lights))) return rc;
    const bool have_tex = d->albedo_textures && d->n_textures > 0;
    size_t n_tris = 0, n_normals = 0, n_texcoords = 0;
    std::vector<uint4> base(d->n_meshes), mesh_mtl(d->n_meshes);
    for (uint32_t k = 0; k < d->n_meshes; ++k) {
        const crt_mesh_shading& m = d->meshes[k];
        const std::string mesh = "mesh " + std::to_string(k) + ": ";
        if (!m.triangles || m.n_triangles != crt::instances_mesh_triangles(d->instances, k))
            return fail(CRT_ERR_INVALID, who + mesh + "n_triangles differs from the handle's mesh (or triangles is null)");
        if ((m.n_normals && !m.normals) || (m.n_texcoords && !m.texcoords)) return fail(CRT_ERR_INVALID, who + mesh + "null normals / texcoords");
        for (size_t i = 0; i < 3 * m.n_normals; ++i)
            if (!std::isfinite(m.normals[i])) return fail(CRT_ERR_INVALID, who + mesh + "a normal is not finite");
        uint32_t mtl_lo = 0xffffffffu, mtl_hi = 0u, vt_ok = 1u;
        for (size_t i = 0; i < m.n_triangles; ++i) {
            const crt_triangle& t = m.triangles[i];
            if (t.v[3] < 0 || (size_t)t.v[3] >= d->n_materials) return fail(CRT_ERR_INVALID, who + mesh + "material index out of range");
            if (lit) {                       // the triangle's own material (offset 0): mesh-local on a light-bearing mesh, else a static light
                const float ew = d->materials[t.v[3]].emission[3];
                const size_t nl = mesh_lights[k].n_lights;
                if (ew != -1.0f && (size_t)ew >= (nl ? nl : d->n_lights))
                    return fail(CRT_ERR_INVALID, who + mesh + (nl ? "an emissive triangle refers to a light its mesh does not carry"
                                                                  : "an emissive triangle of a mesh without lights refers to a static light that does not exist"));
            }
            mtl_lo = std::min(mtl_lo, (uint32_t)t.v[3]); mtl_hi = std::max(mtl_hi, (uint32_t)t.v[3]);
            for (int j = 0; j < 3; ++j)
                if (t.vt[j] < 0 || (size_t)t.vt[j] >= m.n_texcoords) vt_ok = 0u;
            if (t.vn[3] != 0)
                for (int j = 0; j < 3; ++j)
                    if (t.vn[j] < 0 || (size_t)t.vn[j] >= m.n_normals) return fail(CRT_ERR_INVALID, who + mesh + "normal index out of range");
            if (have_tex && d->materials[t.v[3]].tex_ind[0] != -1.0f)
                for (int j = 0; j < 3; ++j)
                    if (t.vt[j] < 0 || (size_t)t.vt[j] >= m.n_texcoords) return fail(CRT_ERR_INVALID, who + mesh + "texcoord index out of range");
        }
        base[k] = make_uint4((uint32_t)n_tris, (uint32_t)n_normals, (uint32_t)n_texcoords, lit ? (uint32_t)mesh_lights[k].n_lights : 0u);
        mesh_mtl[k] = make_uint4(mtl_lo, mtl_hi, vt_ok, 0u);
        n_tris += m.n_triangles; n_normals += m.n_normals; n_texcoords += m.n_texcoords;
    }
    if (n_tris >= (1ull << 31) || n_normals >= (1ull << 31) || n_texcoords >= (1ull << 31)) return fail(CRT_ERR_LIMIT, who + "too many elements");
    // the rule for material offsets (include/crt.h): a material is textured when the shading would read texcoords for it
    if (d->n_materials >= (1ull << 31)) return fail(CRT_ERR_LIMIT, who + "too many materials");
    std::vector<uint32_t> tex_before(d->n_materials + 1, 0u);
    for (size_t m = 0; m < d->n_materials; ++m) tex_before[m + 1] = tex_before[m] + ((have_tex && d->materials[m].tex_ind[0] != -1.0f) ? 1u : 0u);
    HIPCHK(hipSetDevice(v.device));
    std::unique_ptr<crt_scene> owner(new (std::nothrow) crt_scene);
    crt_scene* s = owner.get();
    if (!s) return fail(CRT_ERR_NOMEM, who + "out of memory");
    crt_scene_desc common{};                 // what init_scene_common reads: the frame's scalars and the materials
    common.width = d->width; common.height = d->height; common.max_depth = d->max_depth; common.n_lights = d->n_lights;
    common.materials = d->materials; common.n_materials = d->n_materials; common.n_triangles = n_tris; common.n_normals = n_normals;
    if ((rc = init_scene_common(s, &common))) return rc;
    std::vector<crt_triangle> tris(n_tris);
    std::vector<float> normals(3 * n_normals), texcoords(2 * n_texcoords);
    for (uint32_t k = 0; k < d->n_meshes; ++k) {
        const crt_mesh_shading& m = d->meshes[k];
        std::copy(m.triangles, m.triangles + m.n_triangles, tris.begin() + base[k].x);
        if (m.n_normals) std::copy(m.normals, m.normals + 3 * m.n_normals, normals.begin() + 3 * (size_t)base[k].y);
        if (m.n_texcoords) std::copy(m.texcoords, m.texcoords + 2 * m.n_texcoords, texcoords.begin() + 2 * (size_t)base[k].z);
    }
    if ((rc = upload(&s->d_triangles, tris.data(), n_tris * 3)) || (rc = upload_shading(s, *d, normals.data(), n_normals, texcoords.data(), n_texcoords, nullptr)) ||
        (rc = upload(&s->d_mesh_base, base.data(), base.size())) || (rc = upload(&s->d_mesh_mtl, mesh_mtl.data(), mesh_mtl.size())) ||
        (rc = upload(&s->d_tex_before, tex_before.data(), tex_before.size())))
        return rc;
    std::fill(std::begin(s->shared_bytes), std::end(s->shared_bytes), size_t(0));     // an instanced scene never replicates: it lists nothing
    if (lit) {
        // the static lights, every mesh's object-space lights and the scan's arrays; the world table itself (d_lights, which holds the
        // static lights for now) is sized and filled by the first rebuild
        s->lit = new (std::nothrow) SceneLights;
        SceneLights* L = s->lit;
        if (!L) return fail(CRT_ERR_NOMEM, who + "out of memory");
        L->n_static = (uint32_t)d->n_lights;
        L->table_cap = d->n_lights;
        L->mesh.resize(d->n_meshes);
        L->obj.reserve(n_obj);
        for (uint32_t k = 0; k < d->n_meshes; ++k) {
            L->mesh[k] = make_uint2((uint32_t)L->obj.size(), (uint32_t)mesh_lights[k].n_lights);
            L->obj.insert(L->obj.end(), mesh_lights[k].lights, mesh_lights[k].lights + mesh_lights[k].n_lights);
        }
        const size_t cap = std::max(v.capacity, 1u);
        if ((rc = upload(&L->d_static, d->lights, d->n_lights * 18)) || (rc = upload(&L->d_obj, L->obj.data(), n_obj * 18)) ||
            (rc = upload(&L->d_mesh, L->mesh.data(), L->mesh.size())) || (rc = dev_alloc(&L->d_first, cap)) ||
            (rc = dev_alloc(&L->d_block_sums, (cap + 1023) / 1024)) || (rc = dev_alloc(&L->d_total, 1)))
            return rc;
    }
    s->rows_padded = true;                   // no tree of its own
    if ((rc = crt::finish_scene_setup(s))) return rc;
    if ((rc = crt::instances_bind(d->instances, s->stream, crt::InstOffsetRule{s->d_mesh_mtl, s->d_tex_before, (uint32_t)d->n_materials}))) return rc;
    s->inst = d->instances;
    *out = owner.release();
    return CRT_OK;
}

// nothing may unwind through the C ABI: the vectors built during upload can throw bad_alloc / length_error
template <typename F>
static int no_throw(const char* who, crt_scene** out, F&& create) {
    try {
        return create();
    } catch (const std::exception& e) {
        if (out) *out = nullptr;
        return fail(CRT_ERR_NOMEM, std::string(who) + e.what());
    }
}

extern "C" {

int crt_scene_create(const crt_scene_desc* d, crt_scene** out) {
    return no_throw("crt_scene_create: ", out, [&] { return scene_create_impl(d, out); });
}

int crt_scene_create_instanced(const crt_instanced_scene_desc* d, crt_scene** out) {
    return no_throw("crt_scene_create_instanced: ", out, [&] { return scene_create_instanced_impl(d, nullptr, out); });
}

int crt_scene_create_instanced_lit(const crt_instanced_scene_desc* d, const struct crt_mesh_lights* mesh_lights, crt_scene** out) {
    return no_throw("crt_scene_create_instanced_lit: ", out, [&] { return scene_create_instanced_impl(d, mesh_lights, out); });
}

int crt_scene_destroy(crt_scene* s) {
    delete s;
    return CRT_OK;
}

}  // extern "C"
