// The host side of the deformer (include/crt.h crt_deformer_create .. crt_deform_host): the checks of a desc and of a
// pose, the per-target morph lists turned into one list per vertex, the handle with everything it holds in HBM, the pose on the
// deformer's stream or on a scene's, and the same arithmetic on the CPU (host/deform_math.hpp, which deform.hip includes).
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "crt_scene.hpp"
#include "deform.hpp"
#include "host/deform_math.hpp"

using crt::dev_alloc;
using crt::fail;

// Everything a deformer holds, allocated by crt_deformer_create; a pose allocates nothing.
struct crt_deformer {
    int device = 0;
    hipStream_t stream = nullptr;
    crt::DeformArgs args{};                  // the kernel's arguments: every pointer below, fixed at create
    int form = crt::kDeformPaletteGlobal;    // how the kernel reads the palette
    void* bufs[11] = {};                     // the device allocations behind args, for the destructor
    float* d_pose = nullptr;                 // 12 * n_bones floats of palette, then n_targets morph weights
    float* h_pose = nullptr;                 // the same, pinned: a pose is copied from here
    size_t pose_floats = 0;
    uint32_t n_targets = 0;
    hipEvent_t ev_copy = nullptr;            // the last pose's copy has left h_pose
    hipEvent_t ev_a = nullptr, ev_b = nullptr;   // around the last pose's kernel
    hipEvent_t ev_reader = nullptr;          // crt_deform_scene: the scene's stream is done reading the outputs
    hipEvent_t ev_own = nullptr;             // crt_deform_scene: where the deformer's own stream stood when the call began
    bool reader_pending = false, posed = false, times_pending = false;
    float device_ms = 0.f;
    ~crt_deformer() {                        // on the deformer's device, its streams drained
        for (void* p : bufs) if (p) (void)hipFree(p);
        if (d_pose) (void)hipFree(d_pose);
        if (h_pose) (void)hipHostFree(h_pose);
        for (hipEvent_t e : {ev_copy, ev_a, ev_b, ev_reader, ev_own}) if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace {

bool all_finite(const float* p, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(p[i])) return false;
    return true;
}

// one list of morph entries per vertex, in ascending target order
struct MorphLists {
    std::vector<uint32_t> first;             // n_vertices + 1; empty when no target lists anything
    std::vector<crt::DeformMorph> entry;
};

// The checks of crt_deformer_create and crt_deform_host; *n_entries: the number of morph entries
int check_desc(const crt_deformer_desc* d, const std::string& who, size_t* n_entries) {
    constexpr size_t kMax = (size_t)1 << 31;
    if (!d) return fail(CRT_ERR_INVALID, who + "null desc");
    if (d->abi_version != CRT_ABI_VERSION) return fail(CRT_ERR_INVALID, who + "abi_version differs from CRT_ABI_VERSION");
    if (d->n_vertices == 0 || d->n_vertices >= kMax) return fail(CRT_ERR_INVALID, who + "n_vertices is 0 or at least 2^31");
    if (d->n_normals >= kMax) return fail(CRT_ERR_INVALID, who + "n_normals is at least 2^31");
    if (!d->rest_vertices || !d->vertex_bones || !d->vertex_weights) return fail(CRT_ERR_INVALID, who + "null rest_vertices, vertex_bones or vertex_weights");
    if (d->n_normals ? (!d->rest_normals || !d->normal_bones || !d->normal_weights) : (d->normal_bones || d->normal_weights))
        return fail(CRT_ERR_INVALID, who + "rest_normals, normal_bones and normal_weights are required exactly when n_normals > 0");
    if (d->n_bones < 1 || d->n_bones > 65536) return fail(CRT_ERR_INVALID, who + "n_bones outside 1..65536");
    if (d->n_targets > 65535) return fail(CRT_ERR_INVALID, who + "n_targets above 65535");
    size_t E = 0;
    if (d->n_targets) {
        if (!d->target_first) return fail(CRT_ERR_INVALID, who + "null target_first");
        if (d->target_first[0] != 0) return fail(CRT_ERR_INVALID, who + "target_first does not start at 0");
        for (uint32_t t = 0; t < d->n_targets; ++t)
            if (d->target_first[t + 1] < d->target_first[t]) return fail(CRT_ERR_INVALID, who + "target_first descends");
        E = d->target_first[d->n_targets];
        if (E >= kMax) return fail(CRT_ERR_INVALID, who + "at least 2^31 morph entries");
        if (E && (!d->target_vertex || !d->target_delta)) return fail(CRT_ERR_INVALID, who + "null target_vertex or target_delta");
    }
    for (size_t i = 0; i < 3 * d->n_vertices; ++i)
        if (!(std::fabs(d->rest_vertices[i]) <= 1e18f)) return fail(CRT_ERR_INVALID, who + "a rest position is not finite or exceeds 1e18");
    if (!all_finite(d->vertex_weights, 4 * d->n_vertices)) return fail(CRT_ERR_INVALID, who + "a vertex weight is not finite");
    for (size_t i = 0; i < 4 * d->n_vertices; ++i)
        if (d->vertex_bones[i] >= d->n_bones) return fail(CRT_ERR_INVALID, who + "a vertex bone index is out of range");
    if (d->n_normals) {
        if (!all_finite(d->rest_normals, 3 * d->n_normals)) return fail(CRT_ERR_INVALID, who + "a rest normal is not finite");
        if (!all_finite(d->normal_weights, 4 * d->n_normals)) return fail(CRT_ERR_INVALID, who + "a normal weight is not finite");
        for (size_t i = 0; i < 4 * d->n_normals; ++i)
            if (d->normal_bones[i] >= d->n_bones) return fail(CRT_ERR_INVALID, who + "a normal bone index is out of range");
    }
    if (E && !all_finite(d->target_delta, 3 * E)) return fail(CRT_ERR_INVALID, who + "a morph delta is not finite");
    for (uint32_t t = 0; t < d->n_targets; ++t)
        for (size_t e = d->target_first[t]; e < d->target_first[t + 1]; ++e) {
            if (d->target_vertex[e] >= d->n_vertices) return fail(CRT_ERR_INVALID, who + "a morph target lists a vertex out of range");
            if (e > d->target_first[t] && d->target_vertex[e] <= d->target_vertex[e - 1])
                return fail(CRT_ERR_INVALID, who + "the vertex indices of a morph target are not strictly ascending");
        }
    *n_entries = E;
    return CRT_OK;
}

int check_pose(uint32_t n_bones, uint32_t n_targets, const float* bones, const float* morph_weights, const std::string& who) {
    if (!bones) return fail(CRT_ERR_INVALID, who + "null bones");
    if (!all_finite(bones, 12 * (size_t)n_bones)) return fail(CRT_ERR_INVALID, who + "a bone matrix is not finite");
    if (morph_weights && !all_finite(morph_weights, n_targets)) return fail(CRT_ERR_INVALID, who + "a morph weight is not finite");
    return CRT_OK;
}

// a checked desc's targets, vertex by vertex: the targets are walked in ascending order, so every vertex's list is in target order
void morph_lists(const crt_deformer_desc* d, size_t E, MorphLists* out) {
    if (!E) return;
    out->first.assign(d->n_vertices + 1, 0u);
    for (size_t e = 0; e < E; ++e) ++out->first[d->target_vertex[e] + 1u];
    for (size_t v = 0; v < d->n_vertices; ++v) out->first[v + 1] += out->first[v];
    std::vector<uint32_t> cursor(out->first.begin(), out->first.end() - 1);
    out->entry.resize(E);
    for (uint32_t t = 0; t < d->n_targets; ++t)
        for (size_t e = d->target_first[t]; e < d->target_first[t + 1]; ++e)
            out->entry[cursor[d->target_vertex[e]]++] = crt::DeformMorph{{d->target_delta[3 * e], d->target_delta[3 * e + 1], d->target_delta[3 * e + 2]}, t};
}

// M of one element: its four (bone, weight) pairs over the palette
void blend_host(const uint16_t* b, const float* w, const float* bones, float M[12]) {
    crt::dm::blend_first(M, w[0], bones + 12 * (size_t)b[0]);
    for (int k = 1; k < 4; ++k)
        if (w[k] != 0.0f) crt::dm::blend_add(M, w[k], bones + 12 * (size_t)b[k]);
}

template <typename T>
int upload(crt_deformer* h, int slot, const T** arg, const void* src, size_t bytes) {
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, std::max<size_t>(bytes, 16));
    if (e != hipSuccess) return fail(CRT_ERR_NOMEM, std::string("crt_deformer_create: hipMalloc: ") + hipGetErrorString(e));
    h->bufs[slot] = p;
    if (src && bytes) HIPCHK(hipMemcpy(p, src, bytes, hipMemcpyHostToDevice));
    *arg = static_cast<const T*>(p);
    return CRT_OK;
}

// The pose on `st` (the deformer's stream or a scene's, both on the deformer's device, which is current): the palette and the morph
// weights copied from the pinned block, then the kernel between the deformer's two timing events
int enqueue_pose(crt_deformer* d, const float* bones, const float* morph_weights, hipStream_t st) {
    // the previous pose's copy has left h_pose: long since, unless unsynchronised poses queue up, which therefore run one ahead of the device
    HIPCHK(hipEventSynchronize(d->ev_copy));
    const size_t nb = 12 * (size_t)d->args.n_bones;
    std::memcpy(d->h_pose, bones, nb * sizeof(float));
    if (morph_weights) std::memcpy(d->h_pose + nb, morph_weights, d->n_targets * sizeof(float));
    else std::memset(d->h_pose + nb, 0, d->n_targets * sizeof(float));
    HIPCHK(hipMemcpyAsync(d->d_pose, d->h_pose, d->pose_floats * sizeof(float), hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(d->ev_copy, st));
    HIPCHK(hipEventRecord(d->ev_a, st));
    crt::launch_deform(d->args, d->form, st);
    if (hipGetLastError() != hipSuccess) return fail(CRT_ERR_HIP, "crt_deformer_pose: the launch failed");
    HIPCHK(hipEventRecord(d->ev_b, st));
    d->posed = true;
    d->times_pending = true;
    return CRT_OK;
}

int create_impl(const crt_deformer_desc* desc, crt_deformer** out) {
    const std::string who = "crt_deformer_create: ";
    if (!out) return fail(CRT_ERR_INVALID, who + "null out");
    *out = nullptr;
    size_t E = 0;
    int rc = check_desc(desc, who, &E);
    if (rc) return rc;
    if ((rc = crt::require_device())) return rc;
    int n_dev = 0;
    HIPCHK(hipGetDeviceCount(&n_dev));
    if (desc->device < 0 || desc->device >= n_dev) return fail(CRT_ERR_INVALID, who + "no such device");
    MorphLists lists;
    morph_lists(desc, E, &lists);

    HIPCHK(hipSetDevice(desc->device));
    std::unique_ptr<crt_deformer> owner(new (std::nothrow) crt_deformer);
    crt_deformer* h = owner.get();
    if (!h) return fail(CRT_ERR_NOMEM, who + "out of memory");
    h->device = desc->device;
    h->n_targets = desc->n_targets;
    crt::DeformArgs& a = h->args;
    const size_t nv = desc->n_vertices, nn = desc->n_normals;
    a.n_vertices = (uint32_t)nv; a.n_normals = (uint32_t)nn; a.n_bones = desc->n_bones;
    if ((rc = upload(h, 0, &a.rest_v, desc->rest_vertices, 12 * nv)) || (rc = upload(h, 1, &a.bones_v, desc->vertex_bones, 8 * nv)) ||
        (rc = upload(h, 2, &a.weights_v, desc->vertex_weights, 16 * nv)))
        return rc;
    if (E && ((rc = upload(h, 3, &a.morph_first, lists.first.data(), 4 * (nv + 1))) || (rc = upload(h, 4, &a.morph, lists.entry.data(), 16 * E)))) return rc;
    if (nn && ((rc = upload(h, 5, &a.rest_n, desc->rest_normals, 12 * nn)) || (rc = upload(h, 6, &a.bones_n, desc->normal_bones, 8 * nn)) ||
               (rc = upload(h, 7, &a.weights_n, desc->normal_weights, 16 * nn))))
        return rc;
    const float* o = nullptr;
    if ((rc = upload(h, 8, &o, nullptr, 12 * nv))) return rc;
    a.out_v = const_cast<float*>(o);
    if (nn) {
        if ((rc = upload(h, 9, &o, nullptr, 12 * nn))) return rc;
        a.out_n = const_cast<float*>(o);
    }
    h->pose_floats = 12 * (size_t)desc->n_bones + desc->n_targets;
    if ((rc = dev_alloc(&h->d_pose, h->pose_floats))) return rc;
    HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&h->h_pose), h->pose_floats * sizeof(float)));
    a.palette = reinterpret_cast<const float4*>(h->d_pose);
    a.morph_weights = h->d_pose + 12 * (size_t)desc->n_bones;
    HIPCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&h->ev_copy, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&h->ev_reader, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&h->ev_own, hipEventDisableTiming));
    HIPCHK(hipEventCreate(&h->ev_a));
    HIPCHK(hipEventCreate(&h->ev_b));
    HIPCHK(hipEventRecord(h->ev_copy, h->stream));
    // CRT_DEFORM_PALETTE=global|lds: the probe's and the tests' way to hold one form against the other
    h->form = desc->n_bones <= crt::kDeformLdsBones ? crt::kDeformPaletteLds : crt::kDeformPaletteGlobal;
    if (const char* f = std::getenv("CRT_DEFORM_PALETTE")) {
        if (!std::strcmp(f, "global")) h->form = crt::kDeformPaletteGlobal;
        else if (std::strcmp(f, "lds")) return fail(CRT_ERR_INVALID, who + "CRT_DEFORM_PALETTE is neither global nor lds");
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    *out = owner.release();
    return CRT_OK;
}

int host_impl(const crt_deformer_desc* desc, const float* bones, const float* morph_weights, float* out_vertices, float* out_normals) {
    const std::string who = "crt_deform_host: ";
    size_t E = 0;
    int rc = check_desc(desc, who, &E);
    if (rc) return rc;
    if (!out_vertices) return fail(CRT_ERR_INVALID, who + "null out_vertices");
    if ((rc = check_pose(desc->n_bones, desc->n_targets, bones, morph_weights, who))) return rc;
    MorphLists lists;
    morph_lists(desc, E, &lists);
    float M[12];
    for (size_t v = 0; v < desc->n_vertices; ++v) {
        float p[3] = {desc->rest_vertices[3 * v], desc->rest_vertices[3 * v + 1], desc->rest_vertices[3 * v + 2]};
        if (E)
            for (uint32_t e = lists.first[v]; e < lists.first[v + 1]; ++e)
                crt::dm::morph_add(p, morph_weights ? morph_weights[lists.entry[e].target] : 0.0f, lists.entry[e].d);
        blend_host(desc->vertex_bones + 4 * v, desc->vertex_weights + 4 * v, bones, M);
        crt::dm::skin_position(M, p, out_vertices + 3 * v);
    }
    if (out_normals)
        for (size_t i = 0; i < desc->n_normals; ++i) {
            blend_host(desc->normal_bones + 4 * i, desc->normal_weights + 4 * i, bones, M);
            crt::dm::skin_normal(M, desc->rest_normals + 3 * i, out_normals + 3 * i);
        }
    return CRT_OK;
}

int scene_impl(crt_scene* s, crt_deformer* d, const float* bones, const float* morph_weights, uint32_t flags, int sync) {
    const std::string who = "crt_deform_scene: ";
    if (!s || !d) return fail(CRT_ERR_INVALID, who + "null argument");
    if (flags & ~(uint32_t)(CRT_DEFORM_REBUILD | CRT_DEFORM_KEEP_NORMALS)) return fail(CRT_ERR_INVALID, who + "unknown flag bits");
    if (s->inst) return fail(CRT_ERR_INVALID, who + "an instanced scene's geometry belongs to its handle: pose, then crt_instances_update_meshes_device");
    if (s->primary) return fail(CRT_ERR_INVALID, who + "not on a replica");
    if (d->device != s->device) return fail(CRT_ERR_INVALID, who + "the deformer lives on another device");
    if (d->args.n_vertices != s->n_vertices) return fail(CRT_ERR_INVALID, who + "the deformer's n_vertices differs from the scene's");
    const bool normals = !(flags & CRT_DEFORM_KEEP_NORMALS) && d->args.n_normals;
    if (normals && d->args.n_normals != s->n_normals) return fail(CRT_ERR_INVALID, who + "the deformer's n_normals differs from the scene's");
    int rc = check_pose(d->args.n_bones, d->n_targets, bones, morph_weights, who);
    if (rc) return rc;
    HIPCHK(hipSetDevice(s->device));
    // behind whatever the deformer's own stream, or another scene's, still does with the outputs
    if (d->reader_pending) HIPCHK(hipStreamWaitEvent(s->stream, d->ev_reader, 0));
    HIPCHK(hipEventRecord(d->ev_own, d->stream));
    HIPCHK(hipStreamWaitEvent(s->stream, d->ev_own, 0));
    if ((rc = enqueue_pose(d, bones, morph_weights, s->stream))) return rc;
    rc = crt::scene_take_device_geometry(s, d->args.out_v, d->args.n_vertices, normals ? d->args.out_n : nullptr, normals ? d->args.n_normals : 0,
                                         (flags & CRT_DEFORM_REBUILD) != 0, sync, "crt_deform_scene: ");
    // the deformer's next pose waits until the scene's stream has read these outputs, whether the scene took them or refused
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipEventRecord(d->ev_reader, s->stream));
    d->reader_pending = true;
    return rc;
}

}  // namespace

extern "C" {

int crt_deformer_create(const crt_deformer_desc* desc, crt_deformer** out) {
    try {
        return create_impl(desc, out);
    } catch (const std::exception& e) {
        return fail(CRT_ERR_NOMEM, std::string("crt_deformer_create: ") + e.what());
    }
}

int crt_deformer_destroy(crt_deformer* d) {
    if (!d) return CRT_OK;
    HIPCHK(hipSetDevice(d->device));
    (void)hipStreamSynchronize(d->stream);
    if (d->reader_pending) (void)hipEventSynchronize(d->ev_reader);
    delete d;
    return CRT_OK;
}

int crt_deformer_pose(crt_deformer* d, const float* bones, const float* morph_weights, int sync) {
    if (!d) return fail(CRT_ERR_INVALID, "crt_deformer_pose: null deformer");
    int rc = check_pose(d->args.n_bones, d->n_targets, bones, morph_weights, "crt_deformer_pose: ");
    if (rc) return rc;
    HIPCHK(hipSetDevice(d->device));
    if (d->reader_pending) {                                       // a crt_deform_scene may still read the outputs on its scene's stream
        HIPCHK(hipStreamWaitEvent(d->stream, d->ev_reader, 0));
        d->reader_pending = false;
    }
    if ((rc = enqueue_pose(d, bones, morph_weights, d->stream))) return rc;
    if (sync) return crt_deformer_sync(d);
    return CRT_OK;
}

int crt_deformer_sync(crt_deformer* d) {
    if (!d) return fail(CRT_ERR_INVALID, "crt_deformer_sync: null deformer");
    HIPCHK(hipSetDevice(d->device));
    HIPCHK(hipStreamSynchronize(d->stream));
    if (d->times_pending) {                                        // a pose enqueued on a scene's stream ends with that stream
        HIPCHK(hipEventSynchronize(d->ev_b));
        HIPCHK(hipEventElapsedTime(&d->device_ms, d->ev_a, d->ev_b));
        d->times_pending = false;
    }
    return CRT_OK;
}

int crt_deformer_vertices_device(crt_deformer* d, const float** d_vertices) {
    if (!d || !d_vertices) return fail(CRT_ERR_INVALID, "crt_deformer_vertices_device: null argument");
    *d_vertices = d->args.out_v;
    return CRT_OK;
}

int crt_deformer_normals_device(crt_deformer* d, const float** d_normals) {
    if (!d || !d_normals) return fail(CRT_ERR_INVALID, "crt_deformer_normals_device: null argument");
    *d_normals = d->args.out_n;
    return CRT_OK;
}

int crt_deformer_read(crt_deformer* d, float* vertices, size_t n_floats_v, float* normals, size_t n_floats_n) {
    if (!d || !vertices) return fail(CRT_ERR_INVALID, "crt_deformer_read: null argument");
    if (!d->posed) return fail(CRT_ERR_INVALID, "crt_deformer_read: no pose yet");
    if (n_floats_v != 3 * (size_t)d->args.n_vertices) return fail(CRT_ERR_INVALID, "crt_deformer_read: n_floats_v is not 3 * n_vertices");
    if (normals && n_floats_n != 3 * (size_t)d->args.n_normals) return fail(CRT_ERR_INVALID, "crt_deformer_read: n_floats_n is not 3 * n_normals");
    int rc = crt_deformer_sync(d);
    if (rc) return rc;
    HIPCHK(hipMemcpy(vertices, d->args.out_v, n_floats_v * sizeof(float), hipMemcpyDeviceToHost));
    if (normals && n_floats_n) HIPCHK(hipMemcpy(normals, d->args.out_n, n_floats_n * sizeof(float), hipMemcpyDeviceToHost));
    return CRT_OK;
}

int crt_deformer_last_ms(crt_deformer* d, float* device_ms) {
    if (!d || !device_ms) return fail(CRT_ERR_INVALID, "crt_deformer_last_ms: null argument");
    if (!d->posed) return fail(CRT_ERR_INVALID, "crt_deformer_last_ms: no pose yet");
    int rc = crt_deformer_sync(d);
    if (rc) return rc;
    *device_ms = d->device_ms;
    return CRT_OK;
}

int crt_deform_scene(crt_scene* s, crt_deformer* d, const float* bones, const float* morph_weights, uint32_t flags, int sync) {
    try {
        return scene_impl(s, d, bones, morph_weights, flags, sync);
    } catch (const std::exception& e) {
        return fail(CRT_ERR_NOMEM, std::string("crt_deform_scene: ") + e.what());
    }
}

int crt_deform_host(const crt_deformer_desc* desc, const float* bones, const float* morph_weights, float* out_vertices, float* out_normals) {
    try {
        return host_impl(desc, bones, morph_weights, out_vertices, out_normals);
    } catch (const std::exception& e) {
        return fail(CRT_ERR_NOMEM, std::string("crt_deform_host: ") + e.what());
    }
}

}  // extern "C"
