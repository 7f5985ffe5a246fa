// Device half of include/crt.h: camera, environment, shard, options, several GPUs, crt_trace, packed read-back, refit / rebuild.
// (Making a scene is crt_create.cpp; everything that enqueues a frame is crt_frames.cpp; the images that leave the library — sum, AOVs,
// denoised, accumulated, their RGBA8 — are crt_outputs.cpp; the scene itself crt_scene.hpp.)
// Replaces Scene::gpu_data / update (Caitlyn/Scene.h:1000-1246).  A scene owns its own HIP stream.
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <thread>
#include <new>
#include <string>
#include <vector>

#include "../../include/crt.h"
#include "crt_error.hpp"
#include "crt_scene.hpp"
#include "denoise.hpp"
#include "device_build.hpp"
#include "host/cwbvh.hpp"
#include "host/flatnode_link.hpp"
#include "host/refit_core.hpp"
#include "instances.hpp"
#include "instances_bind.hpp"
#include "rt_kernels.hpp"

using crt::alloc_frame_buffers;
using crt::deal_tiles;
using crt::dev_alloc;
using crt::ensure_frame;
using crt::ensure_planes;
using crt::fail;
using crt::frame_args;
using crt::require_device;

namespace {

uint32_t morton2(uint32_t x, uint32_t y) {
    auto spread = [](uint32_t v) {
        v &= 0xffffu;
        v = (v | (v << 8)) & 0x00ff00ffu;
        v = (v | (v << 4)) & 0x0f0f0f0fu;
        v = (v | (v << 2)) & 0x33333333u;
        v = (v | (v << 1)) & 0x55555555u;
        return v;
    };
    return spread(x) | (spread(y) << 1);
}

}  // namespace

// The tiles of shard `rank` of `world`: the frame's tile x tile squares in Morton order, every world-th one starting at the rank-th
// (SURVEY 8e).  Pure host arithmetic: crt_set_shard, crt_set_devices, option "streams" and the [host] entry crt_shard_tiles share it.
void crt::deal_tiles(uint32_t width, uint32_t height, uint32_t T, uint32_t rank, uint32_t world, std::vector<uint2>& tiles, uint64_t* pixels_in_frame) {
    const uint32_t tx_n = (width + T - 1) / T, ty_n = (height + T - 1) / T;
    struct Item { uint32_t code, x, y; };
    std::vector<Item> all;
    all.reserve((size_t)tx_n * ty_n);
    for (uint32_t y = 0; y < ty_n; ++y)
        for (uint32_t x = 0; x < tx_n; ++x) all.push_back({morton2(x, y), x, y});
    std::sort(all.begin(), all.end(), [](const Item& a, const Item& b) { return a.code < b.code; });
    tiles.clear();
    uint64_t in_frame = 0;
    for (size_t k = rank; k < all.size(); k += world) {
        tiles.push_back(make_uint2(all[k].x, all[k].y));
        const uint32_t w = std::min(T, width - all[k].x * T), h = std::min(T, height - all[k].y * T);
        in_frame += (uint64_t)w * h;
    }
    if (pixels_in_frame) *pixels_in_frame = in_frame;
}

crt::FrameArgs crt::frame_args(const crt_scene* s, float rx, float ry) {
    crt::FrameArgs f{};
    f.tile_xy = s->d_tile_xy;
    f.tile_order = s->d_tile_order;
    f.n_local_pixels = s->n_local_pixels;
    f.tile = s->tile; f.width = s->width; f.height = s->height;
    f.tile_log2 = (s->tile & (s->tile - 1u)) == 0u ? (uint32_t)__builtin_ctz(s->tile) : 0u;
    f.jitter = s->jitter;
    f.rv = rx * ry;
    const float W = (float)s->width, H = (float)s->height;
    f.tan_fov = std::tan(s->cam.fov * 0.5f);
    f.aspect_tan = W / H * f.tan_fov;
    for (int k = 0; k < 3; ++k) {
        f.cam_pos[k] = s->cam.position[k]; f.cam_right[k] = s->cam.right[k];
        f.cam_up[k] = s->cam.up[k]; f.cam_forward[k] = s->cam.forward[k];
    }
    return f;
}

// Logical device k of n_devices, dividing shard base_rank of base_world among themselves (set_devices_of_shard): every n-th tile of that
// shard's list starting at its k-th, i.e. shard base_rank + k * base_world of base_world * n_devices of the whole frame.
static inline void device_share(uint32_t k, uint32_t n_devices, uint32_t base_rank, uint32_t base_world, uint32_t* rank, uint32_t* world) {
    *rank = base_rank + k * base_world;
    *world = base_world * n_devices;
}

// The nodes' child planes as floats (uniform node steps, rt_kernels.hip node8_intersect_planes): 192 B per node, 2.4 x the node array — built
// when a frame first walks the CWBVH, so a scene that only ever renders through its BVH2 (option accel 1 / 2) or only serves crt_trace never
// holds them.  In stream order before the frame's kernels: no host wait.  A replica made later gets its copy with the other scene buffers.
int crt::ensure_planes(crt_scene* s) {                    // crt_frames.cpp calls it too (crt_scene.hpp)
    if (s->d_planes || !s->d_nodes || !s->info.n_nodes8) return CRT_OK;
    int rc;
    s->shared_bytes[kSharedPlanes] = (size_t)s->info.n_nodes8 * 12 * sizeof(float4);
    if (s->primary && s->shares_scene) {
        // a replica on its primary's own device that was made before any CWBVH frame (the scene rendered through its BVH2 until now): it borrows
        // the primary's planes like every other scene buffer.  Rare path: one host wait for the primary's stream.
        crt_scene* const p = s->primary;
        if ((rc = ensure_planes(p))) return rc;
        HIPCHK(hipStreamSynchronize(p->stream));
        s->d_planes = p->d_planes;               // borrowed: the destructor lets go of it
        return CRT_OK;
    }
    if ((rc = dev_alloc(&s->d_planes, (size_t)s->info.n_nodes8 * 12))) return rc;
    crt::launch_expand_planes(s->d_nodes, (uint32_t)CRT_NODE_ROWS, s->d_planes, s->info.n_nodes8, s->stream);
    if (hipGetLastError() != hipSuccess) return fail(CRT_ERR_HIP, "plane expansion failed");
    return CRT_OK;
}

extern "C" {

int crt_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// HIP loads a code object when one of its kernels is first looked up.  The library has four (traversal kernels; the GPU builders
// with their sort / scan kernels; the CWBVH converter; scene assembly), and the builders' alone costs 12.5 ms on MI355X — more than the
// whole build of a million triangles it then runs (profiles/r04_build_probe.txt: the first crt_scene_create(... CRT_BUILD_SAH) of a
// process that had already rendered took 22.2 ms, every later one 8.4).  So the first scene a process creates on a device starts a
// thread that loads all four while the caller uploads and renders; a build-on-device creation waits for it instead of loading
// the same code objects itself.  crt_warmup() does the same synchronously.
namespace {
struct Warmer {
    std::mutex m;
    std::thread t;
    std::vector<int> started;                      // HIP devices whose code objects are loaded or loading
    std::atomic<int> rc{0};                        // first failure of a background load (crt_warmup reports it; a first use then loads again and fails loudly itself)
    static int load_all() {
        int e;
        if ((e = crt::warm_rt_kernels()) || (e = crt::warm_lbvh_kernels()) || (e = crt::warm_cwbvh_kernels()) || (e = crt::warm_scene_build_kernels()) ||
            (e = crt::warm_instance_kernels()) || (e = crt::warm_denoise_kernels()) || (e = crt::warm_temporal_kernels())) return e;
        return 0;
    }
    void start(int device) {                       // returns at once
        std::lock_guard<std::mutex> g(m);
        if (device < 0 || std::find(started.begin(), started.end(), device) != started.end()) return;
        if (t.joinable()) t.join();
        try {
            started.push_back(device);
            t = std::thread([this, device] {
                int e = (int)hipSetDevice(device);
                if (!e) e = load_all();
                int none = 0;
                if (e) rc.compare_exchange_strong(none, e);
            });
        } catch (const std::exception&) { /* no thread: the code objects load at first use, as before */ }
    }
    int wait() {                                   // joins the background load; its result (0 = fine)
        std::lock_guard<std::mutex> g(m);
        if (t.joinable()) t.join();
        return rc.load();
    }
    ~Warmer() { if (t.joinable()) t.join(); }
};
Warmer g_warmer;
}  // namespace

// crt_create.cpp's way to it: the first scene a process creates on a device starts the load, a build on the device waits for it
extern "C++" void crt::warm_start(int device) { g_warmer.start(device); }
extern "C++" int crt::warm_wait() { return g_warmer.wait(); }

// Optional, synchronous: the HIP context of the current device, the library's code objects, and the runtime's own first-use set-up
// (first stream, first host-to-device copy, first event, first kernel dispatch: ~85 ms in a fresh process, profiles/r04_build_probe.txt)
// — what the first crt_scene_create of a process otherwise pays.
int crt_warmup(void) {
    int rc = require_device();
    if (rc) return rc;
    HIPCHK(hipFree(nullptr));                          // creates the context
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    const int bg = g_warmer.wait();
    if (bg) return fail(CRT_ERR_HIP, std::string("crt_warmup: a background load of a code object had failed: ") + hipGetErrorString((hipError_t)bg));
    const int e = Warmer::load_all();
    if (e) return fail(CRT_ERR_HIP, std::string("crt_warmup: loading a code object failed: ") + hipGetErrorString((hipError_t)e));
    hipStream_t st = nullptr;
    hipEvent_t ev = nullptr;
    uint4* d = nullptr;
    std::vector<uint4> h(4096, make_uint4(1u, 2u, 3u, 4u));           // 64 KB: through the pageable-copy staging path
    auto done = [&](int code) { if (ev) (void)hipEventDestroy(ev); if (d) (void)hipFree(d); if (st) (void)hipStreamDestroy(st); return code; };
#define W_CHK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return done(fail(CRT_ERR_HIP, std::string("crt_warmup: " #expr ": ") + hipGetErrorString(e_))); } while (0)
    W_CHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    W_CHK(hipEventCreate(&ev));
    W_CHK(hipMalloc(reinterpret_cast<void**>(&d), 2 * h.size() * sizeof(uint4)));
    W_CHK(hipMemcpyAsync(d, h.data(), h.size() * sizeof(uint4), hipMemcpyHostToDevice, st));
    W_CHK(hipMemsetAsync(d + h.size(), 0, h.size() * sizeof(uint4), st));
    crt::launch_restride(d, 1u, d + h.size(), 1u, h.size(), st);       // one dispatch of a library kernel
    W_CHK(hipEventRecord(ev, st));
    W_CHK(hipMemcpyAsync(h.data(), d + h.size(), 64, hipMemcpyDeviceToHost, st));
    W_CHK(hipStreamSynchronize(st));
    W_CHK(hipGetLastError());
#undef W_CHK
    return done(CRT_OK);
}

int crt_has_experiments(void) {
#ifdef CRT_EXPERIMENTS
    return 1;
#else
    return 0;
#endif
}

// The world light table of a scene with mesh lights, if the handle has changed since it was built (or crt_scene_set_mesh_lights marked
// it): counts and scan, ONE small read for the total (the host's wait: everything queued on the stream before is then done, so a table
// that has to grow can be freed), then transform, tree sum and pdf column on the scene's stream.  The mutators of the handle return done
// and wait for this stream first, so the live arrays are complete and nothing in flight reads the table.
extern "C++" int crt::ensure_light_table(crt_scene* s) {      // crt_frames.cpp calls it too (crt_scene.hpp)
    SceneLights* L = s->lit;
    if (!L) return CRT_OK;
    crt::InstancesView v{};
    crt::instances_view(s->inst, &v);
    if (!L->stale && L->seen == v.mutations) return CRT_OK;
    HIPCHK(hipSetDevice(s->device));
    crt::LightTableArgs a{};
    a.mesh_of = v.mesh_of; a.o2w = v.o2w; a.w2o = v.w2o; a.mesh_lights = L->d_mesh; a.obj_lights = L->d_obj; a.static_lights = L->d_static;
    a.n_instances = v.n_instances; a.n_meshes = v.n_meshes; a.n_static = L->n_static;
    a.first = L->d_first; a.block_sums = L->d_block_sums; a.total = L->d_total;
    crt::launch_light_scan(a, s->stream);
    uint32_t total = 0;
    HIPCHK(hipMemcpyAsync(&total, L->d_total, 4, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    HIPCHK(hipGetLastError());
    const uint64_t n_total = (uint64_t)L->n_static + total;
    if (n_total >= (1ull << 31)) return fail(CRT_ERR_LIMIT, "the world light table exceeds 2^31 lights");
    if (n_total > L->table_cap || !L->d_partial) {
        const size_t cap = std::max<size_t>(n_total + n_total / 2, 64);
        float* table = nullptr; float* partial = nullptr;
        int rc;
        if ((rc = dev_alloc(&table, cap * 18))) return rc;
        if ((rc = dev_alloc(&partial, 2 * ((cap + 255) / 256)))) { (void)hipFree(table); return rc; }
        if (s->d_lights) (void)hipFree(s->d_lights);
        if (L->d_partial) (void)hipFree(L->d_partial);
        s->d_lights = table; L->d_partial = partial; L->table_cap = cap;
    }
    a.table = s->d_lights; a.partial = L->d_partial; a.n_total = (uint32_t)n_total;
    crt::launch_light_table(a, s->stream);
    HIPCHK(hipGetLastError());
    s->n_lights = (uint32_t)n_total;
    L->seen = v.mutations; L->stale = false;
    return CRT_OK;
}

int crt_scene_set_mesh_lights(crt_scene* s, uint32_t mesh, const crt_light* lights, size_t n_lights) {
    const std::string who = "crt_scene_set_mesh_lights: ";
    if (!s) return fail(CRT_ERR_INVALID, who + "null scene");
    if (!s->inst || !s->lit) return fail(CRT_ERR_INVALID, who + "the scene has no mesh lights (crt_scene_create_instanced_lit)");
    SceneLights* L = s->lit;
    if (mesh >= L->mesh.size()) return fail(CRT_ERR_INVALID, who + "mesh index out of range");
    if (n_lights != L->mesh[mesh].y) return fail(CRT_ERR_INVALID, who + "n_lights differs from the count given at create");
    if (n_lights && !lights) return fail(CRT_ERR_INVALID, who + "null lights");
    for (size_t i = 0; i < n_lights; ++i)
        if (!crt::light_finite(lights[i])) return fail(CRT_ERR_INVALID, who + "a field of light " + std::to_string(i) + " is not finite");
    if (n_lights == 0) return CRT_OK;
    HIPCHK(hipSetDevice(s->device));
    std::copy(lights, lights + n_lights, L->obj.begin() + L->mesh[mesh].x);
    // behind whatever the stream holds (frames that read the table built from the old lights), from the scene's own copy
    HIPCHK(hipMemcpyAsync(L->d_obj + 18 * (size_t)L->mesh[mesh].x, L->obj.data() + L->mesh[mesh].x, n_lights * sizeof(crt_light), hipMemcpyHostToDevice, s->stream));
    L->stale = true;
    return CRT_OK;
}

int crt_scene_read_lights(crt_scene* s, crt_light* dst, size_t cap, size_t* n_out) {
    const std::string who = "crt_scene_read_lights: ";
    if (!s) return fail(CRT_ERR_INVALID, who + "null scene");
    if (!s->inst) return fail(CRT_ERR_INVALID, who + "not an instanced scene");
    try {
        const int rc = crt::ensure_light_table(s);
        if (rc) return rc;
    } catch (const std::exception& e) {
        return fail(CRT_ERR_NOMEM, who + e.what());
    }
    if (n_out) *n_out = s->n_lights;
    if (!dst) return CRT_OK;
    if (cap < s->n_lights) return fail(CRT_ERR_INVALID, who + "destination too small");
    if (s->n_lights == 0) return CRT_OK;
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipStreamSynchronize(s->stream));
    HIPCHK(hipMemcpy(dst, s->d_lights, (size_t)s->n_lights * sizeof(crt_light), hipMemcpyDeviceToHost));
    return CRT_OK;
}

int crt_set_camera(crt_scene* s, const crt_camera* cam) {
    if (!s || !cam) return fail(CRT_ERR_INVALID, "crt_set_camera: null argument");
    // the thin lens (include/crt.h at crt_camera): checked before anything is stored, so that a refused call leaves this scene and every
    // peer with the camera they had
    if (!(cam->aperture >= 0.0f) || std::isinf(cam->aperture)) return fail(CRT_ERR_INVALID, "crt_set_camera: aperture must be finite and >= 0");
    if (cam->aperture > 0.0f && !(cam->focal_dist > 0.0f && std::isfinite(cam->focal_dist)))
        return fail(CRT_ERR_INVALID, "crt_set_camera: focal_dist must be finite and > 0 when aperture > 0");
    if (!s->have_camera || std::memcmp(&s->cam, cam, sizeof *cam) != 0) s->tile_state = crt_scene::TILES_WANT;   // a new view: new tile costs
    s->cam = *cam;
    s->have_camera = true;
    for (crt_scene* p : s->peers) { const int rc = crt_set_camera(p, cam); if (rc) return rc; }
    return CRT_OK;
}

// The environment (include/crt.h).  Everything is checked, and every device's copy of the map allocated and filled, before
// any device's state changes: a refused or failed call leaves the scene and its peers with the environment they had.
int crt_set_environment(crt_scene* s, const crt_environment* env) {
    if (!s) return fail(CRT_ERR_INVALID, "crt_set_environment: null scene");
    if (s->primary) return fail(CRT_ERR_INVALID, "crt_set_environment: not on a replica");
    std::vector<crt_scene*> all;
    std::vector<float4> texels;
    std::vector<float4*> fresh;
    size_t n = 0;
    try {
        all.push_back(s);
        all.insert(all.end(), s->peers.begin(), s->peers.end());
        if (env) {
            if (!env->texels) return fail(CRT_ERR_INVALID, "crt_set_environment: texels is null");
            if (env->size < 1u || env->size > 4096u) return fail(CRT_ERR_INVALID, "crt_set_environment: size must be 1..4096");
            if (env->flags & ~CRT_ENV_HIDE_FROM_CAMERA) return fail(CRT_ERR_INVALID, "crt_set_environment: unknown flags bits");
            if (env->reserved[0] != 0u || env->reserved[1] != 0u) return fail(CRT_ERR_INVALID, "crt_set_environment: reserved must be 0");
            for (int k = 0; k < 9; ++k)
                if (!std::isfinite(env->rotation[k])) return fail(CRT_ERR_INVALID, "crt_set_environment: rotation has an entry that is not finite");
            for (int k = 0; k < 3; ++k)
                if (!std::isfinite(env->scale[k]) || env->scale[k] < 0.0f) return fail(CRT_ERR_INVALID, "crt_set_environment: scale must be finite and >= 0");
            if (s->accel != 0u) return fail(CRT_ERR_INVALID, "crt_set_environment: the BVH2 frame mode (option accel) has no environment");
            n = (size_t)env->size * env->size;
            texels.resize(n);
            for (size_t i = 0; i < n; ++i) {
                const float r = env->texels[3 * i], g = env->texels[3 * i + 1], b = env->texels[3 * i + 2];
                if (!std::isfinite(r) || !std::isfinite(g) || !std::isfinite(b) || r < 0.0f || g < 0.0f || b < 0.0f)
                    return fail(CRT_ERR_INVALID, "crt_set_environment: texels must be finite and >= 0");
                texels[i] = make_float4(r, g, b, 0.0f);
            }
            fresh.assign(all.size(), nullptr);
        }
    } catch (const std::exception&) {
        return fail(CRT_ERR_NOMEM, "crt_set_environment: out of host memory");
    }
    int rc = CRT_OK;
    for (size_t k = 0; env && k < all.size() && !rc; ++k) {
        if (hipSetDevice(all[k]->device) != hipSuccess) { rc = fail(CRT_ERR_HIP, "crt_set_environment: hipSetDevice failed"); break; }
        if ((rc = dev_alloc(&fresh[k], n))) break;
        if (hipMemcpy(fresh[k], texels.data(), n * sizeof(float4), hipMemcpyHostToDevice) != hipSuccess) rc = fail(CRT_ERR_HIP, "crt_set_environment: hipMemcpy H2D failed");
    }
    // frames in flight read the map they were enqueued with: every stream drains before its device's copy is replaced
    for (size_t k = 0; k < all.size() && !rc; ++k)
        if (hipSetDevice(all[k]->device) != hipSuccess || hipStreamSynchronize(all[k]->stream) != hipSuccess) rc = fail(CRT_ERR_HIP, "crt_set_environment: hipStreamSynchronize failed");
    if (rc) {
        for (size_t k = 0; k < fresh.size(); ++k) if (fresh[k]) { (void)hipSetDevice(all[k]->device); (void)hipFree(fresh[k]); }
        (void)hipSetDevice(s->device);
        return rc;
    }
    for (size_t k = 0; k < all.size(); ++k) {
        crt_scene* x = all[k];
        (void)hipSetDevice(x->device);
        if (x->d_env) (void)hipFree(x->d_env);
        x->d_env = env ? fresh[k] : nullptr;
        x->env_size = env ? env->size : 0u; x->env_flags = env ? env->flags : 0u;
        for (int j = 0; j < 9; ++j) x->env_rotation[j] = env ? env->rotation[j] : (j % 4 == 0 ? 1.0f : 0.0f);
        for (int j = 0; j < 3; ++j) x->env_scale[j] = env ? env->scale[j] : 1.0f;
    }
    (void)hipSetDevice(s->device);
    return CRT_OK;
}

static int set_devices_of_shard(crt_scene* s, const int32_t* devices, uint32_t n_devices, uint32_t tile, uint32_t base_rank, uint32_t base_world);

int crt_set_shard(crt_scene* s, uint32_t rank, uint32_t world, uint32_t tile) {
    if (!s) return fail(CRT_ERR_INVALID, "crt_set_shard: null scene");
    if (world == 0 || rank >= world) return fail(CRT_ERR_INVALID, "crt_set_shard: rank/world");
    if (tile < 8 || (tile & 7u) || tile > 1024) return fail(CRT_ERR_INVALID, "crt_set_shard: tile must be a multiple of 8 in 8..1024");
    if (s->streams > 1u) {                   // the caller shards the frame itself now: its shard runs on one stream
        const int32_t one = s->device;
        const int rc = crt_set_devices(s, &one, 1, tile);
        if (rc) return rc;
    }
    if (!s->peers.empty() || s->primary) return fail(CRT_ERR_INVALID, "crt_set_shard: this scene deals its tiles to its own devices (crt_set_devices)");
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipStreamSynchronize(s->stream));
    s->rank = rank; s->world = world; s->tile = tile;
    s->shard_rank = rank; s->shard_world = world;
    return alloc_frame_buffers(s);
}

int crt_reset(crt_scene* s) {
    if (!s) return fail(CRT_ERR_INVALID, "crt_reset: null scene");
    HIPCHK(hipSetDevice(s->device));
    int rc = ensure_frame(s);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(s->d_sum, 0, 3 * (size_t)std::max<uint32_t>(s->n_local_pixels, 1) * sizeof(float), s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    for (crt_scene* p : s->peers) { rc = crt_reset(p); if (rc) break; }
    if (!s->peers.empty()) (void)hipSetDevice(s->device);
    return rc;
}

int crt_set_option(crt_scene* s, const char* name, int value) {
    if (!s || !name) return fail(CRT_ERR_INVALID, "crt_set_option: null argument");
    if (s->inst) {
        // an instanced scene: one stream, the two-level walk, no tile clock
        if (!std::strcmp(name, "streams")) {
            if (value != 0 && value != 1) return fail(CRT_ERR_INVALID, "crt_set_option: an instanced scene renders on one stream (streams is 0 or 1)");
            return CRT_OK;
        }
        if (!std::strcmp(name, "accel") && value != 0)
            return fail(CRT_ERR_INVALID, "crt_set_option: an instanced scene has no BVH2: its frames walk the handle's two-level CWBVH (accel is 0)");
        if (!std::strcmp(name, "adaptive_tiles")) return CRT_OK;      // treated as 0: the per-tile clock lives in the fused first-segment kernel
        // masks in frames: read when the next frame is enqueued
        if (!std::strcmp(name, "instance_masks")) {
            if (value != 0 && value != 1) return fail(CRT_ERR_INVALID, "crt_set_option: instance_masks is 0 or 1");
            s->instance_masks = (uint32_t)value;
            return CRT_OK;
        }
        if (!std::strcmp(name, "mask_primary") || !std::strcmp(name, "mask_bounce") || !std::strcmp(name, "mask_shadow")) {
            if (value < 0 || value > 255) return fail(CRT_ERR_INVALID, std::string("crt_set_option: ") + name + " is a ray mask, 0..255");
            (name[5] == 'p' ? s->mask_primary : name[5] == 'b' ? s->mask_bounce : s->mask_shadow) = (uint32_t)value;
            return CRT_OK;
        }
    }
    if (!std::strcmp(name, "jitter")) s->jitter = value ? 1u : 0u;
    else if (!std::strcmp(name, "count_visits")) { s->count_visits = value != 0; s->count_batched = value == 2; }
    else if (!std::strcmp(name, "bounce_refill")) s->bounce_refill = value ? 1u : 0u;
    else if (!std::strcmp(name, "refill_pool") || !std::strcmp(name, "shadow_pool")) {
        if (value != 64 && value != 128 && value != 256 && value != 512) return fail(CRT_ERR_INVALID, std::string("crt_set_option: ") + name + " is 64, 128, 256 or 512");
        (name[0] == 'r' ? s->refill_pool : s->shadow_pool) = (uint32_t)value;
    }
    else if (!std::strcmp(name, "shadow_refill_min")) s->shadow_refill_min = (uint32_t)std::min(65, std::max(1, value));
    else if (!std::strcmp(name, "shadow_waves")) s->shadow_waves = (uint32_t)std::min(8, std::max(1, value));
    else if (!std::strcmp(name, "step_hist_mode")) s->step_hist_mode = value ? 1u : 0u;
    else if (!std::strcmp(name, "persistent")) s->persistent = value ? 1u : 0u;
    else if (!std::strcmp(name, "sort_shadow")) s->sort_shadow = value ? 1u : 0u;
#ifdef CRT_EXPERIMENTS
    else if (!std::strcmp(name, "trace_occupancy")) s->trace_occupancy = (uint32_t)std::max(1, value);
    else if (!std::strcmp(name, "oversubscribe")) s->oversubscribe = (uint32_t)std::max(0, value);
    else if (!std::strcmp(name, "waves_per_workgroup")) {
        if (value != 1 && value != 2 && value != 4) return fail(CRT_ERR_INVALID, "crt_set_option: waves_per_workgroup is 1, 2 or 4");
        s->waves_per_workgroup = (uint32_t)value;
    }
#else
    // persistent grids and multi-wave workgroups live in the CRT_EXPERIMENTS build only (make EXPERIMENTS=1); their default values are accepted
    else if (!std::strcmp(name, "trace_occupancy") || !std::strcmp(name, "oversubscribe") || !std::strcmp(name, "waves_per_workgroup")) {
        const bool is_default = !std::strcmp(name, "waves_per_workgroup") ? value == 1 : !std::strcmp(name, "oversubscribe") ? value == 0 : true;
        if (!is_default) return fail(CRT_ERR_INVALID, std::string("crt_set_option: ") + name + " is an experimental variant: this library was built without CRT_EXPERIMENTS");
    }
#endif
    else if (!std::strcmp(name, "streams")) {
        // k tile shards of the frame, each with its own stream, queues and path state, on this one GPU: the segment launches of one
        // shard fill the tails and gaps of the others' (a multi-segment frame is a chain of dependent launches).  The machinery is
        // crt_set_devices' with the same GPU listed k times; the scene buffers are shared, not copied.
        if (value < 0 || value > 4) return fail(CRT_ERR_INVALID, "crt_set_option: streams is 0 (pick for me) or 1..4");
        // 0: what the measurements say — a frame of a few-node scene is bound by the gaps between its launches (3 streams), a multi-segment
        // frame by the tails of its chain of launches (2), a one-segment frame of a large scene by neither (1)
        if (value == 0) value = s->info.n_nodes8 < 64 ? 3 : s->max_depth > 1 ? 2 : 1;
        if (s->primary) return fail(CRT_ERR_INVALID, "crt_set_option: streams is set on the scene, not on a replica");
        if ((uint32_t)value == s->streams) return CRT_OK;
        if (s->streams == 1u && !s->peers.empty())
            return fail(CRT_ERR_INVALID, "crt_set_option: streams is for a scene on one device (crt_set_devices already deals its tiles to several)");
        const std::vector<int32_t> ids((size_t)value, (int32_t)s->device);
        const int rc = set_devices_of_shard(s, ids.data(), (uint32_t)value, s->tile ? s->tile : 16u, s->shard_rank, s->shard_world);
        if (rc) return rc;
        s->streams = (uint32_t)value;
        return CRT_OK;                       // nothing to pass on to the replicas
    }
    else if (!std::strcmp(name, "wave_samples")) s->wave_samples = value < 0 ? 0u : std::min<uint32_t>(3u, (uint32_t)value);
    else if (!std::strcmp(name, "wide_first")) s->wide_first = value < 0 ? 0u : std::min<uint32_t>(2u, (uint32_t)value);
    else if (!std::strcmp(name, "lanes_per_ray")) {
        if (value != 1 && value != 8) return fail(CRT_ERR_INVALID, "crt_set_option: lanes_per_ray is 1 or 8");
        s->lanes_per_ray = (uint32_t)value;
    }
    else if (!std::strcmp(name, "inplace_shadow")) {
        if (value < 0 || value > 3) return fail(CRT_ERR_INVALID, "crt_set_option: inplace_shadow is 1 (in place), 0 (every segment's shadow rays deferred), 2 (bounce segments' deferred) or 3 (pick for me)");
        s->inplace_shadow = (uint32_t)value;
    }
    else if (!std::strcmp(name, "adaptive_tiles")) { s->adaptive_tiles = value ? 1u : 0u; if (value) s->tile_state = crt_scene::TILES_WANT; }
    else if (!std::strcmp(name, "accel")) {
        if (value < 0 || value > 2) return fail(CRT_ERR_INVALID, "crt_set_option: accel is 0 (CWBVH), 1 (BVH2, reference order) or 2 (BVH2, lowest-id ties)");
        if (value != 0 && !s->d_bvh2) return fail(CRT_ERR_INVALID, "crt_set_option: the scene was created without a BVH2 (desc.bvh)");
        if (value != 0 && s->env()) return fail(CRT_ERR_INVALID, "crt_set_option: accel stays 0 while an environment is set (crt_set_environment): the BVH2 frame mode has none");
        if (value != 0 && s->special_materials)
            return fail(CRT_ERR_INVALID, "crt_set_option: the BVH2 frame mode is the shipped shader, which is Lambert only; this scene has Mirror / Disney materials");
        s->accel = (uint32_t)value;
    }
    else if (!std::strcmp(name, "timing")) s->timing = (uint32_t)std::max(0, value);
    else if (!std::strcmp(name, "timing_accumulate")) {
        HIPCHK(hipSetDevice(s->device));
        HIPCHK(hipStreamSynchronize(s->stream));
        s->timing_accumulate = value != 0;
        s->n_spans = 0;
        const size_t want = value > 0 ? (size_t)std::min(value, 1 << 14) : 0;   // value = launches to make room for
        try { if (s->spans.size() < want) s->spans.resize(want); } catch (const std::exception&) { return fail(CRT_ERR_NOMEM, "crt_set_option: out of host memory (timing spans)"); }
    }
    else if (!std::strcmp(name, "ray_bins")) s->ray_bins = (uint32_t)std::min(5, std::max(0, value));
    else if (!std::strcmp(name, "last_build")) s->last_build = value ? 1u : 0u;
    else if (!std::strcmp(name, "lean_build")) s->lean_build = value ? 1u : 0u;
    else if (!std::strcmp(name, "denoise_form")) {
        if (value < 0 || value > 2) return fail(CRT_ERR_INVALID, "crt_set_option: denoise_form is 0 (per tap spacing), 1 (staged) or 2 (direct)");
        s->denoise_form = (uint32_t)value;
    }
    else if (!std::strcmp(name, "temporal_form")) {
        if (value < 0 || value > 2) return fail(CRT_ERR_INVALID, "crt_set_option: temporal_form is 0 (as measured), 1 (staged) or 2 (direct)");
        s->temporal_form = (uint32_t)value;
    }
    else if (!std::strcmp(name, "debug_fail_batch_alloc")) {
        // one injected failure, on ONE device: 1 = this scene's own, k >= 2 = its (k - 1)-th peer (streams / crt_set_devices); 0 disarms all
        if (value >= 2 && (size_t)(value - 2) < s->peers.size()) s->peers[(size_t)(value - 2)]->debug_fail_batch_alloc = 1u;
        else s->debug_fail_batch_alloc = value == 1 ? 1u : 0u;
        if (value == 0) for (crt_scene* p : s->peers) p->debug_fail_batch_alloc = 0u;
        return CRT_OK;
    }
    else if (!std::strcmp(name, "tri_min")) s->tri_min = (uint32_t)std::min(64, std::max(0, value));   // 0: plain per-lane closest-hit loop (what trees of a few nodes get)
    else if (!std::strcmp(name, "refill_min")) s->refill_min = (uint32_t)std::min(65, std::max(1, value));   // 65: never while a lane is busy (lock-step batches)
    else if (!std::strcmp(name, "trace_pool")) {
        if (value != 64 && value != 128 && value != 256) return fail(CRT_ERR_INVALID, "crt_set_option: trace_pool is 64, 128 or 256");
        s->trace_pool = (uint32_t)value;
    }
    else if (!std::strcmp(name, "gather_transport")) {
        if (value != 0 && value != 1) return fail(CRT_ERR_INVALID, "crt_set_option: gather_transport is 0 (RCCL send / recv) or 1 (hipMemcpyPeerAsync)");
        if (value == 0 && !s->peers.empty() && s->rccl_comms.empty())
            return fail(CRT_ERR_INVALID, "crt_set_option: this scene's devices have no RCCL communicators (virtual devices, or librccl.so could not be loaded)");
        s->gather_transport = (uint32_t)value;
        return CRT_OK;
    }
    else return fail(CRT_ERR_INVALID, std::string("crt_set_option: unknown option ") + name);
    for (crt_scene* p : s->peers) { const int rc = crt_set_option(p, name, value); if (rc) { (void)hipSetDevice(s->device); return rc; } }
    if (!s->peers.empty()) (void)hipSetDevice(s->device);      // "timing_accumulate" visits the peers' devices
    return CRT_OK;
}

int crt_get_bvh_info(crt_scene* s, crt_bvh_info* out) {
    if (!s || !out) return fail(CRT_ERR_INVALID, "crt_get_bvh_info: null argument");
    if (s->inst) {                           // the handle's live totals, as crt_instances_get_info reports them
        crt::InstancesView v{};
        crt::instances_view(s->inst, &v);
        s->info.n_nodes8 = (uint64_t)v.tlas_nodes8 + v.blas_nodes8; s->info.n_tris8 = v.blas_tris;
        s->info.max_depth8 = (uint64_t)v.tlas_depth8 + v.max_blas_depth8; s->info.built_on_device = 1;
    }
    *out = s->info;
    return CRT_OK;
}

// Option "streams": the caller's shard lives in k parts, one per stream; tile i of stream j is tile i * k + j of the shard's own list
// (set_devices_of_shard), so the shard's packed buffer is the parts interleaved tile by tile.
static size_t shard_tiles_of_streams(const crt_scene* s) {
    size_t n = s->n_local_tiles;
    for (const crt_scene* p : s->peers) n += p->n_local_tiles;
    return n;
}
static int copy_packed_of_streams(crt_scene* s, void* dst, hipMemcpyKind kind) {
    const size_t tile_bytes = 3 * (size_t)s->tile * s->tile * sizeof(float);
    const size_t k = s->peers.size() + 1;
    for (crt_scene* p : s->peers) HIPCHK(hipStreamSynchronize(p->stream));     // their frames are in their sums before these are read
    for (size_t j = 0; j < k; ++j) {
        const crt_scene* q = j == 0 ? s : s->peers[j - 1];
        if (!q->n_local_tiles) continue;
        HIPCHK(hipMemcpy2DAsync(static_cast<char*>(dst) + j * tile_bytes, k * tile_bytes, q->d_sum, tile_bytes, tile_bytes, q->n_local_tiles, kind, s->stream));
    }
    return CRT_OK;
}

int crt_packed_info(crt_scene* s, uint32_t* n_local_tiles, uint32_t* tile, size_t* n_floats) {
    if (!s) return fail(CRT_ERR_INVALID, "crt_packed_info: null scene");
    HIPCHK(hipSetDevice(s->device));
    int rc = ensure_frame(s);
    if (rc) return rc;
    // option "streams": the caller's shard is what its streams hold together
    const size_t tiles = s->streams > 1u ? shard_tiles_of_streams(s) : s->n_local_tiles;
    if (n_local_tiles) *n_local_tiles = (uint32_t)tiles;
    if (tile) *tile = s->tile;
    if (n_floats) *n_floats = 3 * tiles * s->tile * s->tile;
    return CRT_OK;
}

int crt_read_packed(crt_scene* s, float* dst, size_t n_floats) {
    if (!s || !dst) return fail(CRT_ERR_INVALID, "crt_read_packed: null argument");
    HIPCHK(hipSetDevice(s->device));
    int rc = ensure_frame(s);
    if (rc) return rc;
    if (s->streams > 1u) {
        if (n_floats != 3 * shard_tiles_of_streams(s) * s->tile * s->tile) return fail(CRT_ERR_INVALID, "crt_read_packed: size mismatch");
        if ((rc = copy_packed_of_streams(s, dst, hipMemcpyDeviceToHost))) return rc;
        HIPCHK(hipStreamSynchronize(s->stream));
        return CRT_OK;
    }
    if (n_floats != 3 * (size_t)s->n_local_pixels) return fail(CRT_ERR_INVALID, "crt_read_packed: size mismatch");
    HIPCHK(hipStreamSynchronize(s->stream));
    HIPCHK(hipMemcpy(dst, s->d_sum, n_floats * sizeof(float), hipMemcpyDeviceToHost));
    return CRT_OK;
}

int crt_copy_packed_device(crt_scene* s, void* d_dst, size_t n_floats, int sync) {
    if (!s || !d_dst) return fail(CRT_ERR_INVALID, "crt_copy_packed_device: null argument");
    HIPCHK(hipSetDevice(s->device));
    int rc = ensure_frame(s);
    if (rc) return rc;
    if (s->streams > 1u) {
        if (n_floats != 3 * shard_tiles_of_streams(s) * s->tile * s->tile) return fail(CRT_ERR_INVALID, "crt_copy_packed_device: size mismatch");
        if ((rc = copy_packed_of_streams(s, d_dst, hipMemcpyDeviceToDevice))) return rc;
        if (sync) HIPCHK(hipStreamSynchronize(s->stream));
        return CRT_OK;
    }
    if (n_floats != 3 * (size_t)s->n_local_pixels) return fail(CRT_ERR_INVALID, "crt_copy_packed_device: size mismatch");
    HIPCHK(hipMemcpyAsync(d_dst, s->d_sum, n_floats * sizeof(float), hipMemcpyDeviceToDevice, s->stream));
    if (sync) HIPCHK(hipStreamSynchronize(s->stream));
    return CRT_OK;
}

// ------------------------------------------------------------------ several GPUs, one handle ----

namespace {

// The slice of RCCL this file uses, resolved from librccl.so at crt_set_devices time: the library is a dependency only of scenes
// that span several GPUs (and a process that already carries an RCCL — PyTorch ships its own — keeps exactly that one).
struct Rccl {
    typedef int (*InitAll)(void**, int, const int*);
    typedef int (*Destroy)(void*);
    typedef int (*Group)(void);
    typedef int (*SendRecv)(void*, size_t, int, int, void*, hipStream_t);      // ncclSend's buffer is const void*: same ABI
    typedef const char* (*ErrStr)(int);
    InitAll init_all = nullptr; Destroy destroy = nullptr; Group group_start = nullptr, group_end = nullptr;
    SendRecv send = nullptr, recv = nullptr; ErrStr err = nullptr;
    bool loaded = false;                // every symbol below resolved: set last, so a partial resolve can never be taken for a loaded library
    bool load(void** lib) {
        if (loaded) return true;
        void* h = nullptr;
        for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"})
            if ((h = dlopen(name, RTLD_NOW | RTLD_LOCAL))) break;
        if (!h) return false;
        Rccl r;
        r.init_all = (InitAll)dlsym(h, "ncclCommInitAll"); r.destroy = (Destroy)dlsym(h, "ncclCommDestroy");
        r.group_start = (Group)dlsym(h, "ncclGroupStart"); r.group_end = (Group)dlsym(h, "ncclGroupEnd");
        r.send = (SendRecv)dlsym(h, "ncclSend"); r.recv = (SendRecv)dlsym(h, "ncclRecv"); r.err = (ErrStr)dlsym(h, "ncclGetErrorString");
        if (!(r.init_all && r.destroy && r.group_start && r.group_end && r.send && r.recv)) { (void)dlclose(h); return false; }
        r.loaded = true;
        *this = r;
        *lib = h;
        return true;
    }
};
Rccl g_rccl;
constexpr int kNcclFloat = 7;       // ncclFloat32 (rccl.h ncclDataType_t)

}  // namespace

void crt_scene::drop_peers() {
    if (!rccl_comms.empty() && g_rccl.destroy)
        for (void* c : rccl_comms) if (c) (void)g_rccl.destroy(c);
    rccl_comms.clear();
    for (crt_scene* p : peers) delete p;
    peers.clear();
    if (!d_gather.empty() || !d_peer_tiles.empty() || !ev_peer.empty()) (void)hipSetDevice(device);
    for (float* b : d_gather) if (b) (void)hipFree(b);
    for (uint2* b : d_peer_tiles) if (b) (void)hipFree(b);
    for (hipEvent_t e : ev_peer) if (e) (void)hipEventDestroy(e);
    d_gather.clear(); d_peer_tiles.clear(); ev_peer.clear();
}

// a complete copy of `src` on another device: configuration by value, scene buffers over the fabric (hipMemcpyPeer), own stream,
// counters and events; frame buffers follow with its shard
static int replicate_scene(const crt_scene* src, int device, crt_scene** out) {
    *out = nullptr;
    HIPCHK(hipSetDevice(device));
    std::unique_ptr<crt_scene> owner(new (std::nothrow) crt_scene);
    crt_scene* r = owner.get();
    if (!r) return fail(CRT_ERR_NOMEM, "crt_set_devices: out of memory");
    r->device = device;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) r->n_cu = prop.multiProcessorCount;
    HIPCHK(hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking));
    r->width = src->width; r->height = src->height; r->max_depth = src->max_depth; r->n_lights = src->n_lights;
    r->tex_width = src->tex_width; r->tex_height = src->tex_height; r->n_textures = src->n_textures;
    r->info = src->info; r->bvh2_stack = src->bvh2_stack; r->stack_entries = src->stack_entries; r->special_materials = src->special_materials;
    r->cam = src->cam; r->have_camera = src->have_camera; r->jitter = src->jitter;
    r->tri_min = src->tri_min; r->inplace_shadow = src->inplace_shadow; r->accel = src->accel; r->refill_min = src->refill_min; r->trace_pool = src->trace_pool; r->count_visits = src->count_visits;
    r->count_batched = src->count_batched;
    r->trace_occupancy = src->trace_occupancy; r->oversubscribe = src->oversubscribe; r->waves_per_workgroup = src->waves_per_workgroup;
    r->lanes_per_ray = src->lanes_per_ray; r->bounce_refill = src->bounce_refill; r->refill_pool = src->refill_pool; r->shadow_pool = src->shadow_pool; r->shadow_refill_min = src->shadow_refill_min; r->shadow_waves = src->shadow_waves; r->persistent = src->persistent; r->sort_shadow = src->sort_shadow;
    r->wave_samples = src->wave_samples; r->wide_first = src->wide_first; r->adaptive_tiles = src->adaptive_tiles; r->timing = src->timing;
    r->ray_bins = src->ray_bins; r->rows_padded = src->rows_padded; r->last_build = src->last_build; r->lean_build = src->lean_build; r->tree_validated = src->tree_validated;
    for (int k = 0; k < 3; ++k) { r->bounds_lo[k] = src->bounds_lo[k]; r->bounds_hi[k] = src->bounds_hi[k]; }
    std::copy(std::begin(src->shared_bytes), std::end(src->shared_bytes), std::begin(r->shared_bytes));
    r->shares_scene = device == src->device;
    if (device != src->device) {          // direct xGMI copies where the platform allows them; staged through the host otherwise
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, device, src->device) == hipSuccess && can) (void)hipDeviceEnablePeerAccess(src->device, 0);
        (void)hipGetLastError();          // "already enabled" is not an error to report later
    }
    for (int k = 0; k < kSharedBufs; ++k) {
        void* const from = src->shared_ptr(k);
        void** const to = r->shared_slot(k);
        const size_t bytes = src->shared_bytes[k];
        if (!from) continue;
        if (device == src->device) { *to = from; continue; }      // the same GPU again: one copy of the scene serves both
        hipError_t e = hipMalloc(to, bytes ? bytes : 16);
        if (e != hipSuccess) return fail(CRT_ERR_NOMEM, std::string("crt_set_devices: hipMalloc: ") + hipGetErrorString(e));
        if (bytes) HIPCHK(hipMemcpyPeer(*to, device, from, src->device, bytes));
    }
    if (src->d_env) {                     // the environment is scene state like the camera: a copy of its own on every logical device
        const size_t n = (size_t)src->env_size * src->env_size;
        int erc = dev_alloc(&r->d_env, n);
        if (erc) return erc;
        if (device == src->device) HIPCHK(hipMemcpy(r->d_env, src->d_env, n * sizeof(float4), hipMemcpyDeviceToDevice));
        else HIPCHK(hipMemcpyPeer(r->d_env, device, src->d_env, src->device, n * sizeof(float4)));
        r->env_size = src->env_size; r->env_flags = src->env_flags;
        for (int k = 0; k < 9; ++k) r->env_rotation[k] = src->env_rotation[k];
        for (int k = 0; k < 3; ++k) r->env_scale[k] = src->env_scale[k];
    }
    int rc = crt::finish_scene_setup(r);
    if (rc) return rc;
    *out = owner.release();
    return CRT_OK;
}

// base_rank / base_world: the shard of the frame the devices divide among themselves — the whole frame (0 of 1) for crt_set_devices,
// the caller's own shard (crt_set_shard) when option "streams" splits it over streams of one GPU: device k takes the tiles
// base_rank + k * base_world, + n * base_world, ... of the Morton order, i.e. every n-th tile of that shard's list starting at its k-th
int crt_set_devices(crt_scene* s, const int32_t* devices, uint32_t n_devices, uint32_t tile) {
    if (s && s->inst && n_devices > 1)
        return fail(CRT_ERR_INVALID, "crt_set_devices: an instanced scene renders on the one device its crt_instances handle lives on");
    if (s && s->camera_rays() && n_devices > 1)
        return fail(CRT_ERR_INVALID, "crt_set_devices: n_devices: a scene with camera rays set (crt_set_camera_rays) renders on one device: crt_clear_camera_rays first");
    const int rc = set_devices_of_shard(s, devices, n_devices, tile, 0u, 1u);
    if (rc == CRT_OK) { s->shard_rank = 0u; s->shard_world = 1u; }      // the devices divide the whole frame (a refused call changes nothing)
    return rc;
}

static int set_devices_of_shard(crt_scene* s, const int32_t* devices, uint32_t n_devices, uint32_t tile, uint32_t base_rank, uint32_t base_world) {
    if (!s || !devices) return fail(CRT_ERR_INVALID, "crt_set_devices: null argument");
    if (s->primary) return fail(CRT_ERR_INVALID, "crt_set_devices: not on a replica");
    if (n_devices == 0 || n_devices > 64) return fail(CRT_ERR_INVALID, "crt_set_devices: 1..64 devices");
    if (tile < 8 || (tile & 7u) || tile > 1024) return fail(CRT_ERR_INVALID, "crt_set_devices: tile must be a multiple of 8 in 8..1024");
    if (devices[0] != s->device) return fail(CRT_ERR_INVALID, "crt_set_devices: devices[0] must be the device the scene was created on");
    int n_visible = 0;
    if (hipGetDeviceCount(&n_visible) != hipSuccess || n_visible <= 0) return fail(CRT_ERR_NO_DEVICE, "crt_set_devices: no HIP device visible");
    bool distinct = true;
    for (uint32_t k = 0; k < n_devices; ++k) {
        if (devices[k] < 0 || devices[k] >= n_visible) return fail(CRT_ERR_INVALID, "crt_set_devices: no such device");
        for (uint32_t j = 0; j < k; ++j) distinct = distinct && devices[j] != devices[k];
    }
    HIPCHK(hipSetDevice(s->device));
    if (n_devices > 1u && s->accel == 0u) { const int prc = ensure_planes(s); if (prc) return prc; }      // replicas copy (or share) the planes (a scene on its BVH2: ensure_planes, later)
    HIPCHK(hipStreamSynchronize(s->stream));
    s->drop_peers();
    s->streams = 1;
    int rc = CRT_OK;
    auto undo = [&](int code) { s->drop_peers(); (void)hipSetDevice(s->device); s->rank = base_rank; s->world = base_world; (void)alloc_frame_buffers(s); return code; };
    try {
        for (uint32_t k = 1; k < n_devices; ++k) {
            crt_scene* p = nullptr;
            if ((rc = replicate_scene(s, devices[k], &p))) return undo(rc);
            p->primary = s;
            s->peers.push_back(p);
            device_share(k, n_devices, base_rank, base_world, &p->rank, &p->world);
            p->tile = tile;
            if ((rc = alloc_frame_buffers(p))) return undo(rc);
        }
        if (hipSetDevice(s->device) != hipSuccess) return undo(fail(CRT_ERR_HIP, "crt_set_devices: hipSetDevice failed"));
        device_share(0u, n_devices, base_rank, base_world, &s->rank, &s->world);
        s->tile = tile;
        if ((rc = alloc_frame_buffers(s))) return undo(rc);
        for (crt_scene* p : s->peers) {                      // where a peer's slice lands on this device, and its tile list
            float* g = nullptr; uint2* t = nullptr; hipEvent_t e = nullptr;
            if ((rc = dev_alloc(&g, 3 * (size_t)p->n_local_pixels))) return undo(rc);
            s->d_gather.push_back(g);
            if ((rc = dev_alloc(&t, p->n_local_tiles))) return undo(rc);
            s->d_peer_tiles.push_back(t);
            if (p->n_local_tiles && hipMemcpy(t, p->tiles.data(), p->tiles.size() * sizeof(uint2), hipMemcpyHostToDevice) != hipSuccess)
                return undo(fail(CRT_ERR_HIP, "crt_set_devices: hipMemcpy H2D failed"));
            // recorded on the peer's stream, waited for on this device's: an event belongs to the device it was created on
            if (hipSetDevice(p->device) != hipSuccess || hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess)
                return undo(fail(CRT_ERR_HIP, "crt_set_devices: hipEventCreate failed"));
            s->ev_peer.push_back(e);
            if (hipSetDevice(s->device) != hipSuccess) return undo(fail(CRT_ERR_HIP, "crt_set_devices: hipSetDevice failed"));
        }
    } catch (const std::exception& e) {
        return undo(fail(CRT_ERR_NOMEM, std::string("crt_set_devices: ") + e.what()));
    }
    // RCCL communicators, one per device, created by this one thread (ncclCommInitAll).  Virtual devices (the same GPU listed more
    // than once: a test arrangement) cannot have them; a missing library is not an error either: the copies below do the same job.
    s->gather_transport = 1;
    if (n_devices > 1 && distinct) {
        const char* env_tr = std::getenv("CRT_GATHER_TRANSPORT");     // "copy": peer copies even where RCCL would load
        if (env_tr && !std::strcmp(env_tr, "copy")) {
            (void)fail(CRT_OK, "crt_set_devices: CRT_GATHER_TRANSPORT=copy, gathering with hipMemcpyPeerAsync");
        } else if (!g_rccl.load(&s->rccl_lib)) {
            (void)fail(CRT_OK, "crt_set_devices: librccl.so not loadable, gathering with hipMemcpyPeerAsync");
        } else {
            std::vector<int> ids(devices, devices + n_devices);
            s->rccl_comms.assign(n_devices, nullptr);
            const int nr = g_rccl.init_all(s->rccl_comms.data(), (int)n_devices, ids.data());
            if (nr != 0) {
                s->rccl_comms.clear();
                (void)fail(CRT_OK, std::string("crt_set_devices: ncclCommInitAll failed (") + (g_rccl.err ? g_rccl.err(nr) : "?") + "), gathering with hipMemcpyPeerAsync");
            } else {
                s->gather_transport = 0;
            }
            (void)hipSetDevice(s->device);                  // ncclCommInitAll visits every device; the scene is complete either way
        }
    }
    return CRT_OK;
}

// [host] the tile list a scene would give logical device `device` of `n_devices` when those divide shard (rank of world) of a width x
// height frame among themselves — crt_set_shard (n_devices = 1), crt_set_devices (rank 0 of world 1) and option "streams" all deal
// tiles through this.  No GPU involved: the multi-GPU bookkeeping can be checked on any machine.
int crt_shard_tiles(uint32_t width, uint32_t height, uint32_t tile, uint32_t rank, uint32_t world, uint32_t device, uint32_t n_devices,
                    uint32_t* tile_xy, size_t capacity, size_t* n_tiles) {
    if (!n_tiles) return fail(CRT_ERR_INVALID, "crt_shard_tiles: null n_tiles");
    if (width == 0 || height == 0 || width > 65535u * 8u || height > 65535u * 8u) return fail(CRT_ERR_INVALID, "crt_shard_tiles: bad resolution");
    if (tile < 8 || (tile & 7u) || tile > 1024) return fail(CRT_ERR_INVALID, "crt_shard_tiles: tile must be a multiple of 8 in 8..1024");
    if (world == 0 || rank >= world || n_devices == 0 || n_devices > 64 || device >= n_devices) return fail(CRT_ERR_INVALID, "crt_shard_tiles: rank/world/device");
    uint32_t r = 0, w = 1;
    device_share(device, n_devices, rank, world, &r, &w);
    std::vector<uint2> tiles;
    try { deal_tiles(width, height, tile, r, w, tiles, nullptr); } catch (const std::exception& e) { return fail(CRT_ERR_NOMEM, std::string("crt_shard_tiles: ") + e.what()); }
    *n_tiles = tiles.size();
    if (tile_xy)
        for (size_t i = 0; i < tiles.size() && i < capacity; ++i) { tile_xy[2 * i] = tiles[i].x; tile_xy[2 * i + 1] = tiles[i].y; }
    return CRT_OK;
}

int crt_get_devices(crt_scene* s, uint32_t* n_devices, int32_t* devices, uint32_t capacity, int32_t* transport, float* last_gather_ms) {
    if (!s) return fail(CRT_ERR_INVALID, "crt_get_devices: null scene");
    if (n_devices) *n_devices = (uint32_t)s->peers.size() + 1u;
    if (devices)
        for (uint32_t k = 0; k < capacity && k <= s->peers.size(); ++k) devices[k] = k == 0 ? s->device : s->peers[k - 1]->device;
    if (transport) *transport = (int32_t)s->gather_transport;
    if (last_gather_ms) *last_gather_ms = s->last_gather_ms;
    return CRT_OK;
}

// every peer's packed sum buffer -> d_gather[k] on the primary device, complete in the primary's stream order when this returns
extern "C++" int crt::gather_peers(crt_scene* s) {       // for crt_outputs.cpp (crt_scene.hpp)
    const auto t0 = std::chrono::steady_clock::now();
    if (s->gather_transport == 0 && !s->rccl_comms.empty()) {
        // grouped point-to-point: device k sends on its own stream (after its frames), device 0 receives on its stream; each slice
        // crosses the one xGMI link between its GPU and this one
        int nr = g_rccl.group_start();
        for (size_t k = 0; k < s->peers.size() && nr == 0; ++k) {
            crt_scene* p = s->peers[k];
            const size_t count = 3 * (size_t)p->n_local_pixels;
            if (!count) continue;
            nr = g_rccl.send(p->d_sum, count, kNcclFloat, 0, s->rccl_comms[k + 1], p->stream);
            if (nr == 0) nr = g_rccl.recv(s->d_gather[k], count, kNcclFloat, (int)k + 1, s->rccl_comms[0], s->stream);
        }
        const int ne = g_rccl.group_end();
        if (nr == 0) nr = ne;
        (void)hipSetDevice(s->device);
        if (nr != 0) {
            // This read fails and the NEXT one gathers with peer copies.  Nothing is waited for here: a failed group can leave unmatched
            // send / recv kernels on the devices' streams, and a synchronise behind them may never return.  (The multi-device path has run
            // on virtual devices and at world size 1 only: DESIGN.md section 7.)
            s->gather_transport = 1;
            return fail(CRT_ERR_HIP, std::string("RCCL gather failed (") + (g_rccl.err ? g_rccl.err(nr) : "?") +
                                     "); this read-back is lost, the next one gathers with hipMemcpyPeerAsync (option gather_transport 1)");
        }
    }
    if (s->gather_transport != 0 || s->rccl_comms.empty()) {
        for (size_t k = 0; k < s->peers.size(); ++k) {
            crt_scene* p = s->peers[k];
            const size_t bytes = 3 * (size_t)p->n_local_pixels * sizeof(float);
            if (!bytes) continue;
            HIPCHK(hipSetDevice(p->device));
            if (p->device == s->device) HIPCHK(hipMemcpyAsync(s->d_gather[k], p->d_sum, bytes, hipMemcpyDeviceToDevice, p->stream));   // a virtual device
            else HIPCHK(hipMemcpyPeerAsync(s->d_gather[k], s->device, p->d_sum, p->device, bytes, p->stream));
            HIPCHK(hipEventRecord(s->ev_peer[k], p->stream));
        }
        HIPCHK(hipSetDevice(s->device));
        for (size_t k = 0; k < s->peers.size(); ++k)
            if (s->peers[k]->n_local_pixels) HIPCHK(hipStreamWaitEvent(s->stream, s->ev_peer[k], 0));
    }
    HIPCHK(hipStreamSynchronize(s->stream));
    s->last_gather_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return CRT_OK;
}

// Measurement aid: enabled lanes per node step of the counting kernels (option count_visits), closest-hit walks in hist[0..64], any-hit
// walks in hist[65..129], accumulated since the previous call (which zeroes it).  Process-wide (one device symbol); null stops it.
int crt_debug_step_hist(crt_scene* s, unsigned long long* hist) {
    static unsigned long long* d_hist = nullptr;
    if (!s) return fail(CRT_ERR_INVALID, "crt_debug_step_hist: null scene");
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipStreamSynchronize(s->stream));
    if (!hist) { crt::set_step_hist(nullptr); return CRT_OK; }
    if (!d_hist) {
        HIPCHK(hipMalloc(reinterpret_cast<void**>(&d_hist), 130 * sizeof(unsigned long long)));
        HIPCHK(hipMemset(d_hist, 0, 130 * sizeof(unsigned long long)));
    }
    HIPCHK(hipMemcpy(hist, d_hist, 130 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    HIPCHK(hipMemset(d_hist, 0, 130 * sizeof(unsigned long long)));
    crt::set_step_hist(d_hist, s->step_hist_mode);
    return CRT_OK;
}

int crt_trace_device(crt_scene* s, const void* d_rays, size_t n, void* d_hits, int mode, void* d_stats, int sync) {
    if (!s || !d_rays || !d_hits) return fail(CRT_ERR_INVALID, "crt_trace_device: null argument");
    if (s->inst) return fail(CRT_ERR_INVALID, "crt_trace_device: an instanced scene has no tree of its own: use crt_instances_trace_device on its handle");
    if (mode < 0 || mode > (CRT_TRACE_ANY | CRT_TRACE_BVH2 | CRT_TRACE_TIE_LOWEST_ID)) return fail(CRT_ERR_INVALID, "crt_trace_device: bad mode");
    const bool any_hit = (mode & CRT_TRACE_ANY) != 0;
    if (n >= (1ull << 31)) return fail(CRT_ERR_LIMIT, "crt_trace_device: too many rays for one launch");
    HIPCHK(hipSetDevice(s->device));
    if (n == 0) return CRT_OK;
    crt::TraceArgs ta{};
    ta.nodes = s->d_nodes; ta.tris = s->d_tris;
    ta.rays = static_cast<const float4*>(d_rays); ta.hits = static_cast<float4*>(d_hits);
    ta.stats = static_cast<uint32_t*>(d_stats); ta.count_ptr = nullptr; ta.n = (uint32_t)n; ta.out_orig_id = 1;
    ta.stack_entries = s->stack_entries;
    ta.refill_min = s->refill_min;
    ta.tri_min = s->tri_min;
    ta.overflow = s->d_overflow;
    ta.pool_split_log2 = s->trace_pool == 64u ? 2u : s->trace_pool == 128u ? 1u : 0u;
    s->n_spans = 0;
    if ((mode & CRT_TRACE_BVH2) && !s->d_bvh2) return fail(CRT_ERR_INVALID, "crt_trace: the scene was created without a BVH2 (desc.bvh)");
    EventSpan* sp = s->new_span(any_hit ? 2 : 1);
    if (sp) crt::set_launch_events(sp->a, sp->b);
    if (mode & CRT_TRACE_BVH2) {
        crt::Bvh2Args ba{};
        ba.nodes = s->d_bvh2; ba.tris = s->d_tris2; ba.rays = ta.rays; ba.hits = ta.hits; ba.stats = ta.stats;
        ba.n = (uint32_t)n; ba.tie = (mode & CRT_TRACE_TIE_LOWEST_ID) ? 1u : 0u; ba.stack_entries = s->bvh2_stack; ba.overflow = s->d_overflow;
        const uint32_t g = s->trace_grid(n, 8);          // every chunk has its workgroup (CRT_CHUNK_LOOP)
        crt::launch_trace_bvh2(ba, any_hit, d_stats != nullptr, g, s->waves_per_workgroup, s->stream);
    } else {
        crt::launch_trace(ta, any_hit ? 1 : 0, d_stats != nullptr, s->trace_grid(n, 8, 1024), s->waves_per_workgroup, s->stream);
    }
    HIPCHK(hipGetLastError());
    s->stats_pending = true;
    s->stats_from_frame = false;
    s->stats.closest_rays = any_hit ? 0 : n;
    s->stats.any_rays = any_hit ? n : 0;
    if (sync) HIPCHK(hipStreamSynchronize(s->stream));
    return CRT_OK;
}

int crt_trace(crt_scene* s, const crt_ray* rays, size_t n, crt_hit* hits, int mode, crt_ray_stats* stats) {
    if (!s || (n && (!rays || !hits))) return fail(CRT_ERR_INVALID, "crt_trace: null argument");
    if (s->inst) return fail(CRT_ERR_INVALID, "crt_trace: an instanced scene has no tree of its own: use crt_instances_trace on its handle");
    HIPCHK(hipSetDevice(s->device));
    if (n == 0) return CRT_OK;
    if (n > s->t_cap) {
        if (s->d_t_rays) hipFree(s->d_t_rays);
        if (s->d_t_hits) hipFree(s->d_t_hits);
        if (s->d_t_stats) hipFree(s->d_t_stats);
        s->d_t_rays = nullptr; s->d_t_hits = nullptr; s->d_t_stats = nullptr; s->t_cap = 0;
        int rc;
        if ((rc = dev_alloc(&s->d_t_rays, 2 * n))) return rc;
        if ((rc = dev_alloc(&s->d_t_hits, n))) return rc;
        if ((rc = dev_alloc(&s->d_t_stats, n))) return rc;
        s->t_cap = n;
    }
    static_assert(sizeof(crt_ray) == 32 && sizeof(crt_hit) == 16 && sizeof(crt_ray_stats) == 4, "ray/hit layout");
    HIPCHK(hipMemcpyAsync(s->d_t_rays, rays, n * sizeof(crt_ray), hipMemcpyHostToDevice, s->stream));
    int rc = crt_trace_device(s, s->d_t_rays, n, s->d_t_hits, mode, stats ? s->d_t_stats : nullptr, 0);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(hits, s->d_t_hits, n * sizeof(crt_hit), hipMemcpyDeviceToHost, s->stream));
    if (stats) HIPCHK(hipMemcpyAsync(stats, s->d_t_stats, n * sizeof(crt_ray_stats), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return CRT_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- crt_update_vertices --
// New positions for an unchanged topology: the CWBVH (node8 boxes re-quantised), the BVH2 and the records of both walks are refitted in
// place on the scene's device (refit.hip), one launch per tree level, deepest first.  The frame path reads none of the state kept for
// this, and a scene that never updates allocates none of it.

static int ensure_refit_state(crt_scene* s) {
    if (s->refit) return CRT_OK;
    std::unique_ptr<RefitState> owner(new (std::nothrow) RefitState);
    RefitState* r = owner.get();
    if (!r) return fail(CRT_ERR_NOMEM, "crt_update_vertices: out of memory");
    r->device = s->device;
    int rc;
    if ((rc = dev_alloc(&r->d_box8, 6 * (size_t)s->info.n_nodes8))) return rc;
    if ((rc = dev_alloc(&r->d_mesh, 1)) || (rc = dev_alloc(&r->d_seg, 1))) return rc;
    HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&r->h_mesh), sizeof(crt::RefitMesh)));
    HIPCHK(hipMemsetAsync(r->d_seg, 0, sizeof(crt::RefitSeg), s->stream));
    // the levels of both trees, found once (parent links and depths on the device, a counting sort of the depths on the host)
    const crt::RefitTree trees[2] = {{s->d_nodes, false, (uint32_t)CRT_NODE_ROWS, (uint32_t)s->info.n_nodes8, 0u},
                                     {s->d_bvh2, true, 0u, (uint32_t)s->info.n_bvh2_nodes, 0u}};
    std::vector<std::vector<uint32_t>> level;
    if ((rc = crt::discover_levels(trees, s->d_bvh2 ? 2 : 1, s->stream, &r->d_order, level))) return rc;
    r->level8 = std::move(level[0]);
    if (s->d_bvh2) r->level2 = std::move(level[1]);
    s->refit = owner.release();
    return CRT_OK;
}

// The front half of crt_update_vertices and crt_rebuild_vertices (`rebuild`): the argument checks under the call's name, the host form's
// positions staged on the device, and the check kernel with the call's one host wait for its verdict.  *verts: the positions on the device
// (the scene's own upload, or the caller's d_user); lo / hi: their bounds.  Nothing the scene shows has been written when this refuses.
// d_normals: new normals already on the scene's device (crt_deform_scene, which passes its name as `caller`), counted by n_normals and
// checked by the same kernel in the same wait.
static int take_vertices(crt_scene* s, bool rebuild, const float* h_verts, const float* d_user, size_t n_vertices, const float* normals, size_t n_normals,
                         const crt_light* lights, size_t n_lights, const float** verts, float lo[3], float hi[3], const float* d_normals = nullptr,
                         const char* caller = nullptr) {
    const std::string who = caller ? caller : rebuild ? "crt_rebuild_vertices: " : "crt_update_vertices: ";
    if (!s || (!h_verts && !d_user)) return fail(CRT_ERR_INVALID, who + "null argument");
    if (s->inst)
        return fail(CRT_ERR_INVALID, who + "an instanced scene's geometry belongs to its handle: use " +
                                         (rebuild ? "crt_instances_replace_meshes" : "crt_instances_update_meshes"));
    if (s->primary) return fail(CRT_ERR_INVALID, who + "not on a replica");
    if (rebuild) {
        if (!s->info.built_on_device)
            return fail(CRT_ERR_INVALID, who + "only a scene built on the device (CRT_BUILD_LBVH_ON_DEVICE) is rebuilt in place; one created from host arrays is created again");
        for (const crt_scene* p : s->peers)
            if (!p->shares_scene)
                return fail(CRT_ERR_INVALID, who + "a replica on another GPU (crt_set_devices) cannot follow a rebuild: return to one device, rebuild, and set the devices again");
    }
    if (n_vertices != s->n_vertices) return fail(CRT_ERR_INVALID, who + "n_vertices differs from the count given at create");
    if ((normals || d_normals) && n_normals != s->n_normals) return fail(CRT_ERR_INVALID, who + "n_normals differs from the count given at create");
    if (lights && n_lights != s->n_lights) return fail(CRT_ERR_INVALID, who + "n_lights differs from the count given at create");
    if (normals)
        for (size_t i = 0; i < 3 * n_normals; ++i)
            if (!std::isfinite(normals[i])) return fail(CRT_ERR_INVALID, who + "a normal is not finite");
    HIPCHK(hipSetDevice(s->device));
    int rc;
    if (!s->intake) {
        std::unique_ptr<VertexIntake> owner(new (std::nothrow) VertexIntake);
        if (!owner) return fail(CRT_ERR_NOMEM, who + "out of memory");
        if ((rc = dev_alloc(&owner->d_check, 16))) return rc;
        HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&owner->h_check), 16 * sizeof(uint32_t)));
        HIPCHK(hipEventCreate(&owner->ev_a));
        HIPCHK(hipEventCreate(&owner->ev_b));
        s->intake = owner.release();
    }
    VertexIntake* in = s->intake;
    hipStream_t st = s->stream;
    *verts = d_user;
    if (h_verts) {
        if (!in->d_verts && (rc = dev_alloc(&in->d_verts, 3 * n_vertices))) return rc;
        HIPCHK(hipMemcpyAsync(in->d_verts, h_verts, 3 * n_vertices * sizeof(float), hipMemcpyHostToDevice, st));
        *verts = in->d_verts;
    }
    const size_t n_check = d_normals ? 16 : 8;    // words 8..15: the same verdict over the device normals
    HIPCHK(hipMemsetAsync(in->d_check, 0, n_check * sizeof(uint32_t), st));
    crt::launch_check_vertices(*verts, (uint32_t)n_vertices, in->d_check, st);
    if (d_normals) crt::launch_check_vertices(d_normals, (uint32_t)n_normals, in->d_check + 8, st);
    HIPCHK(hipMemcpyAsync(in->h_check, in->d_check, n_check * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (in->times_pending) {                      // an unsynchronised update's events have passed by now: read them before this call records its own
        HIPCHK(hipEventElapsedTime(&in->device_ms, in->ev_a, in->ev_b));
        in->times_pending = false;
    }
    if (in->h_check[0]) return fail(CRT_ERR_INVALID, who + "a vertex coordinate is not finite or exceeds 1e18");
    if (d_normals && in->h_check[8]) return fail(CRT_ERR_INVALID, who + "a normal is not finite or exceeds 1e18");
    for (int k = 0; k < 3; ++k) { hi[k] = crt::rf::key_to_float(in->h_check[1 + k]); lo[k] = crt::rf::key_to_float(~in->h_check[4 + k]); }
    return CRT_OK;
}

// After the geometry of scene x (a primary or a replica) changed: the new bounds (ray_bins / sort_shadow cell grid), a new tile-cost
// measurement, and the sum cleared as crt_reset does
static int refresh_after_geometry(crt_scene* x, const float lo[3], const float hi[3]) {
    for (int k = 0; k < 3; ++k) { x->bounds_lo[k] = lo[k]; x->bounds_hi[k] = hi[k]; }
    x->tile_state = crt_scene::TILES_WANT;
    const int rc = ensure_frame(x);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(x->d_sum, 0, 3 * (size_t)std::max<uint32_t>(x->n_local_pixels, 1) * sizeof(float), x->stream));
    return CRT_OK;
}

// normals / lights: host arrays or null; d_normals: normals on the scene's device or null
static int update_impl(crt_scene* s, const float* h_verts, const float* d_user, size_t n_vertices, const float* normals, size_t n_normals,
                       const crt_light* lights, size_t n_lights, int sync, const float* d_normals = nullptr, const char* caller = nullptr) {
    const auto t_begin = std::chrono::steady_clock::now();
    const float* verts = nullptr;
    float lo[3], hi[3];
    int rc = take_vertices(s, false, h_verts, d_user, n_vertices, normals, n_normals, lights, n_lights, &verts, lo, hi, d_normals, caller);
    if (rc) return rc;
    if ((rc = ensure_refit_state(s))) return rc;
    VertexIntake* in = s->intake;
    RefitState* r = s->refit;
    hipStream_t st = s->stream;
    const uint32_t nv = (uint32_t)n_vertices;
    // the scene as one refit mesh: d_triangles in leaf-slot order, keyed by the slot in e1.w.  The stream is idle here, so the previous
    // call's copy of h_mesh is done; the refit launches read it after this copy, in stream order.
    *r->h_mesh = crt::RefitMesh{verts, reinterpret_cast<const int32_t*>(s->d_triangles), 12u, (uint32_t)s->n_slots, 7u, nv};
    HIPCHK(hipMemcpyAsync(r->d_mesh, r->h_mesh, sizeof(crt::RefitMesh), hipMemcpyHostToDevice, st));

    // every stream that reads the scene's buffers is done with the old scene before they change (its own stream is, by order)
    r->ev_peer.resize(s->peers.size(), nullptr);
    for (size_t k = 0; k < s->peers.size(); ++k) {
        crt_scene* p = s->peers[k];
        HIPCHK(hipSetDevice(p->device));
        if (!r->ev_peer[k]) HIPCHK(hipEventCreateWithFlags(&r->ev_peer[k], hipEventDisableTiming));
        HIPCHK(hipEventRecord(r->ev_peer[k], p->stream));
        HIPCHK(hipSetDevice(s->device));
        HIPCHK(hipStreamWaitEvent(st, r->ev_peer[k], 0));
    }
    if (normals && n_normals) HIPCHK(hipMemcpyAsync(s->d_normals, normals, 3 * n_normals * sizeof(float), hipMemcpyHostToDevice, st));
    if (d_normals && n_normals) HIPCHK(hipMemcpyAsync(s->d_normals, d_normals, 3 * n_normals * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (lights && n_lights) HIPCHK(hipMemcpyAsync(s->d_lights, lights, n_lights * sizeof(crt_light), hipMemcpyHostToDevice, st));

    HIPCHK(hipEventRecord(in->ev_a, st));
    const uint32_t n8 = (uint32_t)s->info.n_nodes8, n_tris8 = (uint32_t)s->info.n_tris8, n_slots = (uint32_t)s->n_slots;
    crt::launch_refit_records(s->d_tris, (uint32_t)CRT_TRI_ROWS, n_tris8, r->d_seg, 1u, n_tris8, r->d_mesh, st);
    if (s->d_tris2) crt::launch_refit_records(s->d_tris2, 3u, n_slots, r->d_seg, 1u, n_slots, r->d_mesh, st);
    if (s->d_bvh2)
        for (size_t l = r->level2.size() - 1; l-- > 0;)
            crt::launch_refit_bvh2_level(s->d_bvh2, (uint32_t)s->info.n_bvh2_nodes, r->d_order + r->level2[l], r->level2[l + 1] - r->level2[l],
                                         s->d_triangles, n_slots, verts, st);
    for (size_t l = r->level8.size() - 1; l-- > 0;)
        crt::launch_refit_node8_level(s->d_nodes, (uint32_t)CRT_NODE_ROWS, 0u, n8, r->d_order + r->level8[l], r->d_seg, 1u, r->level8[l + 1] - r->level8[l],
                                      s->d_tris, (uint32_t)CRT_TRI_ROWS, n_tris8, r->d_mesh, r->d_box8, st);
    if (s->d_planes) crt::launch_expand_planes(s->d_nodes, (uint32_t)CRT_NODE_ROWS, s->d_planes, n8, st);
    if (hipGetLastError() != hipSuccess) return fail(CRT_ERR_HIP, "crt_update_vertices: refit launch failed");
    HIPCHK(hipEventRecord(in->ev_b, st));

    if ((rc = refresh_after_geometry(s, lo, hi))) return rc;
    // replicas: on this GPU they share the refitted buffers and only wait for them; on another GPU they receive them by peer copy
    for (crt_scene* p : s->peers) {
        HIPCHK(hipSetDevice(p->device));
        HIPCHK(hipStreamWaitEvent(p->stream, in->ev_b, 0));
        if (!p->shares_scene) {
            for (const SharedBuf k : {kSharedNodes, kSharedTris, kSharedTris2, kSharedBvh2, kSharedNormals, kSharedLights}) {      // what a refit rewrites
                void* const src = s->shared_ptr(k);
                void* const dst = p->shared_ptr(k);
                const size_t bytes = s->shared_bytes[k];
                if (src && dst && bytes) HIPCHK(hipMemcpyPeerAsync(dst, p->device, src, s->device, bytes, p->stream));
            }
            if (p->d_planes) crt::launch_expand_planes(p->d_nodes, (uint32_t)CRT_NODE_ROWS, p->d_planes, n8, p->stream);
        }
        if ((rc = refresh_after_geometry(p, lo, hi))) { (void)hipSetDevice(s->device); return rc; }
    }
    HIPCHK(hipSetDevice(s->device));
    in->have_times = true;
    in->times_pending = true;
    if (sync) {
        HIPCHK(hipStreamSynchronize(st));
        for (crt_scene* p : s->peers) { HIPCHK(hipSetDevice(p->device)); HIPCHK(hipStreamSynchronize(p->stream)); }
        HIPCHK(hipSetDevice(s->device));
        HIPCHK(hipEventElapsedTime(&in->device_ms, in->ev_a, in->ev_b));
        in->times_pending = false;
    }
    in->wall_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    return CRT_OK;
}

// ---------------------------------------------------------------- crt_rebuild_vertices --
// New positions and a new tree: crt_create.cpp scene_create_device_built's chain (build_device_tree) run again over the source-order
// triangles into new buffers, published at the end.  Until then nothing a walk, a frame or a debug read sees has changed.

static int ensure_rebuild_state(crt_scene* s) {
    if (s->rebuild) return CRT_OK;
    std::unique_ptr<RebuildState> owner(new (std::nothrow) RebuildState);
    RebuildState* r = owner.get();
    if (!r) return fail(CRT_ERR_NOMEM, "crt_rebuild_vertices: out of memory");
    // one triangle per slot and no duplicates in a device build: the records' (original id, slot) pairs are a permutation
    const uint32_t n = (uint32_t)s->info.n_tris8;
    int rc;
    if ((rc = dev_alloc(&r->d_src, n))) return rc;
    crt::launch_scatter_source(s->d_tris, (uint32_t)CRT_TRI_ROWS, n, reinterpret_cast<const crt_triangle*>(s->d_triangles), r->d_src, s->stream);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s->stream) != hipSuccess)
        return fail(CRT_ERR_HIP, "crt_rebuild_vertices: the source-order scatter failed");
    s->rebuild = owner.release();
    return CRT_OK;
}

static int rebuild_impl(crt_scene* s, const float* h_verts, const float* d_user, size_t n_vertices, const float* normals, size_t n_normals,
                        const crt_light* lights, size_t n_lights, const float* d_normals = nullptr, const char* caller = nullptr) {
    const auto t_begin = std::chrono::steady_clock::now();
    const float* verts = nullptr;
    float lo[3], hi[3];
    int rc = take_vertices(s, true, h_verts, d_user, n_vertices, normals, n_normals, lights, n_lights, &verts, lo, hi, d_normals, caller);
    if (rc) return rc;
    if ((rc = ensure_rebuild_state(s))) return rc;
    VertexIntake* in = s->intake;
    hipStream_t st = s->stream;

    // the new tree, in buffers of its own: whatever is left in `fresh` when this returns is freed
    const uint32_t n = (uint32_t)s->info.n_tris8;
    crt::DeviceArena arena;
    hipError_t he = arena.reserve(crt::device_tree_tmp_bytes(n, s->gpu_build_flags));
    if (he != hipSuccess) return fail(CRT_ERR_NOMEM, std::string("crt_rebuild_vertices: hipMalloc: ") + hipGetErrorString(he));
    crt::DeviceTree fresh;
    if ((rc = dev_alloc(&fresh.bvh2, (2 * (size_t)n - 1) * 2))) return rc;
    HIPCHK(hipEventRecord(in->ev_a, st));
    if ((rc = crt::build_device_tree(s->rebuild->d_src, verts, n, s->gpu_build_flags, arena, reinterpret_cast<crt_flatnode*>(fresh.bvh2), crt::kSceneTree, st,
                                     "crt_rebuild_vertices: ", &fresh))) return rc;
    // the traversal's strides, as finish_scene_setup pads a create's arrays
    if ((rc = crt::pad_rows(st, "crt_rebuild_vertices: ", &fresh.nodes, 5u, (uint32_t)CRT_NODE_ROWS, (size_t)fresh.n8))) return rc;
    if ((rc = crt::pad_rows(st, "crt_rebuild_vertices: ", &fresh.tris, 3u, (uint32_t)CRT_TRI_ROWS, (size_t)n))) return rc;
    if (s->d_planes) {                            // re-expanded as create's first frame does; a scene without them still builds them lazily
        if ((rc = dev_alloc(&fresh.planes, (size_t)fresh.n8 * 12))) return rc;
        crt::launch_expand_planes(fresh.nodes, (uint32_t)CRT_NODE_ROWS, fresh.planes, fresh.n8, st);
    }
    HIPCHK(hipEventRecord(in->ev_b, st));
    if (hipStreamSynchronize(st) != hipSuccess || hipGetLastError() != hipSuccess) return fail(CRT_ERR_HIP, "crt_rebuild_vertices: scene assembly kernels failed");
    // every stream that reads the shared buffers is done with the old tree (replicas live on this device: take_vertices checked)
    for (crt_scene* p : s->peers) HIPCHK(hipStreamSynchronize(p->stream));

    // ---- publish: nothing below can refuse ----
    if (normals && n_normals) HIPCHK(hipMemcpyAsync(s->d_normals, normals, 3 * n_normals * sizeof(float), hipMemcpyHostToDevice, st));
    if (d_normals && n_normals) HIPCHK(hipMemcpyAsync(s->d_normals, d_normals, 3 * n_normals * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (lights && n_lights) HIPCHK(hipMemcpyAsync(s->d_lights, lights, n_lights * sizeof(crt_light), hipMemcpyHostToDevice, st));
    crt::adopt_tree(s, fresh);
    delete s->refit;                              // its level order described the old tree: the next update finds the new tree's
    s->refit = nullptr;
    if ((rc = refresh_after_geometry(s, lo, hi))) return rc;
    for (crt_scene* p : s->peers) {               // the same buffers, borrowed
        p->d_bvh2 = s->d_bvh2; p->d_nodes = s->d_nodes; p->d_tris = s->d_tris; p->d_triangles = s->d_triangles; p->d_tris2 = s->d_tris2;
        p->d_planes = p->d_planes ? s->d_planes : nullptr;
        p->info = s->info; p->bvh2_stack = s->bvh2_stack; p->stack_entries = s->stack_entries; p->tree_validated = s->tree_validated;
        std::copy(std::begin(s->shared_bytes), std::end(s->shared_bytes), std::begin(p->shared_bytes));
        if (!p->d_planes) p->shared_bytes[kSharedPlanes] = 0;     // not borrowed yet: ensure_planes notes it when it is
        if ((rc = refresh_after_geometry(p, lo, hi))) return rc;
    }
    HIPCHK(hipStreamSynchronize(st));
    for (crt_scene* p : s->peers) HIPCHK(hipStreamSynchronize(p->stream));
    HIPCHK(hipEventElapsedTime(&in->device_ms, in->ev_a, in->ev_b));
    in->have_times = true;
    in->wall_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    return CRT_OK;
}

// crt_deform_scene's way in (crt_deform.cpp): positions and, unless null, normals on the scene's device, refitted or rebuilt
int crt::scene_take_device_geometry(crt_scene* s, const float* d_vertices, size_t n_vertices, const float* d_normals, size_t n_normals, bool rebuild,
                                    int sync, const char* caller) {
    if (rebuild) return rebuild_impl(s, nullptr, d_vertices, n_vertices, nullptr, n_normals, nullptr, 0, d_normals, caller);
    return update_impl(s, nullptr, d_vertices, n_vertices, nullptr, n_normals, nullptr, 0, sync, d_normals, caller);
}

extern "C" {

int crt_rebuild_vertices(crt_scene* s, const float* vertices, size_t n_vertices, const float* normals, size_t n_normals, const crt_light* lights,
                         size_t n_lights) {
    if (!vertices) return fail(CRT_ERR_INVALID, "crt_rebuild_vertices: null vertices");
    try {
        return rebuild_impl(s, vertices, nullptr, n_vertices, normals, n_normals, lights, n_lights);
    } catch (const std::exception& e) {
        return fail(CRT_ERR_NOMEM, std::string("crt_rebuild_vertices: ") + e.what());
    }
}

int crt_rebuild_vertices_device(crt_scene* s, const void* d_vertices, size_t n_vertices, int sync) {
    if (!d_vertices) return fail(CRT_ERR_INVALID, "crt_rebuild_vertices_device: null vertices");
    (void)sync;                                   // the builders wait on the host: a rebuild always returns done
    try {
        return rebuild_impl(s, nullptr, static_cast<const float*>(d_vertices), n_vertices, nullptr, 0, nullptr, 0);
    } catch (const std::exception& e) {
        return fail(CRT_ERR_NOMEM, std::string("crt_rebuild_vertices_device: ") + e.what());
    }
}

int crt_get_tree_cost(crt_scene* s, crt_tree_cost* out) {
    if (!s || !out) return fail(CRT_ERR_INVALID, "crt_get_tree_cost: null argument");
    if (s->inst) return fail(CRT_ERR_INVALID, "crt_get_tree_cost: an instanced scene has no tree of its own: use crt_instances_tree_cost on its handle");
    HIPCHK(hipSetDevice(s->device));
    return crt::tree_cost_on_device(s->d_nodes, (uint32_t)CRT_NODE_ROWS, 0u, s->info.n_nodes8, 0u, s->stream, out);
}

int crt_update_vertices(crt_scene* s, const float* vertices, size_t n_vertices, const float* normals, size_t n_normals, const crt_light* lights,
                        size_t n_lights) {
    if (!vertices) return fail(CRT_ERR_INVALID, "crt_update_vertices: null vertices");
    try {
        return update_impl(s, vertices, nullptr, n_vertices, normals, n_normals, lights, n_lights, 1);
    } catch (const std::exception& e) {
        return fail(CRT_ERR_NOMEM, std::string("crt_update_vertices: ") + e.what());
    }
}

int crt_update_vertices_device(crt_scene* s, const void* d_vertices, size_t n_vertices, int sync) {
    if (!d_vertices) return fail(CRT_ERR_INVALID, "crt_update_vertices_device: null vertices");
    try {
        return update_impl(s, nullptr, static_cast<const float*>(d_vertices), n_vertices, nullptr, 0, nullptr, 0, sync);
    } catch (const std::exception& e) {
        return fail(CRT_ERR_NOMEM, std::string("crt_update_vertices_device: ") + e.what());
    }
}

int crt_last_update_ms(crt_scene* s, float* device_ms, float* wall_ms) {
    if (!s) return fail(CRT_ERR_INVALID, "crt_last_update_ms: null scene");
    VertexIntake* r = s->intake;
    if (!r || !r->have_times) return fail(CRT_ERR_INVALID, "crt_last_update_ms: no update yet");
    if (r->times_pending) {
        HIPCHK(hipSetDevice(s->device));
        HIPCHK(hipEventSynchronize(r->ev_b));
        HIPCHK(hipEventElapsedTime(&r->device_ms, r->ev_a, r->ev_b));
        r->times_pending = false;
    }
    if (device_ms) *device_ms = r->device_ms;
    if (wall_ms) *wall_ms = r->wall_ms;
    return CRT_OK;
}

int crt_debug_read_accel(crt_scene* s, int which, void* dst, size_t cap_bytes, size_t* n_out) {
    if (!s) return fail(CRT_ERR_INVALID, "crt_debug_read_accel: null scene");
    if (s->inst) return fail(CRT_ERR_INVALID, "crt_debug_read_accel: an instanced scene has no tree of its own: use crt_instances_debug_read on its handle");
    const void* src = nullptr;
    size_t n = 0, item = 0, pitch = 0;
    switch (which) {
        case 0: src = s->d_nodes; n = s->info.n_nodes8; item = sizeof(crt_node8); pitch = (size_t)CRT_NODE_ROWS * 16; break;
        case 1: src = s->d_tris; n = s->info.n_tris8; item = 48; pitch = (size_t)CRT_TRI_ROWS * 16; break;
        case 2: src = s->d_bvh2; n = src ? s->info.n_bvh2_nodes : 0; item = sizeof(crt_flatnode); pitch = item; break;
        case 3: src = s->d_tris2; n = src ? s->n_slots : 0; item = 48; pitch = item; break;
        default: return fail(CRT_ERR_INVALID, "crt_debug_read_accel: which must be 0..3");
    }
    if (n_out) *n_out = n;
    if (!dst || n == 0) return CRT_OK;
    if (cap_bytes < n * item) return fail(CRT_ERR_INVALID, "crt_debug_read_accel: destination too small");
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipStreamSynchronize(s->stream));
    HIPCHK(hipMemcpy2D(dst, item, src, pitch, item, n, hipMemcpyDeviceToHost));
    return CRT_OK;
}

}  // extern "C"
