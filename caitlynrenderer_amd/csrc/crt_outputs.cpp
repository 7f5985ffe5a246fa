// Everything that leaves the library as an image (include/crt.h): the running sum, the first-hit feature buffers, the
// denoised image (§22), the accumulated image (§23), the bloomed image (§30), the fogged image (§33), and the RGBA8 of the first four.  The five are described
// once (Image) and read, exposed and resolved through one path each ("Where an image leaves"); crt_frames.cpp renders the frames these read.
#include <cmath>
#include <cstring>
#include <exception>
#include <mutex>
#include <new>

#include "bloom.hpp"
#include "crt_scene.hpp"
#include "denoise.hpp"
#include "display.hpp"
#include "fog.hpp"
#include "instances.hpp"

using crt::dev_alloc;
using crt::ensure_frame;
using crt::fail;
using crt::frame_args;

namespace {

// crt_render_aov, crt_denoise and crt_temporal work on whole frames in one place
int require_single_device(const crt_scene* s, const char* who) {
    if (s->primary || (!s->peers.empty() && s->streams <= 1u))
        return fail(CRT_ERR_INVALID, std::string(who) + ": a scene on one device only (crt_set_devices has dealt this one's tiles to several)");
    return CRT_OK;
}

int check_sigma_depth(float sigma_depth, const char* who) {
    if (!(std::isfinite(sigma_depth) && sigma_depth >= 1e-6f && sigma_depth <= 1e6f))
        return fail(CRT_ERR_INVALID, std::string(who) + ": sigma_depth must be finite and in [1e-6, 1e6]");
    return CRT_OK;
}

// the channel buffers as the kernels take them: what crt_render_aov writes, and the guides crt_denoise and crt_temporal read
crt::AovOut aov_channels(const AovState* av) {
    crt::AovOut c{};
    c.hit = static_cast<float4*>(av->d_chan[0]); c.ids = static_cast<int4*>(av->d_chan[1]); c.normal = static_cast<float4*>(av->d_chan[2]);
    c.albedo = static_cast<float4*>(av->d_chan[3]); c.emission = static_cast<float4*>(av->d_chan[4]);
    return c;
}

int copy_and_sync(crt_scene* s, void* dst, const void* d_src, size_t n_bytes) {
    HIPCHK(hipMemcpyAsync(dst, d_src, n_bytes, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return CRT_OK;
}

template <typename T>
int sync_and_expose(crt_scene* s, const T* d_src, const T** d_out) {
    HIPCHK(hipStreamSynchronize(s->stream));
    *d_out = d_src;
    return CRT_OK;
}

// launch(f, packed, grid) for this scene's packed tile buffer, then for every peer's as gathered to this device ("multi-GPU
// gather happens inside these"), each with its own tile list; tiles are disjoint, so the order does not matter
template <typename Launch>
int for_each_slice(crt_scene* s, Launch launch) {
    if (s->n_local_pixels) launch(frame_args(s, 0.f, 0.f), s->d_sum, s->flat_grid(s->n_local_pixels));
    if (s->peers.empty()) return CRT_OK;
    const int rc = crt::gather_peers(s);
    if (rc) return rc;
    for (size_t k = 0; k < s->peers.size(); ++k) {
        const crt_scene* p = s->peers[k];
        if (!p->n_local_pixels) continue;
        crt::FrameArgs f = frame_args(p, 0.f, 0.f);
        f.tile_xy = s->d_peer_tiles[k];
        f.tile_order = nullptr;
        launch(f, s->d_gather[k], s->flat_grid(p->n_local_pixels));
    }
    return CRT_OK;
}

int untile_to_linear(crt_scene* s) {
    const size_t n = 3 * (size_t)s->width * s->height;
    if (!s->d_linear) { int rc = dev_alloc(&s->d_linear, n); if (rc) return rc; }
    HIPCHK(hipMemsetAsync(s->d_linear, 0, n * sizeof(float), s->stream));
    return for_each_slice(s, [s](const crt::FrameArgs& f, const float* packed, uint32_t grid) { crt::launch_untile(f, packed, s->d_linear, grid, s->stream); });
}

// The pinned gamma of the resolve kernels: thr[j] (j = 1..255) = the smallest float x >= 0 whose reference byte
// (uint8)(clamp01((float)pow((double)x, 1 / 2.2)) * 255 + 0.5) is >= j — pow in double, rounded once.  The byte of any x is then the number of
// thresholds it has reached, whatever the device's own powf does in its last bits.  (oracle/oracle.c builds the same table by itself.)
const float* gamma_thresholds() {
    static float thr[256];
    static std::once_flag once;
    std::call_once(once, [] {
        auto ref_byte = [](float x) {
            float v = (float)std::pow((double)x, (double)(1.0f / 2.2f));
            v = v < 0.f ? 0.f : v > 1.f ? 1.f : v;
            return (uint32_t)(uint8_t)(v * 255.0f + 0.5f);
        };
        thr[0] = 0.f;
        for (uint32_t j = 1; j < 256u; ++j) {
            uint32_t lo = 0u, hi = 0x7f800000u;              // bit patterns of the non-negative floats, ordered like their values; ref_byte(+inf) = 255
            while (lo < hi) {
                const uint32_t mid = lo + (hi - lo) / 2u;
                float x; std::memcpy(&x, &mid, 4);
                if (ref_byte(x) >= j) hi = mid; else lo = mid + 1u;
            }
            std::memcpy(&thr[j], &lo, 4);
        }
    });
    return thr;
}

// One of the five float images (width * height * 3, linear pixel order) and its RGBA8.  The running sum lives as packed tiles, on every
// device of the scene: a read un-tiles (and gathers) it into d_linear first, a resolve tone-maps the tiles directly.  The other four are
// what their call left on the stream, on a device that must be there, and exist only after such a call.  `rgba` is null for an image
// without a resolve (the fogged image): no resolve entry names it.
struct Image {
    bool packed;             // the running sum
    const char* refusal;     // null = it exists; else why not, as it follows the entry's name
    float* const* rgb;       // where its float pointer is (the sum's d_linear is allocated by its first un-tiling)
    uint8_t** rgba;          // where its RGBA8 pointer is: a buffer of its own, allocated by its first resolve
};
typedef Image (*ImageOf)(crt_scene*);

Image sum_image(crt_scene* s) { return {true, nullptr, &s->d_linear, &s->d_rgba}; }
Image denoised_image(crt_scene* s) {
    DenoiseState* const dn = s->denoise;
    if (!dn || !dn->valid) return {false, ": no crt_denoise call has succeeded on this scene", nullptr, nullptr};
    return {false, nullptr, &dn->d_out, &dn->d_rgba};
}
Image temporal_image(crt_scene* s) {
    TemporalState* const ts = s->temporal;
    if (!ts || !ts->valid) return {false, ": no crt_temporal call has succeeded on this scene", nullptr, nullptr};
    return {false, nullptr, &ts->d_out, &ts->d_rgba};
}
Image bloom_image(crt_scene* s) {
    BloomState* const bl = s->bloom;
    if (!bl || !bl->valid) return {false, ": no crt_bloom call has succeeded on this scene", nullptr, nullptr};
    return {false, nullptr, &bl->d_out, &bl->d_rgba};
}

Image fogged_image(crt_scene* s) {       // it has no resolve, so no RGBA8 of its own
    FogState* const fg = s->fog;
    if (!fg || !fg->composited) return {false, ": no crt_fog_composite call has succeeded on this scene", nullptr, nullptr};
    return {false, nullptr, &fg->d_fogged, nullptr};
}

int null_argument(const char* who) { return fail(CRT_ERR_INVALID, std::string(who) + ": null argument"); }

// What every accessor of an image does after its null check, in this order: the visible device and the image's existence (not asked of
// the sum), the size of the caller's buffer, the scene's device made current.
int begin_image(crt_scene* s, const Image& im, const char* who, bool size_ok = true, const char* size_text = "") {
    if (!im.packed) {
        const int rc = crt::require_device();
        if (rc) return rc;
        if (im.refusal) return fail(CRT_ERR_INVALID, std::string(who) + im.refusal);
    }
    if (!size_ok) return fail(CRT_ERR_INVALID, std::string(who) + size_text);
    HIPCHK(hipSetDevice(s->device));
    return CRT_OK;
}

// its floats up to date in stream order
int update_image(crt_scene* s, const Image& im) {
    if (!im.packed) return CRT_OK;
    const int rc = ensure_frame(s);
    return rc ? rc : untile_to_linear(s);
}

int read_image(crt_scene* s, ImageOf image_of, const char* who, float* rgb, size_t n_floats) {
    if (!s || !rgb) return null_argument(who);
    const Image im = image_of(s);
    int rc = begin_image(s, im, who, n_floats == 3 * (size_t)s->width * s->height, ": n_floats must be width*height*3");
    if (rc || (rc = update_image(s, im))) return rc;
    return copy_and_sync(s, rgb, *im.rgb, n_floats * sizeof(float));
}

int expose_image(crt_scene* s, ImageOf image_of, const char* who, const float** d_rgb) {
    if (!s || !d_rgb) return null_argument(who);
    *d_rgb = nullptr;
    const Image im = image_of(s);
    int rc = begin_image(s, im, who);
    if (rc || (rc = update_image(s, im))) return rc;
    return sync_and_expose<float>(s, *im.rgb, d_rgb);
}

// the table on the device, from the first resolve or display of any image on
int ensure_gamma(crt_scene* s) {
    if (s->d_gamma) return CRT_OK;
    const int rc = dev_alloc(&s->d_gamma, 256);
    if (rc) return rc;
    HIPCHK(hipMemcpy(s->d_gamma, gamma_thresholds(), 256 * sizeof(float), hipMemcpyHostToDevice));
    return CRT_OK;
}

// tone-mapped RGBA8 of the image in its own buffer (this device), through the pinned gamma: the sum straight from the packed tile buffers,
// this scene's and its peers' as gathered
int resolve_image(crt_scene* s, const Image& im, float inv_count) {
    const size_t npx = (size_t)s->width * s->height;
    int rc;
    if (im.packed && (rc = ensure_frame(s))) return rc;
    if (!*im.rgba && (rc = dev_alloc(im.rgba, 4 * npx))) return rc;
    if ((rc = ensure_gamma(s))) return rc;
    uint8_t* const d_rgba = *im.rgba;
    if (!im.packed) {
        crt::launch_resolve(*im.rgb, (uint32_t)npx, inv_count, s->d_gamma, d_rgba, s->flat_grid((uint32_t)npx), s->stream);
        HIPCHK(hipGetLastError());
        return CRT_OK;
    }
    // a shard of a frame (crt_set_shard with world > 1) leaves the other ranks' pixels at 0
    if (s->shard_world > 1u) HIPCHK(hipMemsetAsync(d_rgba, 0, 4 * npx, s->stream));
    return for_each_slice(s, [=](const crt::FrameArgs& f, const float* packed, uint32_t grid) {
        crt::launch_resolve_packed(f, packed, inv_count, s->d_gamma, d_rgba, grid, s->stream);
    });
}

int resolve_image_host(crt_scene* s, ImageOf image_of, const char* who, float inv_count, uint8_t* rgba, size_t n_bytes) {
    if (!s || !rgba) return null_argument(who);
    const Image im = image_of(s);
    int rc = begin_image(s, im, who, n_bytes == 4 * (size_t)s->width * s->height, ": n_bytes must be width*height*4");
    if (rc || (rc = resolve_image(s, im, inv_count))) return rc;
    // through the scene's pinned staging buffer: a copy into pageable memory is staged by the runtime in small pieces (8.3 MB: ~2.5 ms against 0.4)
    if (!s->h_rgba) HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&s->h_rgba), n_bytes));
    if ((rc = copy_and_sync(s, s->h_rgba, *im.rgba, n_bytes))) return rc;
    std::memcpy(rgba, s->h_rgba, n_bytes);
    return CRT_OK;
}

int resolve_image_device(crt_scene* s, ImageOf image_of, const char* who, float inv_count, const uint8_t** d_rgba, int sync) {
    if (!s || !d_rgba) return null_argument(who);
    *d_rgba = nullptr;
    const Image im = image_of(s);
    int rc = begin_image(s, im, who);
    if (rc || (rc = resolve_image(s, im, inv_count))) return rc;
    if (sync) HIPCHK(hipStreamSynchronize(s->stream));
    *d_rgba = *im.rgba;
    return CRT_OK;
}

}  // namespace

// ---------------------------------------------------------------- the running sum --

int crt_read_sum(crt_scene* s, float* rgb, size_t n_floats) { return read_image(s, sum_image, "crt_read_sum", rgb, n_floats); }
int crt_sum_device(crt_scene* s, const float** d_rgb) { return expose_image(s, sum_image, "crt_sum_device", d_rgb); }
int crt_resolve(crt_scene* s, float inv_count, uint8_t* rgba, size_t n_bytes) { return resolve_image_host(s, sum_image, "crt_resolve", inv_count, rgba, n_bytes); }
int crt_resolve_device(crt_scene* s, float inv_count, const uint8_t** d_rgba, int sync) { return resolve_image_device(s, sum_image, "crt_resolve_device", inv_count, d_rgba, sync); }

// ---------------------------------------------------------------- crt_render_aov --
// First-hit feature buffers of the current view: enqueued on the scene's stream behind whatever frames are queued there.
// Nothing a frame reads or reports is written: not the sum, the counter banks, the spans or the stats.  An instanced scene borrows the
// frame's segment-0 queue, hit buffers and path state, which every frame writes anew before it reads them.

static int aov_channel_index(uint32_t channel) {                            // bit k of CRT_AOV_* is AovState::d_chan[k]
    for (int k = 0; k < 5; ++k) if (channel == 1u << k) return k;
    return -1;
}

int crt_render_aov(crt_scene* s, float rx, float ry, uint32_t channels, int sync) {
    if (!s) return fail(CRT_ERR_INVALID, "crt_render_aov: null scene");
    if (s->camera_rays()) return fail(CRT_ERR_INVALID, "crt_render_aov: the scene is seen along the caller's camera rays, which this call cannot follow (it looks through the pinhole): crt_clear_camera_rays first");
    if (channels == 0u || (channels & ~(uint32_t)CRT_AOV_ALL)) return fail(CRT_ERR_INVALID, "crt_render_aov: channels is a non-empty set of CRT_AOV_* bits");
    if (!s->have_camera) return fail(CRT_ERR_INVALID, "crt_render_aov: crt_set_camera was never called");
    if (s->accel != 0u) return fail(CRT_ERR_INVALID, "crt_render_aov: the feature buffers come from the CWBVH walk (option accel is 0): the BVH2 walk has another tie rule");
    int rc = require_single_device(s, "crt_render_aov");
    if (rc) return rc;
    HIPCHK(hipSetDevice(s->device));
    if (!s->aov) {
        s->aov = new (std::nothrow) AovState;
        if (!s->aov) return fail(CRT_ERR_NOMEM, "crt_render_aov: out of host memory");
    }
    AovState* const av = s->aov;
    const size_t n_pixels = (size_t)s->width * s->height;
    if (n_pixels >= (1ull << 31)) return fail(CRT_ERR_LIMIT, "crt_render_aov: frame too large for 32-bit pixel indices");
    for (int k = 0; k < 5; ++k)
        if ((channels >> k & 1u) && !av->d_chan[k]) {
            float4* p = nullptr;
            if ((rc = dev_alloc(&p, n_pixels))) return rc;
            av->d_chan[k] = p;
        }
    const crt::AovOut out = aov_channels(av);
    if (s->inst) {
        if ((rc = ensure_frame(s))) return rc;
        if ((rc = crt::ensure_queue_hits(s, true, true))) return rc;
        if (!av->d_count && (rc = dev_alloc(&av->d_count, 8 * kCounterStride))) return rc;
    } else if (!av->d_tile_xy || av->rank != s->shard_rank || av->world != s->shard_world || av->tile != s->tile) {
        // the caller's shard, dealt as crt_set_shard deals it
        std::vector<uint2> tiles;
        try { crt::deal_tiles(s->width, s->height, s->tile, s->shard_rank, s->shard_world, tiles, nullptr); }
        catch (const std::exception&) { return fail(CRT_ERR_NOMEM, "crt_render_aov: out of host memory (tile list)"); }
        const uint64_t px = (uint64_t)tiles.size() * s->tile * s->tile;
        if (px >= (1ull << 31)) return fail(CRT_ERR_LIMIT, "crt_render_aov: shard too large for 32-bit pixel indices");
        HIPCHK(hipStreamSynchronize(s->stream));                          // an earlier call may still read the old list
        if (av->d_tile_xy) { (void)hipFree(av->d_tile_xy); av->d_tile_xy = nullptr; }
        if ((rc = dev_alloc(&av->d_tile_xy, tiles.size()))) return rc;
        if (!tiles.empty()) HIPCHK(hipMemcpy(av->d_tile_xy, tiles.data(), tiles.size() * sizeof(uint2), hipMemcpyHostToDevice));
        av->n_local_pixels = (uint32_t)px; av->rank = s->shard_rank; av->world = s->shard_world; av->tile = s->tile;
    }
    crt::launch_aov_fill(out, channels, (uint32_t)n_pixels, s->stream);
    if (s->inst) {
        if (s->n_local_pixels) {
            crt::InstancesView v{};
            crt::instances_view(s->inst, &v);
            const bool masked = s->instance_masks != 0u;
            if (masked && (rc = crt::instances_child_masks_for(s->inst, s->stream, &s->cmask_seen))) return rc;
            HIPCHK(hipMemsetAsync(av->d_count, 0, 8 * kCounterStride * sizeof(uint32_t), s->stream));
            const crt::RaygenArgs ra = crt::raygen_args(s, frame_args(s, rx, ry), s->d_rays[0], av->d_count, false);      // the frames' counter banks stay as the last frame left them
            crt::launch_raygen(ra, s->stream);
            crt::launch_closest_instances_queue(crt::inst_queue_args(s, v, s->d_rays[0], av->d_count, s->mask_primary, nullptr), false, masked, s->stream);
            crt::InstAovArgs a{};
            a.triangles = s->d_triangles; a.normals = s->d_normals; a.materials = s->d_materials;
            a.texcoords = s->d_texcoords; a.textures = s->d_textures;
            a.tex_width = s->tex_width; a.tex_height = s->tex_height; a.n_textures = s->n_textures;
            a.f = ra.f;
            a.sub_capacity = s->sub_capacity;
            a.rays_in = s->d_rays[0]; a.count_in = av->d_count; a.hits_in = s->d_qhits;
            a.hit_inst = s->d_qinst; a.inst_w2o = v.w2o; a.inst_mesh = v.mesh_of; a.mesh_base = s->d_mesh_base;
            a.channels = channels; a.out = out;
            crt::launch_aov_instanced(a, s->stream);
        }
    } else if (av->n_local_pixels) {
        crt::AovArgs a{};
        a.nodes = s->d_nodes; a.tris = s->d_tris; a.triangles = s->d_triangles; a.normals = s->d_normals; a.materials = s->d_materials;
        a.stack_entries = s->stack_entries;
        a.texcoords = s->d_texcoords; a.textures = s->d_textures;
        a.tex_width = s->tex_width; a.tex_height = s->tex_height; a.n_textures = s->n_textures;
        a.f = frame_args(s, rx, ry);
        a.f.tile_xy = av->d_tile_xy; a.f.tile_order = nullptr; a.f.n_local_pixels = av->n_local_pixels;
        a.overflow = s->d_overflow;
        a.channels = channels; a.out = out;
        crt::launch_aov(a, s->stream);
    }
    HIPCHK(hipGetLastError());
    av->rendered |= channels;
    av->last = channels;
    if (channels & CRT_AOV_HIT) {                                         // the view crt_temporal reprojects from
        const crt::FrameArgs f = frame_args(s, rx, ry);
        for (int k = 0; k < 3; ++k) {
            s->aov_view.pos[k] = f.cam_pos[k]; s->aov_view.right[k] = f.cam_right[k];
            s->aov_view.up[k] = f.cam_up[k]; s->aov_view.fwd[k] = f.cam_forward[k];
        }
        s->aov_view.aspect_tan = f.aspect_tan; s->aov_view.tan_fov = f.tan_fov; s->aov_view.rv = f.rv; s->aov_view.jitter = f.jitter;
        s->have_aov_view = true;
    }
    if (sync) HIPCHK(hipStreamSynchronize(s->stream));
    return CRT_OK;
}

static int aov_channel_of(crt_scene* s, uint32_t channel, const char* who, void** d_ptr) {
    const int k = aov_channel_index(channel);
    if (k < 0) return fail(CRT_ERR_INVALID, std::string(who) + ": channel is ONE of the CRT_AOV_* bits");
    if (!s->aov || !(s->aov->rendered & channel) || !s->aov->d_chan[k]) return fail(CRT_ERR_INVALID, std::string(who) + ": no crt_render_aov call has rendered this channel");
    *d_ptr = s->aov->d_chan[k];
    return CRT_OK;
}

int crt_read_aov(crt_scene* s, uint32_t channel, void* dst, size_t n_bytes) {
    if (!s || !dst) return fail(CRT_ERR_INVALID, "crt_read_aov: null argument");
    void* d = nullptr;
    const int rc = aov_channel_of(s, channel, "crt_read_aov", &d);
    if (rc) return rc;
    if (n_bytes != (size_t)s->width * s->height * 16u) return fail(CRT_ERR_INVALID, "crt_read_aov: n_bytes must be width*height*16");
    HIPCHK(hipSetDevice(s->device));
    return copy_and_sync(s, dst, d, n_bytes);
}

int crt_aov_device(crt_scene* s, uint32_t channel, const void** d_ptr) {
    if (!s || !d_ptr) return fail(CRT_ERR_INVALID, "crt_aov_device: null argument");
    *d_ptr = nullptr;
    void* d = nullptr;
    const int rc = aov_channel_of(s, channel, "crt_aov_device", &d);
    if (rc) return rc;
    HIPCHK(hipSetDevice(s->device));
    return sync_and_expose<void>(s, d, d_ptr);
}

// ---------------------------------------------------------------- crt_denoise --
// An edge-avoiding a-trous filter over the un-tiled sum, guided by the feature buffers (kernels in denoise.hip): enqueued
// on the scene's stream behind whatever frames and crt_render_aov calls are queued there.  It reads the sum and four AOV channels and
// writes only DenoiseState's buffers (and d_linear, which every crt_read_sum / crt_sum_device writes anew).

int crt_denoise(crt_scene* s, float inv_count, const crt_denoise_params* params, int sync) {
    if (!s) return fail(CRT_ERR_INVALID, "crt_denoise: null scene");
    if (s->camera_rays()) return fail(CRT_ERR_INVALID, "crt_denoise: the scene is seen along the caller's camera rays, which this call cannot follow (it looks through the pinhole): crt_clear_camera_rays first");
    crt_denoise_params p{};
    if (params) p = *params;
    else { p.passes = 5; p.flags = CRT_DENOISE_DEMODULATE; p.sigma_color = 4.0f; p.sigma_depth = 0.05f; p.normal_power_log2 = 7; }
    if (!std::isfinite(inv_count) || !(inv_count > 0.f)) return fail(CRT_ERR_INVALID, "crt_denoise: inv_count must be finite and > 0");
    if (p.passes < 1u || p.passes > 6u) return fail(CRT_ERR_INVALID, "crt_denoise: passes must be 1..6");
    if (p.flags & ~(uint32_t)CRT_DENOISE_DEMODULATE) return fail(CRT_ERR_INVALID, "crt_denoise: unknown flag bits");
    if (p.reserved[0] | p.reserved[1] | p.reserved[2]) return fail(CRT_ERR_INVALID, "crt_denoise: reserved words must be 0");
    if (p.sigma_color != 0.f && !(std::isfinite(p.sigma_color) && p.sigma_color >= 1e-6f && p.sigma_color <= 1e6f))
        return fail(CRT_ERR_INVALID, "crt_denoise: sigma_color must be 0 (no colour term) or finite and in [1e-6, 1e6]");
    int rc = check_sigma_depth(p.sigma_depth, "crt_denoise");
    if (rc) return rc;
    if (p.normal_power_log2 > 10u) return fail(CRT_ERR_INVALID, "crt_denoise: normal_power_log2 must be 0..10");
    const uint32_t need = CRT_AOV_HIT | CRT_AOV_IDS | CRT_AOV_NORMAL | CRT_AOV_ALBEDO;
    if (!s->aov || (s->aov->rendered & need) != need)
        return fail(CRT_ERR_INVALID, "crt_denoise: crt_render_aov must have rendered the HIT, IDS, NORMAL and ALBEDO channels");
    if (s->shard_world > 1u) return fail(CRT_ERR_INVALID, "crt_denoise: a shard of a frame (crt_set_shard with world > 1) lacks its neighbours' pixels");
    if ((rc = require_single_device(s, "crt_denoise"))) return rc;
    if ((rc = crt::require_device())) return rc;
    HIPCHK(hipSetDevice(s->device));
    const size_t n_pixels = (size_t)s->width * s->height;
    if (n_pixels >= (1ull << 31) / 3u) return fail(CRT_ERR_LIMIT, "crt_denoise: frame too large for 32-bit indices");
    if ((rc = ensure_frame(s))) return rc;
    if (!s->denoise) {
        s->denoise = new (std::nothrow) DenoiseState;
        if (!s->denoise) return fail(CRT_ERR_NOMEM, "crt_denoise: out of host memory");
    }
    DenoiseState* const dn = s->denoise;
    if (!dn->d_g && (rc = dev_alloc(&dn->d_g, n_pixels))) return rc;
    if (!dn->d_x[0] && (rc = dev_alloc(&dn->d_x[0], n_pixels))) return rc;
    if (!dn->d_x[1] && (rc = dev_alloc(&dn->d_x[1], n_pixels))) return rc;
    if (!dn->d_out && (rc = dev_alloc(&dn->d_out, 3 * n_pixels))) return rc;
    if ((rc = untile_to_linear(s))) return rc;
    const uint32_t demodulate = (p.flags & CRT_DENOISE_DEMODULATE) ? 1u : 0u;
    const crt::AovOut guide = aov_channels(s->aov);
    crt::DenoisePrepareArgs pa{};
    pa.sum = s->d_linear;
    pa.hit = guide.hit; pa.ids = guide.ids; pa.normal = guide.normal; pa.albedo = guide.albedo;
    pa.g = dn->d_g; pa.x = dn->d_x[0];
    pa.n_pixels = (uint32_t)n_pixels; pa.inv_count = inv_count; pa.demodulate = demodulate;
    crt::launch_denoise_prepare(pa, s->stream);
    float sigma = p.sigma_color;
    for (uint32_t i = 0; i < p.passes; ++i) {
        crt::DenoisePassArgs a{};
        a.g = dn->d_g; a.x_in = dn->d_x[i & 1u]; a.x_out = dn->d_x[(i & 1u) ^ 1u]; a.out = dn->d_out; a.albedo = pa.albedo;
        a.width = s->width; a.height = s->height; a.step_log2 = i;
        a.use_color = p.sigma_color != 0.f ? 1u : 0u;
        a.inv_c = a.use_color ? 1.0f / (sigma * sigma) : 0.f;
        a.sigma_depth = p.sigma_depth;
        a.normal_squarings = p.normal_power_log2;
        a.demodulate = demodulate;
        crt::launch_denoise_pass(a, i + 1u == p.passes, s->denoise_form, s->stream);
        sigma = sigma * 0.5f;
    }
    HIPCHK(hipGetLastError());
    dn->valid = true;
    if (sync) HIPCHK(hipStreamSynchronize(s->stream));
    return CRT_OK;
}

int crt_read_denoised(crt_scene* s, float* rgb, size_t n_floats) { return read_image(s, denoised_image, "crt_read_denoised", rgb, n_floats); }
int crt_denoised_device(crt_scene* s, const float** d_rgb) { return expose_image(s, denoised_image, "crt_denoised_device", d_rgb); }
// the denoised image through crt_resolve's tone map and pinned gamma, into DenoiseState's own RGBA8: crt_resolve_device's stays as it is
int crt_resolve_denoised(crt_scene* s, uint8_t* rgba, size_t n_bytes) { return resolve_image_host(s, denoised_image, "crt_resolve_denoised", 1.0f, rgba, n_bytes); }
int crt_resolve_denoised_device(crt_scene* s, const uint8_t** d_rgba, int sync) { return resolve_image_device(s, denoised_image, "crt_resolve_denoised_device", 1.0f, d_rgba, sync); }

// ---------------------------------------------------------------- crt_temporal --
// Temporal accumulation by reprojection (kernel in temporal.hip): enqueued on the scene's stream behind whatever frames,
// crt_render_aov and crt_denoise calls are queued there.  It reads the source image, four AOV channels, its own previous set and an
// instanced scene's live transforms, and writes only TemporalState's buffers (and d_linear, which every crt_read_sum / crt_sum_device
// writes anew).  crt_reset never comes here: the history outlives the sum.

int crt_temporal(crt_scene* s, float inv_count, const crt_temporal_params* params, int sync) {
    if (!s) return fail(CRT_ERR_INVALID, "crt_temporal: null scene");
    if (s->camera_rays()) return fail(CRT_ERR_INVALID, "crt_temporal: the scene is seen along the caller's camera rays, which this call cannot follow (it looks through the pinhole): crt_clear_camera_rays first");
    crt_temporal_params p{};
    if (params) p = *params;
    else { p.flags = CRT_TEMPORAL_DEMODULATE; p.source = CRT_TEMPORAL_SOURCE_SUM; p.max_history = 32; p.sigma_depth = 0.1f; p.normal_min = 0.9f; }
    if (!std::isfinite(inv_count) || !(inv_count > 0.f)) return fail(CRT_ERR_INVALID, "crt_temporal: inv_count must be finite and > 0");
    if (p.flags & ~(uint32_t)(CRT_TEMPORAL_DEMODULATE | CRT_TEMPORAL_CLAMP)) return fail(CRT_ERR_INVALID, "crt_temporal: unknown flag bits");
    if (p.source > (uint32_t)CRT_TEMPORAL_SOURCE_DENOISED) return fail(CRT_ERR_INVALID, "crt_temporal: source is CRT_TEMPORAL_SOURCE_SUM or CRT_TEMPORAL_SOURCE_DENOISED");
    if (p.max_history < 1u || p.max_history > 4096u) return fail(CRT_ERR_INVALID, "crt_temporal: max_history must be 1..4096");
    int rc = check_sigma_depth(p.sigma_depth, "crt_temporal");
    if (rc) return rc;
    if (!(std::isfinite(p.normal_min) && p.normal_min >= -1.0f && p.normal_min <= 1.0f))
        return fail(CRT_ERR_INVALID, "crt_temporal: normal_min must be finite and in [-1, 1]");
    if (p.reserved[0] | p.reserved[1] | p.reserved[2]) return fail(CRT_ERR_INVALID, "crt_temporal: reserved words must be 0");
    const uint32_t demodulate = (p.flags & CRT_TEMPORAL_DEMODULATE) ? 1u : 0u;
    const uint32_t need = CRT_AOV_HIT | CRT_AOV_IDS | CRT_AOV_NORMAL | (demodulate ? (uint32_t)CRT_AOV_ALBEDO : 0u);
    if (!s->aov || (s->aov->rendered & need) != need || !s->have_aov_view)
        return fail(CRT_ERR_INVALID, "crt_temporal: crt_render_aov must have rendered the HIT, IDS and NORMAL channels, and ALBEDO for CRT_TEMPORAL_DEMODULATE");
    if (p.source == CRT_TEMPORAL_SOURCE_DENOISED && (!s->denoise || !s->denoise->valid))
        return fail(CRT_ERR_INVALID, "crt_temporal: source CRT_TEMPORAL_SOURCE_DENOISED needs a successful crt_denoise");
    if (s->shard_world > 1u) return fail(CRT_ERR_INVALID, "crt_temporal: a shard of a frame (crt_set_shard with world > 1) lacks the rest of the previous frame");
    if ((rc = require_single_device(s, "crt_temporal"))) return rc;
    if ((rc = crt::require_device())) return rc;
    HIPCHK(hipSetDevice(s->device));
    const size_t n_pixels = (size_t)s->width * s->height;
    if (n_pixels >= (1ull << 31) / 3u) return fail(CRT_ERR_LIMIT, "crt_temporal: frame too large for 32-bit indices");
    if ((rc = ensure_frame(s))) return rc;
    if (!s->temporal) {
        s->temporal = new (std::nothrow) TemporalState;
        if (!s->temporal) return fail(CRT_ERR_NOMEM, "crt_temporal: out of host memory");
    }
    TemporalState* const ts = s->temporal;
    for (int k = 0; k < 2; ++k) {
        if (!ts->d_hist[k] && (rc = dev_alloc(&ts->d_hist[k], n_pixels))) return rc;
        if (!ts->d_guide[k] && (rc = dev_alloc(&ts->d_guide[k], n_pixels))) return rc;
        if (!ts->d_key[k] && (rc = dev_alloc(&ts->d_key[k], n_pixels))) return rc;
    }
    if (!ts->d_out && (rc = dev_alloc(&ts->d_out, 3 * n_pixels))) return rc;
    crt::InstancesView v{};
    if (s->inst) {
        crt::instances_view(s->inst, &v);                                 // the live arrays, read at enqueue as a frame reads them
        if (!ts->d_o2w_prev && (rc = dev_alloc(&ts->d_o2w_prev, 12 * (size_t)std::max(v.capacity, 1u)))) return rc;
    }
    crt::TemporalArgs a{};
    if (p.source == CRT_TEMPORAL_SOURCE_SUM) {
        if ((rc = untile_to_linear(s))) return rc;
        a.src = s->d_linear; a.scale_source = 1u;
    } else {
        a.src = s->denoise->d_out; a.scale_source = 0u;
    }
    const uint32_t from = ts->cur, to = ts->cur ^ 1u;
    const crt::AovOut guide = aov_channels(s->aov);
    a.hit = guide.hit; a.ids = guide.ids; a.normal = guide.normal; a.albedo = guide.albedo;
    a.hist_in = ts->d_hist[from]; a.guide_in = ts->d_guide[from]; a.key_in = ts->d_key[from];
    a.hist_out = ts->d_hist[to]; a.guide_out = ts->d_guide[to]; a.key_out = ts->d_key[to];
    a.out = ts->d_out;
    if (s->inst) {
        a.o2w = v.o2w; a.w2o = v.w2o; a.o2w_prev = ts->d_o2w_prev;
        a.n_instances = v.n_instances; a.n_prev_instances = ts->n_prev_instances;
    }
    a.width = s->width; a.height = s->height;
    a.inv_count = inv_count;
    a.demodulate = demodulate; a.clamp = (p.flags & CRT_TEMPORAL_CLAMP) ? 1u : 0u;
    // history-less: the first call, after crt_temporal_reset, after a change of the DEMODULATE bit (the history holds the other quantity),
    // and at max_history 1, where the definition takes y = x
    a.has_history = (ts->have_history && ts->demodulate == demodulate && p.max_history > 1u) ? 1u : 0u;
    a.max_history = (float)p.max_history; a.sigma_depth = p.sigma_depth; a.normal_min = p.normal_min;
    a.cur = s->aov_view; a.prev = ts->prev_view;
    crt::launch_temporal(a, s->temporal_form, s->stream);
    HIPCHK(hipGetLastError());
    if (s->inst && v.n_instances) HIPCHK(hipMemcpyAsync(ts->d_o2w_prev, v.o2w, (size_t)v.n_instances * 48, hipMemcpyDeviceToDevice, s->stream));
    ts->n_prev_instances = s->inst ? v.n_instances : 0u;
    ts->cur = to;
    ts->prev_view = s->aov_view;
    ts->demodulate = demodulate;
    ts->have_history = true;
    ts->valid = true;
    if (sync) HIPCHK(hipStreamSynchronize(s->stream));
    return CRT_OK;
}

int crt_temporal_reset(crt_scene* s) {
    if (!s) return fail(CRT_ERR_INVALID, "crt_temporal_reset: null scene");
    if (s->temporal) s->temporal->have_history = false;
    return CRT_OK;
}

int crt_read_temporal(crt_scene* s, float* rgb, size_t n_floats) { return read_image(s, temporal_image, "crt_read_temporal", rgb, n_floats); }
int crt_temporal_device(crt_scene* s, const float** d_rgb) { return expose_image(s, temporal_image, "crt_temporal_device", d_rgb); }
// the accumulated image through crt_resolve's tone map and pinned gamma, into TemporalState's own RGBA8
int crt_resolve_temporal(crt_scene* s, uint8_t* rgba, size_t n_bytes) { return resolve_image_host(s, temporal_image, "crt_resolve_temporal", 1.0f, rgba, n_bytes); }
int crt_resolve_temporal_device(crt_scene* s, const uint8_t** d_rgba, int sync) { return resolve_image_device(s, temporal_image, "crt_resolve_temporal_device", 1.0f, d_rgba, sync); }

int crt_read_temporal_history(crt_scene* s, float* n, size_t n_floats) {
    if (!s || !n) return fail(CRT_ERR_INVALID, "crt_read_temporal_history: null argument");
    const size_t npx = (size_t)s->width * s->height;
    int rc = begin_image(s, temporal_image(s), "crt_read_temporal_history", n_floats == npx, ": n_floats must be width*height");
    if (rc) return rc;
    std::vector<float4> hist;
    try { hist.resize(npx); } catch (const std::exception&) { return fail(CRT_ERR_NOMEM, "crt_read_temporal_history: out of host memory"); }
    if ((rc = copy_and_sync(s, hist.data(), s->temporal->d_hist[s->temporal->cur], npx * sizeof(float4)))) return rc;
    for (size_t i = 0; i < npx; ++i) n[i] = hist[i].w;
    return CRT_OK;
}

// ---------------------------------------------------------------- crt_display --
// The display transform (kernels in display.hip): enqueued on the scene's stream behind whatever frames, crt_render_aov,
// crt_denoise and crt_temporal calls are queued there.  It reads the image it names and writes only DisplayState's buffers.  The exposure
// is metered, adapted and kept on the device: nothing here waits for it.

namespace {

bool finite_in(float v, float lo, float hi) { return std::isfinite(v) && v >= lo && v <= hi; }

int no_display(const char* who) { return fail(CRT_ERR_INVALID, std::string(who) + ": no crt_display call has succeeded on this scene"); }

}  // namespace

// crt_display, crt_display_bloom and crt_display_fogged: one body, `input` names the image (a stage's in place of the one params.source names)
enum class DisplayInput { SOURCE, BLOOMED, FOGGED };
static int display_call(crt_scene* s, const char* who, DisplayInput input, float inv_count, const crt_display_params* params, int sync) {
    const auto bad = [who](const char* what) { return fail(CRT_ERR_INVALID, std::string(who) + what); };
    if (!s) return bad(": null scene");
    crt_display_params p{};
    if (params) p = *params;
    else {
        p.source = CRT_DISPLAY_SOURCE_SUM; p.curve = CRT_DISPLAY_CURVE_REFERENCE; p.flags = 0u;
        p.exposure = 1.0f; p.white = 4.0f; p.key = 0.18f; p.adapt = 1.0f; p.exposure_min = 1e-6f; p.exposure_max = 1e6f;
        p.low_permille = 0u; p.high_permille = 1000u;
    }
    if (!std::isfinite(inv_count) || !(inv_count > 0.f)) return bad(": inv_count must be finite and > 0");
    if (input == DisplayInput::BLOOMED && p.source != 0u) return bad(": source must be 0 (the image is crt_bloom's)");
    if (input == DisplayInput::FOGGED && p.source != 0u) return bad(": source must be 0 (the image is crt_fog_composite's)");
    if (p.source > (uint32_t)CRT_DISPLAY_SOURCE_TEMPORAL) return bad(": source is CRT_DISPLAY_SOURCE_SUM, _DENOISED or _TEMPORAL");
    if (p.curve > (uint32_t)CRT_DISPLAY_CURVE_CLAMP) return bad(": curve is CRT_DISPLAY_CURVE_REFERENCE, _REINHARD, _ACES or _CLAMP");
    if (p.flags & ~(uint32_t)CRT_DISPLAY_AUTO_EXPOSURE) return bad(": unknown flag bits");
    if (p.reserved) return bad(": reserved must be 0");
    if (!finite_in(p.exposure, 1e-9f, 1e9f)) return bad(": exposure must be finite and in [1e-9, 1e9]");
    if (!finite_in(p.white, 1e-3f, 1e6f)) return bad(": white must be finite and in [1e-3, 1e6]");
    const bool metered = (p.flags & CRT_DISPLAY_AUTO_EXPOSURE) != 0u;
    if (metered) {
        if (!finite_in(p.key, 1e-6f, 1e6f)) return bad(": key must be finite and in [1e-6, 1e6]");
        if (!(std::isfinite(p.adapt) && p.adapt > 0.f && p.adapt <= 1.0f)) return bad(": adapt must be finite and in (0, 1]");
        if (!finite_in(p.exposure_min, 1e-9f, 1e9f)) return bad(": exposure_min must be finite and in [1e-9, 1e9]");
        if (!finite_in(p.exposure_max, 1e-9f, 1e9f)) return bad(": exposure_max must be finite and in [1e-9, 1e9]");
        if (p.exposure_min > p.exposure_max) return bad(": exposure_min must not exceed exposure_max");
        if (p.high_permille > 1000u) return bad(": high_permille must be at most 1000");
        if (p.low_permille >= p.high_permille) return bad(": low_permille must be below high_permille");
    }
    const Image im = input == DisplayInput::BLOOMED ? bloom_image(s) : input == DisplayInput::FOGGED ? fogged_image(s) : p.source == CRT_DISPLAY_SOURCE_SUM ? sum_image(s) : p.source == CRT_DISPLAY_SOURCE_DENOISED ? denoised_image(s) : temporal_image(s);
    int rc = begin_image(s, im, who);
    if (rc) return rc;
    const size_t npx = (size_t)s->width * s->height;
    if (npx >= (1ull << 31)) return fail(CRT_ERR_LIMIT, std::string(who) + ": frame too large for 32-bit pixel indices");
    if (im.packed && (rc = ensure_frame(s))) return rc;
    if (!s->display) {
        s->display = new (std::nothrow) DisplayState;
        if (!s->display) return fail(CRT_ERR_NOMEM, std::string(who) + ": out of host memory");
    }
    DisplayState* const ds = s->display;
    if (!ds->d_rgba && (rc = dev_alloc(&ds->d_rgba, 4 * npx))) return rc;
    if (!ds->d_words) {
        const size_t n_words = crt::kDisplayWords;
        if ((rc = dev_alloc(&ds->d_words, n_words))) return rc;
        HIPCHK(hipMemsetAsync(ds->d_words, 0, n_words * sizeof(uint32_t), s->stream));
    }
    if ((rc = ensure_gamma(s))) return rc;

    // the image's slices: the packed tile buffers of this scene and its peers as gathered, or the one linear image
    std::vector<crt::DisplaySlice> slices;
    try { slices.reserve(1 + s->peers.size()); } catch (const std::exception&) { return fail(CRT_ERR_NOMEM, std::string(who) + ": out of host memory"); }
    if (im.packed) {
        rc = for_each_slice(s, [&slices](const crt::FrameArgs& f, const float* packed, uint32_t grid) {
            crt::DisplaySlice sl{};
            sl.f = f; sl.image = packed; sl.packed = 1u; sl.grid = grid;
            slices.push_back(sl);
        });
        if (rc) return rc;
    } else {
        crt::DisplaySlice sl{};
        sl.image = *im.rgb; sl.n_pixels = (uint32_t)npx; sl.grid = s->flat_grid(npx);
        slices.push_back(sl);
    }

    if (metered) for (const crt::DisplaySlice& sl : slices) crt::launch_display_hist(sl, inv_count, (ds->d_words + crt::kDisplayBinsAt), s->stream);
    crt::DisplayMeterArgs m{};
    m.bins = (ds->d_words + crt::kDisplayBinsAt); m.last = (ds->d_words + crt::kDisplayLastAt); m.state = ds->d_words;
    m.metered = metered ? 1u : 0u;
    m.exposure = p.exposure; m.key = p.key; m.adapt = p.adapt; m.exposure_min = p.exposure_min; m.exposure_max = p.exposure_max;
    m.low_permille = p.low_permille; m.high_permille = p.high_permille;
    crt::launch_display_meter(m, s->stream);
    // a shard of a frame (crt_set_shard with world > 1) leaves the other ranks' pixels at 0
    if (im.packed && s->shard_world > 1u) HIPCHK(hipMemsetAsync(ds->d_rgba, 0, 4 * npx, s->stream));
    const float w2 = p.white * p.white;
    for (const crt::DisplaySlice& sl : slices) crt::launch_display(sl, inv_count, p.curve, w2, ds->d_words, s->d_gamma, ds->d_rgba, s->stream);
    HIPCHK(hipGetLastError());
    ds->valid = true;
    if (metered) ds->metered = true;
    if (sync) HIPCHK(hipStreamSynchronize(s->stream));
    return CRT_OK;
}

int crt_display(crt_scene* s, float inv_count, const crt_display_params* params, int sync) { return display_call(s, "crt_display", DisplayInput::SOURCE, inv_count, params, sync); }
// the bloomed image is a mean: there is no inv_count
int crt_display_bloom(crt_scene* s, const crt_display_params* params, int sync) { return display_call(s, "crt_display_bloom", DisplayInput::BLOOMED, 1.0f, params, sync); }
// so is the fogged image
int crt_display_fogged(crt_scene* s, const crt_display_params* params, int sync) { return display_call(s, "crt_display_fogged", DisplayInput::FOGGED, 1.0f, params, sync); }

int crt_read_display(crt_scene* s, uint8_t* rgba, size_t n_bytes) {
    if (!s || !rgba) return null_argument("crt_read_display");
    if (!s->display || !s->display->valid) return no_display("crt_read_display");
    if (n_bytes != 4 * (size_t)s->width * s->height) return fail(CRT_ERR_INVALID, "crt_read_display: n_bytes must be width*height*4");
    HIPCHK(hipSetDevice(s->device));
    return copy_and_sync(s, rgba, s->display->d_rgba, n_bytes);
}

int crt_display_device(crt_scene* s, const uint8_t** d_rgba) {
    if (!s || !d_rgba) return null_argument("crt_display_device");
    *d_rgba = nullptr;
    if (!s->display || !s->display->valid) return no_display("crt_display_device");
    HIPCHK(hipSetDevice(s->device));
    return sync_and_expose<uint8_t>(s, s->display->d_rgba, d_rgba);
}

int crt_display_get_state(crt_scene* s, crt_display_state* out) {
    if (!s || !out) return null_argument("crt_display_get_state");
    if (!s->display || !s->display->valid) return no_display("crt_display_get_state");
    HIPCHK(hipSetDevice(s->device));
    uint32_t w[crt::kDisplayStateWords];
    const int rc = copy_and_sync(s, w, s->display->d_words, sizeof w);
    if (rc) return rc;
    std::memset(out, 0, sizeof *out);
    std::memcpy(&out->exposure, &w[crt::kDisplayExposure], 4);
    std::memcpy(&out->metered, &w[crt::kDisplayMetered], 4);
    out->counted = w[crt::kDisplayCounted]; out->q = w[crt::kDisplayQ]; out->calls = w[crt::kDisplayCalls];
    return CRT_OK;
}

int crt_read_display_histogram(crt_scene* s, uint32_t hist[256]) {
    if (!s || !hist) return null_argument("crt_read_display_histogram");
    if (!s->display || !s->display->valid) return no_display("crt_read_display_histogram");
    if (!s->display->metered) return fail(CRT_ERR_INVALID, "crt_read_display_histogram: no crt_display call with CRT_DISPLAY_AUTO_EXPOSURE has metered on this scene");
    HIPCHK(hipSetDevice(s->device));
    return copy_and_sync(s, hist, (s->display->d_words + crt::kDisplayLastAt), 256 * sizeof(uint32_t));
}

// in stream order: a queued crt_display still adapts from what it had
int crt_display_reset(crt_scene* s) {
    if (!s) return fail(CRT_ERR_INVALID, "crt_display_reset: null scene");
    if (!s->display || !s->display->d_words) return CRT_OK;
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipMemsetAsync(s->display->d_words + crt::kDisplayCalls, 0, sizeof(uint32_t), s->stream));
    return CRT_OK;
}

// ---------------------------------------------------------------- crt_bloom --
// Bloom (kernels in bloom.hip): enqueued on the scene's stream behind whatever frames, crt_render_aov, crt_denoise and
// crt_temporal calls are queued there.  It reads the image it names and writes only BloomState's buffers (and d_linear, which every
// crt_read_sum / crt_sum_device writes anew).

namespace {

// level k of the pyramid of a w x h frame: its size, and where its floats begin in BloomState::d_pyramid (level 1 at 0)
struct BloomLevels {
    uint32_t w[crt::kBloomMaxLevels + 1], h[crt::kBloomMaxLevels + 1];
    size_t at[crt::kBloomMaxLevels + 2];
    uint32_t n;                                            // levels the frame has, at most `levels`
    BloomLevels(uint32_t width, uint32_t height, uint32_t levels) {
        w[0] = width; h[0] = height; at[0] = at[1] = 0; n = 0;
        for (uint32_t k = 1; k <= crt::kBloomMaxLevels; ++k) {
            const bool has = n == k - 1u && k <= levels && std::min(w[k - 1], h[k - 1]) >= 2u;
            w[k] = has ? (w[k - 1] + 1u) >> 1 : 0u; h[k] = has ? (h[k - 1] + 1u) >> 1 : 0u;
            at[k + 1] = at[k] + 3 * (size_t)w[k] * h[k];
            if (has) n = k;
        }
    }
    size_t floats(uint32_t from, uint32_t to) const { return at[to + 1] - at[from]; }     // of levels from .. to
};

}  // namespace

int crt_bloom(crt_scene* s, float inv_count, const crt_bloom_params* params, int sync) {
    if (!s) return fail(CRT_ERR_INVALID, "crt_bloom: null scene");
    crt_bloom_params p{};
    if (params) p = *params;
    else { p.source = CRT_BLOOM_SOURCE_SUM; p.levels = 6; p.flags = CRT_BLOOM_CONSERVE; p.threshold = 0.0f; p.clamp = 0.0f; p.scatter = 0.7f; p.strength = 0.05f; }
    if (!std::isfinite(inv_count) || !(inv_count > 0.f)) return fail(CRT_ERR_INVALID, "crt_bloom: inv_count must be finite and > 0");
    if (p.source > (uint32_t)CRT_BLOOM_SOURCE_TEMPORAL) return fail(CRT_ERR_INVALID, "crt_bloom: source is CRT_BLOOM_SOURCE_SUM, _DENOISED or _TEMPORAL");
    if (p.flags & ~(uint32_t)CRT_BLOOM_CONSERVE) return fail(CRT_ERR_INVALID, "crt_bloom: unknown flag bits");
    if (p.levels < 1u || p.levels > crt::kBloomMaxLevels) return fail(CRT_ERR_INVALID, "crt_bloom: levels must be 1..8");
    if (p.reserved) return fail(CRT_ERR_INVALID, "crt_bloom: reserved must be 0");
    if (!finite_in(p.threshold, 0.0f, 1e6f)) return fail(CRT_ERR_INVALID, "crt_bloom: threshold must be finite and in [0, 1e6]");
    if (p.clamp != 0.0f && !finite_in(p.clamp, 1e-6f, 1e9f)) return fail(CRT_ERR_INVALID, "crt_bloom: clamp must be 0 (none) or finite and in [1e-6, 1e9]");
    if (!finite_in(p.scatter, 0.0f, 1.0f)) return fail(CRT_ERR_INVALID, "crt_bloom: scatter must be finite and in [0, 1]");
    const bool conserve = (p.flags & CRT_BLOOM_CONSERVE) != 0u;
    if (!finite_in(p.strength, 0.0f, conserve ? 1.0f : 1e3f))
        return fail(CRT_ERR_INVALID, conserve ? "crt_bloom: strength must be finite and in [0, 1] with CRT_BLOOM_CONSERVE" : "crt_bloom: strength must be finite and in [0, 1e3]");
    if (s->shard_world > 1u) return fail(CRT_ERR_INVALID, "crt_bloom: a shard of a frame (crt_set_shard with world > 1) lacks its neighbours' pixels");
    const Image im = p.source == CRT_BLOOM_SOURCE_SUM ? sum_image(s) : p.source == CRT_BLOOM_SOURCE_DENOISED ? denoised_image(s) : temporal_image(s);
    int rc = begin_image(s, im, "crt_bloom");
    if (rc) return rc;
    const size_t npx = (size_t)s->width * s->height;
    if (npx >= (1ull << 31) / 3u) return fail(CRT_ERR_LIMIT, "crt_bloom: frame too large for 32-bit indices");
    if (im.packed && (rc = ensure_frame(s))) return rc;
    if (!s->bloom) {
        s->bloom = new (std::nothrow) BloomState;
        if (!s->bloom) return fail(CRT_ERR_NOMEM, "crt_bloom: out of host memory");
    }
    BloomState* const bl = s->bloom;
    // sized for every level the frame can have, whatever this call asks for
    if (!bl->d_pyramid && (rc = dev_alloc(&bl->d_pyramid, std::max<size_t>(BloomLevels(s->width, s->height, crt::kBloomMaxLevels).floats(1, crt::kBloomMaxLevels), 1)))) return rc;
    if (!bl->d_out && (rc = dev_alloc(&bl->d_out, 3 * npx))) return rc;
    if (!bl->d_rgba && (rc = dev_alloc(&bl->d_rgba, 4 * npx))) return rc;
    if (im.packed && (rc = untile_to_linear(s))) return rc;

    crt::BloomSource src{};
    src.image = *im.rgb; src.width = s->width; src.height = s->height;
    src.scale = im.packed ? 1u : 0u; src.inv_count = inv_count;
    src.threshold = p.threshold; src.clamp = p.clamp;
    const BloomLevels lv(s->width, s->height, p.levels);
    const uint32_t n = lv.n;
    if (n == 0u) crt::launch_bloom_copy(src, bl->d_out, s->stream);
    else {
        float* const D = bl->d_pyramid;
        // a launch per step: the forms that took several small levels per launch, or Down through LDS tiles, measured slower
        crt::launch_bloom_down_first(src, D + lv.at[1], s->stream);
        for (uint32_t k = 2; k <= n; ++k) crt::launch_bloom_down(D + lv.at[k - 1], lv.w[k - 1], lv.h[k - 1], D + lv.at[k], s->stream);
        for (uint32_t k = n - 1u; k >= 1u; --k) crt::launch_bloom_up(D + lv.at[k + 1], D + lv.at[k], lv.w[k], lv.h[k], p.scatter, s->stream);
        crt::launch_bloom_composite(src, D + lv.at[1], conserve ? 1u : 0u, p.strength, bl->d_out, s->stream);
    }
    HIPCHK(hipGetLastError());
    bl->valid = true;
    if (sync) HIPCHK(hipStreamSynchronize(s->stream));
    return CRT_OK;
}

int crt_read_bloom(crt_scene* s, float* rgb, size_t n_floats) { return read_image(s, bloom_image, "crt_read_bloom", rgb, n_floats); }
int crt_bloom_device(crt_scene* s, const float** d_rgb) { return expose_image(s, bloom_image, "crt_bloom_device", d_rgb); }
// the bloomed image through crt_resolve's tone map and pinned gamma, into BloomState's own RGBA8
int crt_resolve_bloom(crt_scene* s, uint8_t* rgba, size_t n_bytes) { return resolve_image_host(s, bloom_image, "crt_resolve_bloom", 1.0f, rgba, n_bytes); }
int crt_resolve_bloom_device(crt_scene* s, const uint8_t** d_rgba, int sync) { return resolve_image_device(s, bloom_image, "crt_resolve_bloom_device", 1.0f, d_rgba, sync); }

// ---------------------------------------------------------------- crt_fog_composite --
// The fog of the view put on an image (k_fog_composite in rt_kernels.hip): enqueued on the scene's stream like crt_bloom.  It
// reads the image it names and crt_render_fog's, and writes only the fogged image (and d_linear, which every crt_read_sum writes anew).

int crt_fog_composite(crt_scene* s, float inv_count, uint32_t source, int sync) {
    if (!s) return fail(CRT_ERR_INVALID, "crt_fog_composite: null scene");
    if (!std::isfinite(inv_count) || !(inv_count > 0.f)) return fail(CRT_ERR_INVALID, "crt_fog_composite: inv_count must be finite and > 0");
    if (source > (uint32_t)CRT_DISPLAY_SOURCE_TEMPORAL) return fail(CRT_ERR_INVALID, "crt_fog_composite: source is CRT_DISPLAY_SOURCE_SUM, _DENOISED or _TEMPORAL");
    if (s->shard_world > 1u) return fail(CRT_ERR_INVALID, "crt_fog_composite: a whole frame only (crt_set_shard has world > 1)");
    if (s->primary || !s->peers.empty()) return fail(CRT_ERR_INVALID, "crt_fog_composite: a scene on one device and one stream only (crt_set_devices / option streams have dealt this one's tiles)");
    FogState* const fg = s->fog;
    if (!fg || !fg->rendered) return fail(CRT_ERR_INVALID, "crt_fog_composite: no crt_render_fog call has succeeded on this scene");
    const Image im = source == CRT_DISPLAY_SOURCE_SUM ? sum_image(s) : source == CRT_DISPLAY_SOURCE_DENOISED ? denoised_image(s) : temporal_image(s);
    int rc = begin_image(s, im, "crt_fog_composite");
    if (rc) return rc;
    const size_t npx = (size_t)s->width * s->height;
    if (npx >= (1ull << 31) / 3u) return fail(CRT_ERR_LIMIT, "crt_fog_composite: frame too large for 32-bit indices");
    if (im.packed && (rc = ensure_frame(s))) return rc;
    if (!fg->d_fogged && (rc = dev_alloc(&fg->d_fogged, 3 * npx))) return rc;
    if (im.packed && (rc = untile_to_linear(s))) return rc;
    crt::FogCompositeArgs a{};
    a.image = *im.rgb; a.fog = fg->d_image; a.out = fg->d_fogged; a.n_pixels = (uint32_t)npx;
    a.scale = im.packed ? 1u : 0u; a.inv_count = inv_count;
    crt::launch_fog_composite(a, s->stream);
    HIPCHK(hipGetLastError());
    fg->composited = true;
    if (sync) HIPCHK(hipStreamSynchronize(s->stream));
    return CRT_OK;
}

int crt_read_fogged(crt_scene* s, float* rgb, size_t n_floats) { return read_image(s, fogged_image, "crt_read_fogged", rgb, n_floats); }
int crt_fogged_device(crt_scene* s, const float** d_rgb) { return expose_image(s, fogged_image, "crt_fogged_device", d_rgb); }
