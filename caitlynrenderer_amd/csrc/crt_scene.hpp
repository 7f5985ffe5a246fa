// struct crt_scene and the state structs it points to, shared by the translation units behind the device half of include/crt.h:
// crt_create.cpp (creation), crt_device.cpp (options, several GPUs, refit / rebuild), crt_frames.cpp (frame dispatch) and crt_outputs.cpp
// (everything that leaves as an image).
// Private to csrc/: not installed, include/crt.h knows crt_scene by name only, and nothing declared here is exported by the library.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "../../include/crt.h"
#include "crt_error.hpp"
#include "device_build.hpp"
#include "host/refit_core.hpp"
#include "instances_bind.hpp"
#include "rt_kernels.hpp"
#include "temporal.hpp"

#pragma GCC visibility push(hidden)

#define HIPCHK(expr)                                                                             \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return crt::fail(CRT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));    \
    } while (0)

constexpr uint32_t kCounterStride = 32;                        // == CRT_COUNTER_STRIDE in rt_kernels.hip (128 B)
// kind 0 = rays into the segment, 1 = its shadow rays
constexpr uint32_t kQueueCounters = 2 * 17 * 8 * kCounterStride;    // (segment, kind, group) x stride
inline uint32_t counter_index(uint32_t seg, uint32_t kind, uint32_t group) { return ((seg * 2 + kind) * 8 + group) * kCounterStride; }
// behind them, in the same banks (cleared with them): the cursors of the persistent grids (rt_kernels.hip PoolStream) — one per sub-queue of
// a segment's path-ray queue (k_closest_queue), one per (region, sub-queue) of the frame's NEE queue (k_shadow_deferred)
inline uint32_t cursor_index_closest(uint32_t seg) { return kQueueCounters + seg * 8 * kCounterStride; }
constexpr uint32_t kCursorShadow = kQueueCounters + 17 * 8 * kCounterStride;
constexpr uint32_t kCounters = kCursorShadow + 17 * 8 * kCounterStride;

struct EventSpan { hipEvent_t a = nullptr, b = nullptr; int kind = 0; };   // kind: 0 raygen 1 closest 2 any 3 shade/other

// What segment 0 of the last chain of launches ran (crt_debug_launch_form, crt_debug_launch_info).  form: how its samples sat on the hardware
// (option "wave_samples").  build: bit 0 the 6-wave build, 1 a build without the sample loop, 2 one compiled as the path's last segment
// (option "last_build"), 3 its LEAN form (option "lean_build"), 4 segment 0 was fed by the lens ray generator, 5 the frame ran k_env_miss
// behind its closest-hit launches, 6 segment 0 was fed by the caller's camera rays (k_raygen_rays).  samples: samples per pixel of the chain.
struct LaunchInfo { int form = 0, build = 0, samples = 1; };

// What crt_render_aov keeps, allocated by a scene's first call: the five channel buffers, each by the first call that asks
// for it, and what the dispatch needs beside the frame's own buffers.  The scene's stream has drained when this is destroyed.
struct AovState {
    void* d_chan[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // HIT, IDS, NORMAL, ALBEDO, EMISSION: width * height * 16 bytes, linear pixel order
    uint32_t rendered = 0;               // channels some call has written
    uint32_t last = 0;                   // the channels of the last call
    // flat scenes: the tiles of the CALLER's shard (crt_set_shard), whatever option "streams" made of them for the frames
    uint2* d_tile_xy = nullptr;
    uint32_t n_local_pixels = 0, rank = 0, world = 0, tile = 0;
    uint32_t* d_count = nullptr;         // instanced scenes: the 8 counters of the primary rays' queue (the frames' banks stay as they are)
    ~AovState() {
        for (void* p : d_chan) if (p) (void)hipFree(p);
        if (d_tile_xy) (void)hipFree(d_tile_xy);
        if (d_count) (void)hipFree(d_count);
    }
};

// What crt_denoise keeps, allocated by a scene's first call: the guide records, the two images the passes alternate
// between, the denoised linear image and its RGBA8.  A scene that never denoises holds none of it.
struct DenoiseState {
    float4* d_g = nullptr;               // (unit normal, t) per pixel, constant over the passes
    float4* d_x[2] = {nullptr, nullptr}; // (x, key) per pixel: pass i reads [i & 1] and writes the other
    float* d_out = nullptr;              // the denoised MEAN radiance, 3 floats per pixel, linear pixel order
    uint8_t* d_rgba = nullptr;           // crt_resolve_denoised*'s buffer, from their first call on
    bool valid = false;                  // some crt_denoise has been enqueued
    ~DenoiseState() {
        void* bufs[] = {d_g, d_x[0], d_x[1], d_out, d_rgba};
        for (void* p : bufs) if (p) (void)hipFree(p);
    }
};

// What crt_temporal keeps, allocated by a scene's first call: two sets of (history, guide, key) that the calls alternate
// between, the accumulated linear image and its RGBA8, the previous call's view and, for an instanced scene, its object_to_world.
struct TemporalState {
    float4* d_hist[2] = {nullptr, nullptr};      // (y, N) per pixel: a call reads [cur] and writes the other
    float4* d_guide[2] = {nullptr, nullptr};     // (unit normal, t) per pixel
    uint32_t* d_key[2] = {nullptr, nullptr};     // instance + 1, 0 for a pixel that is not filterable
    float* d_out = nullptr;                      // the accumulated MEAN radiance, 3 floats per pixel, linear pixel order
    uint8_t* d_rgba = nullptr;                   // crt_resolve_temporal*'s buffer, from their first call on
    float* d_o2w_prev = nullptr;                 // an instanced scene: object_to_world as of the previous call (capacity x 12)
    uint32_t n_prev_instances = 0;
    uint32_t cur = 0;                            // the set the most recent call wrote
    crt::TemporalView prev_view{};               // the view of the most recent call
    uint32_t demodulate = 0;                     // the DEMODULATE bit of the most recent call: what the history holds
    bool have_history = false;                   // false until a call succeeds, and after crt_temporal_reset
    bool valid = false;                          // some crt_temporal has been enqueued
    ~TemporalState() {
        void* bufs[] = {d_hist[0], d_hist[1], d_guide[0], d_guide[1], d_key[0], d_key[1], d_out, d_rgba, d_o2w_prev};
        for (void* p : bufs) if (p) (void)hipFree(p);
    }
};

// What crt_display keeps, allocated by a scene's first call: the RGBA8 it writes (one buffer, whichever source a call
// names), and one block of device words: the state the meter kernel writes and the display kernel reads its exposure from, the live
// luminance bins and the bins of the last metered call.  The exposure never comes back to the host unless crt_display_get_state asks.
struct DisplayState {
    uint8_t* d_rgba = nullptr;
    uint32_t* d_words = nullptr;         // display.hpp's layout: the state block, the live bins (kDisplayBinCopies x 256), 256 bins as last metered
    bool valid = false;                  // some crt_display has been enqueued
    bool metered = false;                // some call with CRT_DISPLAY_AUTO_EXPOSURE has been enqueued: the last bins exist
    ~DisplayState() {
        if (d_rgba) (void)hipFree(d_rgba);
        if (d_words) (void)hipFree(d_words);
    }
};

// What crt_bloom keeps, allocated by a scene's first call: the pyramid (every level the frame can have, one after the
// other; a level's U is written over its D on the way back up), the bloomed linear image and its RGBA8.
struct BloomState {
    float* d_pyramid = nullptr;          // levels 1 .. 8, 3 floats per pixel
    float* d_out = nullptr;              // the bloomed MEAN radiance, 3 floats per pixel, linear pixel order
    uint8_t* d_rgba = nullptr;           // crt_resolve_bloom*'s buffer
    bool valid = false;                  // some crt_bloom has been enqueued
    ~BloomState() {
        void* bufs[] = {d_pyramid, d_out, d_rgba};
        for (void* p : bufs) if (p) (void)hipFree(p);
    }
};

// What the first hits of a view into a stage's own buffers need beside their destination (first_hits.hpp), allocated by the first call
// that needs it.
struct FirstHitWork {
    uint2* d_tile_xy = nullptr;          // flat scenes: the tiles of the whole frame, for k_aov
    uint32_t n_local_pixels = 0, tile = 0;
    uint32_t* d_count = nullptr;         // instanced scenes: the 8 counters of the primary rays' queue
    ~FirstHitWork() {
        if (d_tile_xy) (void)hipFree(d_tile_xy);
        if (d_count) (void)hipFree(d_count);
    }
};

// What the ambient-occlusion entries keep, each buffer allocated by the first call that needs it.  View mode: the first hits
// of the view (HIT and NORMAL values in buffers of their own: crt_render_aov's channels stay as they are), the points made of them and the
// image.  Both modes: the visibility words of the call in flight.  Points mode with host pointers: its upload and download buffers.
struct AoState {
    float4* d_hit = nullptr;             // width * height each
    float4* d_normal = nullptr;
    float4* d_view_points = nullptr;     // 2 rows per pixel
    float4* d_image = nullptr;           // what crt_read_ao / crt_ao_device hand out
    bool rendered = false;               // some crt_render_ao has been enqueued
    uint32_t* d_vis = nullptr;           // n x ceil(K / 32) words
    float4* d_points = nullptr;          // crt_ao_points: 2 rows per point
    float4* d_out = nullptr;
    size_t vis_cap = 0, points_cap = 0, out_cap = 0;
    FirstHitWork first_hits;
    ~AoState() {
        void* bufs[] = {d_hit, d_normal, d_view_points, d_image, d_vis, d_points, d_out};
        for (void* p : bufs) if (p) (void)hipFree(p);
    }
};

// What the fog entries keep, each buffer allocated by the first call that needs it.  View mode: the first hits of the view
// (HIT values in a buffer of their own: crt_render_aov's channels stay as they are), the segments made of them and the image.  Both
// modes: the visibility words of the call in flight.  Segments mode with host pointers: its upload and download buffers.  The composite:
// the fogged image, the fifth float image of crt_outputs.cpp.
struct FogState {
    float4* d_hit = nullptr;             // width * height
    float4* d_view_segments = nullptr;   // 2 rows per pixel
    float4* d_image = nullptr;           // what crt_read_fog / crt_fog_device hand out
    bool rendered = false;               // some crt_render_fog has been enqueued
    uint32_t* d_vis = nullptr;           // n x ceil(K / 32) words
    float4* d_segments = nullptr;        // crt_fog_segments: 2 rows per segment
    float4* d_out = nullptr;
    size_t vis_cap = 0, segments_cap = 0, out_cap = 0;
    FirstHitWork first_hits;
    float* d_fogged = nullptr;           // crt_fog_composite's image, width * height * 3
    bool composited = false;             // some crt_fog_composite has been enqueued
    ~FogState() {
        void* bufs[] = {d_hit, d_view_segments, d_image, d_vis, d_segments, d_out, d_fogged};
        for (void* p : bufs) if (p) (void)hipFree(p);
    }
};

// What crt_update_vertices and crt_rebuild_vertices take new positions through, allocated by a scene's first call of either: a scene that
// never moves holds none of it.  The times are those of the most recent call that succeeded (crt_last_update_ms).
struct VertexIntake {
    float* d_verts = nullptr;                // the host forms' upload of the positions
    uint32_t* d_check = nullptr;             // k_check_vertices: non-finite flag, max keys, complemented min keys
    uint32_t* h_check = nullptr;             // pinned
    hipEvent_t ev_a = nullptr, ev_b = nullptr;
    bool have_times = false, times_pending = false;
    float device_ms = 0.f, wall_ms = 0.f;
    ~VertexIntake() {                        // on the scene's device
        if (d_verts) (void)hipFree(d_verts);
        if (d_check) (void)hipFree(d_check);
        if (h_check) (void)hipHostFree(h_check);
        if (ev_a) (void)hipEventDestroy(ev_a);
        if (ev_b) (void)hipEventDestroy(ev_b);
    }
};

// What crt_update_vertices keeps between updates, allocated by a scene's first update: a scene that never updates holds none of it.
struct RefitState {
    int device = 0;
    uint32_t* d_order = nullptr;             // node8 indices level by level, root level first, then the BVH2's the same way
    std::vector<uint32_t> level8, level2;    // level8[l] = position in d_order of node8 level l (+ end); level2 the same for the BVH2
    crt::RefitMesh* d_mesh = nullptr;        // the scene as one refit mesh (its vertex pointer changes between calls) ...
    crt::RefitMesh* h_mesh = nullptr;        // ... sent from here, pinned
    crt::RefitSeg* d_seg = nullptr;          // the one segment of every launch: entries from 0, items from 0, mesh 0
    float* d_box8 = nullptr;                 // the float box of every node8 (6 floats), which its parent's slot reads
    std::vector<hipEvent_t> ev_peer;         // per peer, on its device: "the peer's stream is done with the old scene"
    ~RefitState() {
        (void)hipSetDevice(device);
        void* ptrs[] = {d_order, d_box8, d_mesh, d_seg};
        for (void* p : ptrs) if (p) (void)hipFree(p);
        if (h_mesh) (void)hipHostFree(h_mesh);
        for (hipEvent_t e : ev_peer) if (e) (void)hipEventDestroy(e);
        (void)hipSetDevice(device);
    }
};

// What crt_rebuild_vertices keeps between rebuilds, allocated by a scene's first rebuild: a scene that never rebuilds holds
// none of it, and no walk or frame reads it.
struct RebuildState {
    crt_triangle* d_src = nullptr;           // the triangles in SOURCE order (create threw its copy away): scattered back from the leaf order once
    ~RebuildState() { if (d_src) (void)hipFree(d_src); }     // on the scene's device
};

// The lights of an instanced scene that follow its instances (crt_scene_create_instanced_lit).  The scene's d_lights is
// then the world table these are rebuilt into, n_lights its current total.
struct SceneLights {
    uint32_t n_static = 0;
    std::vector<uint2> mesh;              // per mesh: (first light in `obj`, count)
    std::vector<crt_light> obj;           // every mesh's object-space lights, mesh after mesh (the source of set_mesh_lights' upload)
    float* d_static = nullptr;            // n_static x 18
    float* d_obj = nullptr;
    uint2* d_mesh = nullptr;
    uint32_t* d_first = nullptr;          // per instance (the handle's capacity): the table index of its first light
    uint32_t* d_block_sums = nullptr;     // one word per 1024 instances
    uint32_t* d_total = nullptr;
    float* d_partial = nullptr;           // the tree sum's partials, sized with the table
    size_t table_cap = 0;                 // lights d_lights holds
    uint64_t seen = 0;                    // the handle's mutation count the table was built from
    bool stale = true;
    ~SceneLights() {
        void* bufs[] = {d_static, d_obj, d_mesh, d_first, d_block_sums, d_total, d_partial};
        for (void* p : bufs) if (p) (void)hipFree(p);
    }
};

// The scene-level device buffers a replica shares (same GPU: crt_set_devices with a device listed again, option "streams") or copies
// (another GPU).  crt_scene::shared_slot gives the pointer member of each, shared_bytes its size.  A slot takes part when its pointer is
// non-null: a flat scene's creators fill nodes .. lights always (an array of no elements, such as the normals of a mesh without any, still
// gets a small allocation: its pointer is non-null, its size 0, and a replica on another GPU allocates 16 bytes of its own), texcoords and
// textures with textures, bvh2 and tris2 with a BVH2, planes at the first CWBVH frame (ensure_planes).  That is exactly the set the
// creators used to list by hand, and each size is written where the buffer is allocated.  An instanced scene never replicates and leaves
// every size 0.
enum SharedBuf { kSharedNodes, kSharedPlanes, kSharedTris, kSharedTriangles, kSharedNormals, kSharedMaterials, kSharedLights, kSharedTexcoords,
                 kSharedTextures, kSharedBvh2, kSharedTris2, kSharedBufs };

struct crt_scene {
    int device = 0;
    int n_cu = 256;
    hipStream_t stream = nullptr;
    uint32_t width = 0, height = 0, max_depth = 1, n_lights = 0;

    // scene (replicated on every rank)
    uint4* d_nodes = nullptr;
    float4* d_planes = nullptr;          // the nodes' child planes as floats, 12 rows per node (uniform node steps; built by ensure_planes at the first CWBVH frame)
    float4* d_tris = nullptr;
    int4* d_triangles = nullptr;
    float* d_normals = nullptr;
    float4* d_materials = nullptr;
    float* d_lights = nullptr;
    float2* d_texcoords = nullptr;
    float* d_textures = nullptr;         // albedo array as RGB32F (c / 255.0f)
    int32_t tex_width = 0, tex_height = 0, n_textures = 0;
    crt_bvh_info info{};
    float4* d_bvh2 = nullptr;            // FlatNode array as uploaded by the reference (only when desc.bvh was given)
    float4* d_tris2 = nullptr;           // intersection records in BVH2 leaf-slot order
    uint32_t bvh2_stack = 0;             // BVH2 depth + 2
    size_t n_vertices = 0, n_normals = 0, n_slots = 0;   // as created (n_slots: the leaf-order triangle array); crt_update_vertices checks against them
    VertexIntake* intake = nullptr;      // what both take new positions through, from the first update or rebuild on
    RefitState* refit = nullptr;         // crt_update_vertices' state, from the first update on
    RebuildState* rebuild = nullptr;     // crt_rebuild_vertices' state, from the first rebuild on
    uint32_t gpu_build_flags = 0;        // build-on-device scenes: the builder (CRT_GPU_BUILD_*) a rebuild runs again
    // A scene whose geometry is a live crt_instances handle (crt_scene_create_instanced): BORROWED, and bound from create to
    // destroy.  d_nodes / d_tris / d_planes stay null: a frame reads the handle's arrays as they are when it is enqueued.  d_triangles,
    // d_normals and d_texcoords hold every mesh's arrays one after the other, d_mesh_base where each mesh's start.
    crt_instances* inst = nullptr;
    uint4* d_mesh_base = nullptr;        // per mesh: first triangle, first normal, first texcoord, the lights it carries (§18)
    int32_t* d_qinst = nullptr;          // the hit instance of every entry of the path-ray queue (beside d_qhits)
    // material offsets and masks in its frames.  The two tables are the rule the handle holds offsets to while bound
    uint4* d_mesh_mtl = nullptr;         // per mesh: least, greatest v[3], 1 = every vt indexes the mesh's texcoords, 0
    uint32_t* d_tex_before = nullptr;    // n_materials + 1: the textured materials below each index
    uint32_t instance_masks = 0, mask_primary = 255, mask_bounce = 255, mask_shadow = 255;   // options of those names
    uint64_t cmask_seen = 0;             // the handle's child-mask pass this scene's stream last waited for
    SceneLights* lit = nullptr;          // lights that follow the instances; null = desc->lights alone, as before
    AovState* aov = nullptr;             // crt_render_aov's buffers, from the first call on
    DenoiseState* denoise = nullptr;     // crt_denoise's buffers, from the first call on
    TemporalState* temporal = nullptr;   // crt_temporal's buffers, from the first call on
    DisplayState* display = nullptr;     // crt_display's buffers and exposure state, from the first call on
    BloomState* bloom = nullptr;         // crt_bloom's buffers, from the first call on
    AoState* ao = nullptr;               // the ambient-occlusion entries' buffers, from the first call on
    FogState* fog = nullptr;             // the fog entries' buffers, from the first call on
    uint32_t temporal_form = 0;          // option "temporal_form": how a CLAMP call reads its neighbourhood: 0 = the form measured faster, 1 = staged, 2 = direct
    crt::TemporalView aov_view{};        // the view of the most recent crt_render_aov that rendered HIT, recorded at enqueue: crt_temporal's current view
    bool have_aov_view = false;
    uint32_t denoise_form = 0;           // option "denoise_form": 0 = each pass in the form measured faster at its tap spacing, 1 = staged, 2 = direct

    // shard + frame buffers
    uint32_t rank = 0, world = 1, tile = 16;   // 16x16: four waves per tile — fine enough for the cost-sorted schedule (1 M triangles: 0.273 ms at 64, 0.257 at 16)
    std::vector<uint2> tiles;            // local tiles
    // Processing order of the local tiles (FrameArgs::tile_order): centre-out to begin with, then by measured cost, most
    // expensive first (longest-processing-time-first scheduling of the launch).  One frame after every change of camera,
    // shard or frame size has each wave add the clock ticks it spent to its tile's counter; the counters come back
    // through a pinned buffer without a stream synchronise, and the re-sorted order is uploaded in stream order.
    uint32_t* d_tile_order = nullptr; uint32_t* d_tile_cost = nullptr;
    uint32_t* h_tile_cost = nullptr; uint32_t* h_tile_order = nullptr;      // pinned
    hipEvent_t ev_tile_cost = nullptr, ev_tile_order = nullptr;
    enum { TILES_WANT = 0, TILES_PENDING = 1, TILES_DONE = 2 };
    int tile_state = TILES_WANT;
    uint32_t adaptive_tiles = 1;             // option: 0 keeps the centre-out order
    bool tile_order_uploading = false;
    bool tiles_measured_once = false;
    uint32_t frames_since_tile_measure = 0;
    bool capturing = false;                  // crt_debug_time_graph: no host-side decisions inside a stream capture
    uint2* d_tile_xy = nullptr;
    uint32_t n_local_tiles = 0, n_local_pixels = 0;
    uint64_t n_local_in_frame = 0;
    float* d_sum = nullptr;
    float* d_linear = nullptr;
    uint8_t* d_rgba = nullptr;
    uint8_t* h_rgba = nullptr;           // pinned staging buffer of crt_resolve
    float* d_gamma = nullptr;            // the 256 thresholds of the pinned gamma (resolve kernels)
    float4* d_rays[2] = {nullptr, nullptr};   // path-ray queues: max_depth > 1, instanced scenes, and from the first frame through a lens on
    // the primary rays of a frame through a lens (camera aperture > 0; k_raygen_lens): a queue of their own, which no later segment of the
    // frame writes over, sized like one of d_rays for the sub_capacity in force (crt_debug_read_queue(0, 0) reads it)
    float4* d_rays_lens = nullptr;
    uint32_t lens_sub_capacity = 0;
    bool lens() const { return cam.aperture > 0.0f; }     // crt_set_camera has checked the two fields
    // The caller's own camera rays (crt_set_camera_rays): width x height entries of crt_ray, a copy the scene owns, allocated
    // by the first set, reused by later ones and freed with the scene.  While set, segment 0 of a frame is fed by k_raygen_rays and the
    // camera is not read.  A stream replica (option "streams") reads its primary's buffer: every shard the same one.
    float4* d_cam_rays = nullptr;
    bool cam_rays_set = false;
    bool camera_rays() const { return primary ? primary->cam_rays_set : cam_rays_set; }
    const float4* camera_rays_buffer() const { return primary ? primary->d_cam_rays : d_cam_rays; }
    // The environment (crt_set_environment): scene state like the camera, on every device of the scene a copy of its own.
    // d_env: size x size texels (r, g, b, 0), row 0 first; null = none, and every frame is launched as without this member.  With one, a
    // flat scene's frame runs every segment queue-fed and pretraced, k_env_miss between the closest-hit launch and the shade-only pass.
    float4* d_env = nullptr;
    uint32_t env_size = 0, env_flags = 0;
    float env_rotation[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, env_scale[3] = {1.f, 1.f, 1.f};
    bool env() const { return d_env != nullptr; }
    // DEFERRED NEE shadow rays (option "inplace_shadow" 0 / 2, rt_kernels.hip k_segment<!INPLACE>): the frame's NEE queue — one region per
    // deferring segment, 8 sub-queues each, 2 x float4 per ray: (o, tmax) (d, contribution slot) — and the contribution slots, one per
    // (deferring segment, path): (C | T e, visibility word)
    float4* d_nee = nullptr;
    float4* d_contrib = nullptr;
    // option "sort_shadow": the frame's deferred shadow rays walked in the order of the cell they start in (rt_kernels.hip k_nee_*):
    // perm[place] = queue entry, 4096-bin histogram + cursors + the eight parts' lengths
    uint32_t* d_nee_perm = nullptr;
    uint32_t* d_nee_bins = nullptr;           // hist [4096] | cursor [4096] | meta [9 x stride]
    uint32_t sort_shadow = 0;                 // (1 M triangles, four segments: 7.18 against 7.59 Gray/s unsorted — the sort costs more than the 4 % fewer any-hit node steps return)
    uint32_t defer_cap = 0, defer_regions = 0, defer_sub_capacity = 0;   // what the two were sized for
    uint32_t lfinal_cap = 0;                  // samples d_lfinal is sized for
    float4* d_qhits = nullptr;                // closest hits of the path-ray queue (max_depth > 1, option bounce_refill)
    // segments >= 1: 0 = fused lock-step k_segment (default); 1 = closest hits through lane-refill pools (k_closest_queue) + shade-only pass
    uint32_t bounce_refill = 0;
    uint32_t refill_pool = 256;               // rays per wave of k_closest_queue (64 with refill_min 65: lock-step batches)
    // k_shadow_deferred: rays per pool / per chunk a wave reserves, and the idle lanes that trigger a refill (65: never — one lock-step
    // batch per 64 rays of the pool).  1 M triangles, four segments: lock-step 64 7.34, static pools 128 / 16 7.42 (7.61 - 7.67 after the
    // kernarg change), persistent 256 / 16 7.72 Gray/s
    uint32_t shadow_pool = 256;
    uint32_t shadow_refill_min = 16;
    uint32_t step_hist_mode = 0;             // crt_debug_step_hist: 0 = node steps by enabled lanes, 1 = by distinct (node, octant) keys in the wave
    uint32_t shadow_waves = 6;               // waves per SIMD the persistent any-hit grid of the deferred shadow rays is sized for (the kernel fits 8; two shards'
                                             // grids share the chip: 4 / 5 / 6 / 7 / 8 = 7,723 / 7,767 / 7,776 / 7,750 / 7,721 on four segments, 10,540 / 10,450 / 10,338 at 5 / 6 / 8 on two)
    // the pool launches (k_shadow_deferred, k_closest_queue) as PERSISTENT grids: as many waves as the chip holds, each reserving chunks of
    // `pool` rays through per-queue cursors until every queue is dry; 0 = one workgroup per pool
    uint32_t persistent = 1;
    // crt_render_frames, how the samples of a launch sit on the hardware (include/crt.h, option "wave_samples"): 0 = one after the other in
    // each wave; 1 = side by side on the waves of a workgroup; 2 (default) = four samples of a 4 x 4 pixel quadrant in the lanes of a wave
    // where the launch allows it (a multiple of 4 samples, a tree of >= 64 nodes, CWBVH), otherwise 1 when the launch is bound by its longest
    // waves rather than by throughput (use_wave_samples) and 0 when not; 3 = lanes where allowed, else 0
    uint32_t wave_samples = 2;
    uint32_t wide_first = 2;            // first-segment kernels built for 6 waves per SIMD: 0 never, 1 always, 2 by the same measure
    float tile_cost_spread = 0.f;       // 99th percentile of the measured tile costs over their mean; 0 = nothing measured yet
    LaunchInfo last_launch;             // set once per chain by the renderer that enqueued it
    bool use_wave_samples() const { return wave_samples == 2u ? bound_by_longest_waves() : wave_samples == 1u; }
    bool bound_by_longest_waves() const {
        // One wave renders the n samples of its 64 pixels one after the other: the launch cannot end before the most expensive
        // waves have done n samples, c99 * n, while the chip needs about mean * n * waves / slots for all of them.  When the first
        // is the larger, the samples go on 4 waves side by side (1 M triangles at 1080p, 8 frames per launch: 1/4 of the frame
        // 0.133 -> 0.062 ms per frame, 1/8 0.114 -> 0.039; the whole frame is throughput-bound and stays as it is, and so does a
        // Cornell box down to 1/4 of the frame — its waves are short and four times as many of them cost more than they save).
        const double waves = (double)(n_local_pixels + 63u) / 64.0, slots = (double)n_cu * 4.0 * 5.0;
        if (tile_cost_spread == 0.f) return waves <= 2.0 * slots;
        return (double)tile_cost_spread * slots >= 0.9 * waves;
    }
    crt::PathBuffers pb{};
    uint32_t stack_entries = CRT_STACK_ENTRIES;
    uint32_t sub_capacity = 0;                // entries per sub-queue (8 per queue)
    uint32_t* d_counts = nullptr;        // 2 banks (frame parity) of counter(seg, kind, group): kind 0 = rays into segment, 1 = its shadow rays
    uint32_t bank = 0;                   // bank of the most recent frame
    bool counts_clean = false;           // both banks known to be zero where the next frame needs them
    uint32_t* counts() const { return d_counts + (size_t)bank * kCounters; }
    uint32_t* h_counts = nullptr;        // pinned
    bool frame_buffers_ready = false;

    crt_camera cam{};
    bool have_camera = false;
    uint32_t jitter = 1;
    bool count_visits = false;
    bool count_batched = false;               // option count_visits 2: counting frames may share a launch in the timed form (four samples in the lanes of a wave)
    unsigned long long* d_visit_totals = nullptr;   // [0..3] lane visits: closest nodes/tris, any nodes/tris; [4..7] wave-level steps of the same blocks; [8] closest-hit rays that hit; [10], [11] closest / any-hit node visits of uniform node steps
    unsigned long long* h_visit_totals = nullptr;   // pinned

    // scratch for crt_trace (host rays)
    float4* d_t_rays = nullptr; float4* d_t_hits = nullptr; uint32_t* d_t_stats = nullptr; size_t t_cap = 0;

    // telemetry
    std::vector<EventSpan> spans;
    int n_spans = 0;
    crt_frame_stats stats{};
    bool stats_pending = false;
    bool stats_from_frame = false;
    bool stats_counted = false;
    uint32_t tri_min = 2;                    // traverse_pool vote: node step while node-ready lanes >= tri_min x triangle-waiting lanes
    // NEE shadow rays: 1 = walked inside k_segment, every segment; 0 = every segment's deferred to ONE any-hit launch behind the last
    // segment (k_shadow_deferred) with the contributions folded per path in segment order (k_fold_paths); 2 = first segment in place,
    // bounce segments deferred; 3 (default) = 2 for trees of 64+ nodes (1 M triangles, four segments: 7.23 -> 7.72 Gray/s), else 1
    uint32_t inplace_shadow = 3;
    uint32_t accel = 0;                      // frames: 0 CWBVH; 1 BVH2 walked as the shipped shader does (first visited wins); 2 BVH2, lowest id wins
    uint32_t refill_min = 8;                // walk_pool (crt_trace, k_closest_queue): idle lanes that trigger a refill
    // crt_trace: rays per wave (its refill pool): 64, 128 or 256.  64 = one lock-step batch per single-wave workgroup: four times the
    // workgroups for the dispatcher to balance, which is what a launch of a few million rays needs (tools/refill_probe.py, 1 M
    // triangles: 2.07 M primary rays 0.153 ms against 0.346 with 256-ray pools, whose 8,100 waves all start at once and end with the
    // slowest; 0.81 M shadow rays 0.192 / 0.202 / 0.230 ms for 64 / 128 / 256; 1.16 M bounce rays 0.332 / 0.320 / 0.321 — the one
    // case where refill beats the finer grain, by 4 %)
    uint32_t trace_pool = 64;
    uint32_t trace_occupancy = 8;            // persistent grids only (oversubscribe >= 1): workgroups per CU
    // 0: one chunk per workgroup, the hardware dispatcher hands chunks to CUs as they drain (measured 13 % faster than
    // a persistent grid on the 1 M mesh: per-chunk cost varies 10x between sky and grazing rays);
    // k >= 1: persistent grid of k x the resident workgroups, static schedule (rt_kernels.hip)
    uint32_t oversubscribe = 0;
    bool special_materials = false;          // some material is Mirror_type / Disney_type (albedo.w, Scene.h:111-132): k_segment<MAT>
    uint32_t waves_per_workgroup = 1;        // 1 = every wave its own workgroup (default), 2, or 4 = 256-thread workgroups
    uint32_t lanes_per_ray = 8;              // option "lanes_per_ray" (1, 2, 4, 8): how far a ray may spread over the lanes of its draining wave (rt_kernels.hip walk_batch)
    uint32_t* d_overflow = nullptr;          // dropped stack pushes since scene creation (stays 0 for every accepted tree)
    float4* d_lfinal = nullptr;              // batched frames on multi-segment paths: per (sample, pixel) final radiance (SegmentArgs::l_final)
    // bounce rays regrouped by (direction octant, origin cell) between segments (rt_kernels.hpp RayBins).  Tables per segment a ray
    // can enter (1..16), capacities / offsets twice (frame parity: the launch that consumes a segment's rays reads the layout its
    // producer used while k_bin_scan already writes the next frame's).
    // option "ray_bins": 0 (default) = per-group sub-queues in emission order; 1 = bins, the lanes of a wave that share a key take their
    // places with one atomic; 2 = bins, one atomic per ray; 3 = 1 for the first segment's emission, 2 for the bounce segments'.
    // Measured on the 1 M-triangle frame, 4 segments, 4 samples per launch: wave-level traversal steps -10 % (lane utilisation of
    // the closest-hit node block 46.5 -> 51.7 %), frame time +3.6 % / +31 % / +5 % for 1 / 2 / 3 — what the append costs
    // (a wave of bounce rays holds ~50 different keys) exceeds what the walk gains; profiles/r03_experiments.md.
    uint32_t ray_bins = 0;
    bool rows_padded = false;                // d_nodes / d_tris are at the build's stride (CRT_NODE_ROWS / CRT_TRI_ROWS)
    bool rays_doubled = false;               // the path-ray queues have their overflow half (allocated when the bins are first used)
    uint32_t* d_bins = nullptr;              // one allocation: count [17][B] | cap [2][17][B] | off [2][17][B] | start [17][B + 1] | ovf [17 x 32]
    float bounds_lo[3] = {0.f, 0.f, 0.f}, bounds_hi[3] = {1.f, 1.f, 1.f};   // of the vertices: the cell grid of the bins
    uint32_t* bin_count(uint32_t seg) const { return d_bins + (size_t)seg * CRT_RAY_BINS; }
    uint32_t* bin_cap(uint32_t par, uint32_t seg) const { return d_bins + (size_t)(17 + par * 17 + seg) * CRT_RAY_BINS; }
    uint32_t* bin_off(uint32_t par, uint32_t seg) const { return d_bins + (size_t)(17 * 3 + par * 17 + seg) * CRT_RAY_BINS; }
    uint32_t* bin_start(uint32_t seg) const { return d_bins + (size_t)17 * 5 * CRT_RAY_BINS + (size_t)seg * (CRT_RAY_BINS + 1u); }
    uint32_t* bin_ovf(uint32_t seg) const { return d_bins + (size_t)17 * 5 * CRT_RAY_BINS + (size_t)17 * (CRT_RAY_BINS + 1u) + (size_t)seg * 32u; }
    static size_t bins_words() { return (size_t)17 * 5 * CRT_RAY_BINS + (size_t)17 * (CRT_RAY_BINS + 1u) + 17u * 32u; }
    uint32_t last_build = 1;                 // option "last_build": a one-pass launch that is the path's last segment runs the build compiled as one (k_segment<LAST>)
    uint32_t lean_build = 1;                 // option "lean_build": such a launch runs that build's LEAN form (k_segment<LAST,LEAN>) where launch_segment finds what the form has compiled in
    bool tree_validated = false;             // the CWBVH passed crt_scene_create's host validator (validate_cwbvh), whose depth sized the stack: the LEAN form's bare pushes rest on it.
                                             // A tree built or rebuilt on the device never went through it and keeps the checked pushes
    uint32_t debug_fail_batch_alloc = 0;     // test hook (option of the same name): the next growth of the batch buffers fails before it allocates
    uint32_t batch_cap = 1;                  // samples the path state, the ray queues and d_lfinal are sized for (1 until crt_render_frames needs more)
    bool stats_seg0_counted = false;         // the launch the pending stats describe ran along the caller's camera rays: segment 0's ray count is its queue's
    uint32_t samples_in_stats = 1;           // samples per pixel of the launch the pending stats describe (crt_render_frames batches)
    // event spans behind crt_frame_stats.ms_*: 2 = every launch, 1 = closest-hit launches only, 0 = none (the default: an event-carrying
    // dispatch cannot overlap its neighbours, ~5 us of stream time per launch — 8 % of a Cornell-box frame, 0.8 % of a 1 M-triangle one)
    uint32_t timing = 0;
    bool timing_accumulate = false;          // spans pile up over frames (crt_frame_stats then holds sums) instead of per frame

    // ---- several GPUs behind ONE handle (crt_set_devices): this scene is logical device 0, `peers` are devices 1..n-1, each a
    // complete scene on its own GPU (replicated buffers, own stream, own shard of the tiles).  Every entry point fans out to them;
    // crt_read_sum / crt_resolve gather their packed tile buffers to this device and un-tile the whole frame here.
    std::vector<crt_scene*> peers;           // owned
    crt_scene* primary = nullptr;            // set in a peer
    size_t shared_bytes[kSharedBufs] = {};   // the replica table (SharedBuf): bytes of each buffer as it stands, read by copies to another GPU
    void** shared_slot(int k) {
        switch (k) {
            case kSharedNodes: return reinterpret_cast<void**>(&d_nodes);
            case kSharedPlanes: return reinterpret_cast<void**>(&d_planes);
            case kSharedTris: return reinterpret_cast<void**>(&d_tris);
            case kSharedTriangles: return reinterpret_cast<void**>(&d_triangles);
            case kSharedNormals: return reinterpret_cast<void**>(&d_normals);
            case kSharedMaterials: return reinterpret_cast<void**>(&d_materials);
            case kSharedLights: return reinterpret_cast<void**>(&d_lights);
            case kSharedTexcoords: return reinterpret_cast<void**>(&d_texcoords);
            case kSharedTextures: return reinterpret_cast<void**>(&d_textures);
            case kSharedBvh2: return reinterpret_cast<void**>(&d_bvh2);
            case kSharedTris2: return reinterpret_cast<void**>(&d_tris2);
        }
        return nullptr;
    }
    void* shared_ptr(int k) const { return *const_cast<crt_scene*>(this)->shared_slot(k); }
    uint32_t shard_rank = 0, shard_world = 1; // the caller's shard of the frame (crt_set_shard); rank / world below are this stream's share of it
    uint32_t streams = 1;                    // option "streams": this many tile shards of the frame on streams of their own, on this one GPU
    bool shares_scene = false;               // a replica on its primary's own device: the scene buffers are the primary's, not copies
    std::vector<float*> d_gather;            // per peer, on THIS device: its packed sum buffer as received
    std::vector<uint2*> d_peer_tiles;        // per peer, on THIS device: its local tile list (for the un-tiling launch)
    std::vector<hipEvent_t> ev_peer;         // per peer: "your slice has arrived" (copy transport)
    void* rccl_lib = nullptr;                // dlopen handle; comms[k] = communicator of logical device k
    std::vector<void*> rccl_comms;
    uint32_t gather_transport = 0;           // 0 = RCCL send/recv over xGMI, 1 = hipMemcpyPeerAsync (also: virtual devices, RCCL absent)
    float last_gather_ms = 0.f;

    ~crt_scene() {
        drop_peers();
        hipSetDevice(device);
        if (stream) hipStreamSynchronize(stream);
        if (inst) crt::instances_unbind(inst, stream);
        delete refit;
        delete rebuild;
        delete intake;
        delete lit;
        delete aov;
        delete denoise;
        delete temporal;
        delete display;
        delete bloom;
        delete ao;
        delete fog;
        if (shares_scene)                   // borrowed from the primary, which frees them
            for (int k = 0; k < kSharedBufs; ++k) *shared_slot(k) = nullptr;
        void* ptrs[] = {d_gamma, d_texcoords, d_textures, d_bvh2, d_tris2, d_nodes, d_planes, d_tris, d_triangles, d_normals, d_materials, d_lights, d_tile_xy, d_sum, d_linear, d_rgba,
                        d_rays[0], d_rays[1], d_rays_lens, d_cam_rays, d_env, d_nee, d_contrib, d_nee_perm, d_nee_bins, d_qhits, pb.L, pb.T, pb.seed, d_counts,
                        d_t_rays, d_t_hits, d_t_stats, d_visit_totals, d_overflow, d_tile_order, d_tile_cost, d_lfinal, d_bins, d_mesh_base, d_qinst, d_mesh_mtl, d_tex_before};
        for (void* p : ptrs) if (p) hipFree(p);
        if (h_tile_cost) hipHostFree(h_tile_cost);
        if (h_tile_order) hipHostFree(h_tile_order);
        if (ev_tile_cost) hipEventDestroy(ev_tile_cost);
        if (ev_tile_order) hipEventDestroy(ev_tile_order);
        if (h_counts) hipHostFree(h_counts);
        if (h_rgba) hipHostFree(h_rgba);
        if (h_visit_totals) hipHostFree(h_visit_totals);
        for (EventSpan& s : spans) { if (s.a) hipEventDestroy(s.a); if (s.b) hipEventDestroy(s.b); }
        if (stream) hipStreamDestroy(stream);
    }

    void drop_peers();      // defined with crt_set_devices

    // grid of a traversal kernel (always a multiple of 8: one slice per XCD group); persistent variant bounded by LDS and registers
    // (the XCD-aware schedule in rt_kernels.hip groups workgroups by blockIdx & 7)
    // reg_cap = workgroups per CU the kernel's VGPR count admits (k_segment ~90 VGPRs -> 5, k_trace/k_shadow <= 64 -> 8)
    // chunk = items one workgroup pass covers: 256 (lock-step kernels) or 1024 (pool kernels)
    uint32_t trace_grid(uint64_t n, uint32_t reg_cap, uint32_t chunk = CRT_TRACE_BLOCK) const {
        // every group's share in one pass: group 0 owns ceil(units / 8) units of 4096 items (== sub_capacity for n = P)
        const uint64_t share = ((n + 4095) / 4096 + 7) / 8 * 4096;
        uint64_t g = 8 * ((share + chunk - 1) / chunk);
        if (oversubscribe != 0u) {
            const uint64_t lds = (uint64_t)(CRT_TRACE_BLOCK / 64) * (stack_entries + CRT_HIT_SLOTS) * 64 * 8;
            const uint64_t per_cu = std::min<uint64_t>(std::min(trace_occupancy, reg_cap), std::max<uint64_t>(1, (160 * 1024) / lds));
            g = std::min(g, ((uint64_t)n_cu * per_cu * oversubscribe + 7) / 8 * 8);
        }
        return (uint32_t)std::max<uint64_t>(g, 8);
    }
    // waves the chip holds at once of a kernel whose wave needs `lds` bytes (handed out in 1,280-byte units) and runs `per_simd` to a SIMD:
    // the grid of a persistent launch (a multiple of 8: one slice per XCD group)
    uint32_t resident_waves(size_t lds, uint32_t per_simd) const {
        const uint64_t units = (lds + 1279) / 1280, by_lds = units ? (160u * 1024u / 1280u) / units : 32u;
        const uint64_t per_cu = std::max<uint64_t>(1, std::min<uint64_t>(4ull * per_simd, by_lds));
        return (uint32_t)((uint64_t)n_cu * per_cu / 8 * 8);
    }
    size_t pool_lds() const { return (size_t)(stack_entries + CRT_HIT_SLOTS) * 64 * sizeof(uint2); }     // LDS of a wave of the pool kernels (k_closest_queue, k_shadow_deferred)
    uint32_t flat_grid(uint64_t n) const {
        uint64_t blocks = (n + 255) / 256;
        return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(blocks, (uint64_t)n_cu * 8));
    }
    // a span's events are attached to the launches themselves (crt::set_launch_events), not recorded between them
    EventSpan* new_span(int kind) {
        if (timing == 0u || (timing == 1u && kind != 1)) return nullptr;
        if (n_spans >= (int)spans.size()) return nullptr;
        EventSpan* s = &spans[n_spans];
        // the events of a span are created the first time it is used: a scene that never asks for timings creates none (272 event creations
        // were a quarter of a millisecond of every crt_scene_create)
        if (!s->a && hipEventCreate(&s->a) != hipSuccess) { s->a = nullptr; return nullptr; }
        if (!s->b && hipEventCreate(&s->b) != hipSuccess) { s->b = nullptr; return nullptr; }
        ++n_spans;
        s->kind = kind;
        return s;
    }
};

// What crosses between the translation units
namespace crt {
// crt_create.cpp
bool light_finite(const crt_light& l);   // every field of a light is finite
// what a create and a replica both end with: nodes and records at the traversal's strides, the overflow word, the counter banks, the spans
int finish_scene_setup(crt_scene* s);
void adopt_tree(crt_scene* s, DeviceTree& t);     // publishes a built tree into the scene (create on the device, rebuild); cannot fail
// The traversal's copies of nodes and records at the build's stride (CRT_NODE_ROWS / CRT_TRI_ROWS): packed input -> padded copy.
template <typename T>
int pad_rows(hipStream_t st, const char* who, T** buf, uint32_t rows_in, uint32_t rows_out, size_t n_items) {
    if (rows_in == rows_out || !*buf) return CRT_OK;
    T* padded = nullptr;
    int rc = dev_alloc(&padded, n_items * rows_out);
    if (rc) return rc;
    launch_restride(*buf, rows_in, padded, rows_out, n_items, st);
    if (hipStreamSynchronize(st) != hipSuccess || hipGetLastError() != hipSuccess) { (void)hipFree(padded); return fail(CRT_ERR_HIP, std::string(who) + "re-striding failed"); }
    (void)hipFree(*buf);
    *buf = padded;
    return CRT_OK;
}
// A device buffer of a stage that follows the size of its calls: at least `need` items at *p, *cap what it holds.
template <typename T>
int grow(crt_scene* s, T** p, size_t* cap, size_t need) {
    if (*p && *cap >= need) return CRT_OK;
    if (*p) {
        HIPCHK(hipStreamSynchronize(s->stream));                          // an earlier call may still use the old one
        (void)hipFree(*p); *p = nullptr; *cap = 0;
    }
    const int rc = dev_alloc(p, need);
    if (rc) return rc;
    *cap = need;
    return CRT_OK;
}
// crt_device.cpp
void warm_start(int device);             // the library's code objects start loading on `device` in the background, once per device (crt_warmup's Warmer)
int warm_wait();                         // waits for that load; its result (0 = fine)
void deal_tiles(uint32_t width, uint32_t height, uint32_t T, uint32_t rank, uint32_t world, std::vector<uint2>& tiles, uint64_t* pixels_in_frame);
crt::FrameArgs frame_args(const crt_scene* s, float rx, float ry);
int ensure_planes(crt_scene* s);         // the nodes' child planes as floats, built in stream order before the first frame that walks the CWBVH
int ensure_light_table(crt_scene* s);    // the world light table of a scene with mesh lights, rebuilt if its handle has changed
// every peer's packed sum buffer -> d_gather[k] on the primary device, complete in the primary's stream order when this returns
int gather_peers(crt_scene* s);
// crt_update_vertices_device / crt_rebuild_vertices_device (`rebuild`) with normals on the device beside the positions (null: the scene's
// stay), under `caller`'s name in every refusal
int scene_take_device_geometry(crt_scene* s, const float* d_vertices, size_t n_vertices, const float* d_normals, size_t n_normals, bool rebuild, int sync,
                               const char* caller);
// crt_frames.cpp
int alloc_frame_buffers(crt_scene* s);   // the frame buffers of the shard (rank, world, tile) as they stand, anew
int ensure_frame(crt_scene* s);          // the shard's frame buffers, allocated by the first call that needs them
int ensure_queue_hits(crt_scene* s, bool hits, bool instances);     // d_qhits / d_qinst beside the path-ray queue
crt::RaygenArgs raygen_args(const crt_scene* s, const crt::FrameArgs& f, float4* rays, uint32_t* count, bool zero_bank);
crt::InstMaskQueueArgs inst_queue_args(const crt_scene* s, const crt::InstancesView& v, const float4* rays, const uint32_t* count, uint32_t ray_mask,
                                       unsigned long long* visit_totals);
}  // namespace crt
#pragma GCC visibility pop
