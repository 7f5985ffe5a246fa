/*
 * crt.h — C ABI of the MI355X-native ray/BVH-traversal hot path.
 *
 * Drop-in boundary for the place where the reference dispatches its GLSL fragment
 * shader (Caitlyn/Scene.h:1000-1156 upload, :1158-1231 per-frame dispatch,
 * :1233-1246 camera uniforms).  Every entry point cites the reference interface it
 * replaces.  Plain pointers and sizes only; no C++ or torch types cross this line.
 *
 * Conventions
 *   - every function returns 0 on success, a negative crt_status otherwise;
 *     crt_last_error() returns a thread-local description (the reference prints and
 *     continues, Scene.h:510-511 / Shader.h:84-94; this ABI never throws).
 *   - a crt_scene handle is NOT thread-safe: one caller thread (the reference is a
 *     single thread owning the GL context, main.cpp:22).
 *   - all calls are synchronous on return unless named *_async.
 *   - functions marked [host] need no GPU; everything else fails with
 *     CRT_ERR_NO_DEVICE when no gfx950 device is visible (there is no CPU fallback).
 *   - image rows are bottom-row-first like GL (Quad.h:16-24).
 */
#ifndef CRT_H_
#define CRT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CRT_ABI_VERSION 6   /* 6: crt_resolve_device, crt_get_launch_times, count_visits 2; options inplace_shadow 2 (deferred shadow rays), bounce_refill / refill_pool / shadow_pool / shadow_refill_min in every build,
                              *    tri_share / compact_shadow gone; crt_debug_launch_info's build word carries the one-pass bit;
                              * 5: crt_frame_stats.nodes_closest_uniform / nodes_any_uniform (the struct grew);
                              * 4: crt_warmup, crt_shard_tiles, crt_debug_launch_info, crt_debug_step_hist; options lanes_per_ray, ray_bins 4 / 5, tri_share bits;
                              * 3: crt_frame_stats.closest_hits, crt_set_devices (one process, several GPUs), crt_has_experiments;
                              * 2: crt_frame_stats.stack_overflows + wave_steps_*, crt_scene_desc.build_flags, crt_bvh_info build times */

typedef enum crt_status {
    CRT_OK = 0,
    CRT_ERR_INVALID = -1,     /* bad argument / inconsistent buffers           */
    CRT_ERR_NO_DEVICE = -2,   /* no HIP device: the product path refuses to run */
    CRT_ERR_HIP = -3,         /* a HIP runtime call failed                      */
    CRT_ERR_IO = -4,          /* file not found / parse failure                 */
    CRT_ERR_LIMIT = -5,       /* a structural limit was exceeded (stack depth…) */
    CRT_ERR_NOMEM = -6
} crt_status;

/* ---------------------------------------------------------------- layouts -- */

/* Caitlyn/Triangle.h:19-27 — 48-byte index record, uploaded RGBA32I ×3
 * (Scene.h:1036-1041).  v = (i0,i1,i2,material); vn = (n0,n1,n2,1) or the integer-
 * truncated geometric normal with w=0 (Scene.h:849-852); vt = (t0,t1,t2,0). */
typedef struct crt_triangle { int32_t v[4]; int32_t vn[4]; int32_t vt[4]; } crt_triangle;

/* Caitlyn/FlatNode.h:34-40 — 32-byte BVH2 node, uploaded RGBA32F ×2
 * (Scene.h:1057-1062).  Interior: bmin[3]=left child (right=left+1), bmax[3]=0.
 * Leaf: bmin[3]=first triangle slot, bmax[3]=count (>=1).  Links are floats. */
typedef struct crt_flatnode { float bmin[4]; float bmax[4]; } crt_flatnode;

/* Caitlyn/cwbvh.h:11-25 == Shader/cwbvh.fs:355-362 — 80-byte compressed 8-wide
 * node, five 16-byte rows exactly as the shader fetches them (cwbvh.fs:484-488). */
typedef struct crt_node8 {
    float    p[3];               /* quantisation origin                          */
    uint8_t  e[3];               /* biased exponents, scale = 2^(e-127)          */
    uint8_t  imask;              /* bit i <=> slot i is an inner child           */
    uint32_t child_base_index;
    uint32_t triangle_base_index;
    uint8_t  meta[8];
    uint8_t  qlo_x[8], qhi_x[8];
    uint8_t  qlo_y[8], qhi_y[8];
    uint8_t  qlo_z[8], qhi_z[8];
} crt_node8;

/* Caitlyn/Scene.h:75-85 — 64-byte material, RGBA32F ×4 (Scene.h:1043-1048). */
typedef struct crt_material { float albedo[4]; float emission[4]; float specular[4]; float tex_ind[4]; } crt_material;

/* Caitlyn/Scene.h:151-166 — 72-byte light, RGB32F ×6 (Scene.h:1050-1055):
 * p,u,v,n,e,(area,pdf,0). */
typedef struct crt_light { float p[3], u[3], v[3], n[3], e[3], area_pdf[3]; } crt_light;

/* camera uniform block, Scene.h:1143-1149 / :1237-1243 (fov = vertical, radians).
 * aperture == 0 is the pinhole camera of path_trace.fs:1026-1047; focal_dist is then not looked at.
 * aperture > 0 is a thin lens (no reference counterpart: the shader uploads the two uniforms and never reads them).  The lens
 * is a disc of radius `aperture`, in world units, in the plane spanned by right and up through position; the plane of focus is the plane
 * whose coordinate along forward equals focal_dist.  Per pixel-sample, every step one IEEE float32 operation under DESIGN.md §3's rules (no
 * contraction; dot, normalize, the correctly rounded sqrt and the pinned sine / cosine as the bounce sampler uses them):
 *   v   = (right*dx + up*dy) + forward     the pinhole's direction before normalize(), jitter included (path_trace.fs:1041-1046)
 *   u1  = rand();  u2 = rand();            two MORE draws of the shader RNG, directly behind the two jitter draws (option "jitter" 0: the
 *                                          path's first two draws)
 *   r   = aperture * sqrt(u1);  phi = 6.2831853f * u2;
 *   lx  = r * cos(phi);  ly = r * sin(phi);
 *   lo  = right*lx + up*ly;                per component (right.k*lx) + (up.k*ly)
 *   o   = position + lo;
 *   d   = normalize(v*focal_dist - lo);    per component (v.k*focal_dist) - lo.k
 * and the path's RNG state goes on behind u2; everything after the primary ray is unchanged.  No case is special: a basis that is not
 * orthonormal gives what this arithmetic gives, as for the pinhole.  crt_render_frame(s) through a lens adds what the definition above
 * gives, bit for bit, on flat and instanced scenes, for every option that does not change a pinhole frame's sums either; frames run as a
 * chain of queue-fed segments behind a ray-generation launch (crt_debug_launch_info bit 4) and take no part in the adaptive tile order.
 * crt_set_camera refuses (CRT_ERR_INVALID, crt_last_error names the field, the previous camera stays, on every device of the scene): an
 * aperture that is NaN, infinite or negative; with aperture > 0, a focal_dist that is not finite and > 0.
 * The feature buffers, the denoiser's guides and the temporal reprojection keep the PINHOLE view through position (see there). */
typedef struct crt_camera {
    float position[3]; float right[3]; float up[3]; float forward[3];
    float fov; float focal_dist; float aperture;
} crt_camera;

/* explicit ray / hit records for crt_trace (no reference counterpart). */
typedef struct crt_ray { float o[3]; float tmax; float d[3]; uint32_t pad; } crt_ray;          /* 32 B */
typedef struct crt_hit { float t, u, v; int32_t tri; } crt_hit;   /* tri = original triangle id, -1 = miss */
typedef struct crt_ray_stats { uint16_t nodes, tris; } crt_ray_stats;  /* per-ray visit counters (optional) */

/* crt_trace mode = CLOSEST or ANY, optionally OR-ed with:
 *   CRT_TRACE_BVH2          walk the BVH2 exactly as the shipped shader does (path_trace.fs:511-819:
 *                           FlatNode array, near child first, raw 1/d) instead of the CWBVH;
 *   CRT_TRACE_TIE_LOWEST_ID with BVH2: equal-t hits resolve to the lowest original id (the CWBVH path's rule)
 *                           instead of the shader's first-visited rule (path_trace.fs:363). */
enum { CRT_TRACE_CLOSEST = 0, CRT_TRACE_ANY = 1, CRT_TRACE_BVH2 = 2, CRT_TRACE_TIE_LOWEST_ID = 4 };

/* Everything Scene::gpu_data uploads (Scene.h:1015-1078) plus the intended bvh8
 * buffer.  All pointers are HOST memory and are COPIED (the reference frees its CPU
 * vectors right after upload, Scene.h:503).  `triangles` are in BVH2 leaf order with
 * spatial-split duplicates (sbvh.h:130-139).  Either `bvh` (BVH2; converted to CWBVH
 * on the host) or `bvh8` + `bvh8_tri_slots` must be given; both may be — or neither, with
 * build_flags = CRT_BUILD_LBVH_ON_DEVICE (below). */
typedef struct crt_scene_desc {
    uint32_t abi_version;               /* CRT_ABI_VERSION */
    const float*        vertices;   size_t n_vertices;   /* xyz, 12 B   Scene.h:1015-1020 */
    const float*        normals;    size_t n_normals;    /* xyz         Scene.h:1022-1027 */
    const float*        texcoords;  size_t n_texcoords;  /* uv          Scene.h:1029-1034 */
    const crt_triangle* triangles;  size_t n_triangles;  /*             Scene.h:1036-1041 */
    const int32_t*      tri_orig_ids;                    /* sbvh.h:136-137 triangle_indices; NULL -> slot id */
    const crt_material* materials;  size_t n_materials;  /*             Scene.h:1043-1048 */
    const crt_light*    lights;     size_t n_lights;     /*             Scene.h:1050-1055 */
    const crt_flatnode* bvh;        size_t n_bvh;        /*             Scene.h:1057-1062 */
    const crt_node8*    bvh8;       size_t n_bvh8;       /* intended bvh8 buffer (cwbvh.fs:484) */
    const int32_t*      bvh8_tri_slots; size_t n_bvh8_tris; /* CWBVH triangle order -> slot in `triangles` */
    const uint8_t*      albedo_textures; uint32_t tex_width, tex_height, n_textures; /* RGB8 array, Scene.h:1065-1078 */
    uint32_t width, height;             /* screenResolution, Scene.h:1151 */
    uint32_t max_depth;                 /* path segments; the shader hard-codes 3 (path_trace.fs:867) */
    uint32_t build_flags;               /* CRT_BUILD_*: 0 unless neither bvh nor bvh8 is given */
} crt_scene_desc;

/* crt_scene_desc.build_flags.  With CRT_BUILD_LBVH_ON_DEVICE (bvh == bvh8 == NULL) `triangles` come in SOURCE order
 * (tri_orig_ids must be NULL: a triangle's id is its index) and everything Scene::build_bvh (Scene.h:929-958) and the
 * intended CWBVH::convert would have produced on the host is produced in HBM instead: linear BVH (crt_lbvh_build's
 * kernels), CWBVH conversion (crt_cwbvh_convert_device's kernels: same bytes as the host converter), leaf-order
 * triangle array and intersection records.  Only the seven input arrays cross PCIe, once.  The tree is the LBVH, not
 * the reference's SBVH; frames are bit-identical to a scene created from crt_lbvh_build's host arrays. */
enum { CRT_BUILD_LBVH_ON_DEVICE = 1,
       /* with CRT_BUILD_LBVH_ON_DEVICE: build the tree by PLOC (CRT_GPU_BUILD_PLOC of crt_lbvh_build) instead of the linear
        * BVH; bits 8..15 = search radius, 0 = 16 */
       CRT_BUILD_PLOC = 2,
       /* with CRT_BUILD_LBVH_ON_DEVICE: the binned-SAH builder (CRT_GPU_BUILD_SAH) */
       CRT_BUILD_SAH = 4 };

typedef struct crt_scene crt_scene;

/* ------------------------------------------------- device path (needs GPU) -- */

/* replaces Scene::gpu_data, Scene.h:1000-1156 */
int crt_scene_create(const crt_scene_desc* desc, crt_scene** out);
/* replaces Scene::delete_gpu_data / delete_tex_data, Scene.h:978-998 */
int crt_scene_destroy(crt_scene* s);
/* replaces Scene::update, Scene.h:1233-1246 */
int crt_set_camera(crt_scene* s, const crt_camera* cam);
/* Environment lighting: radiance for path rays that leave the scene (no reference counterpart: RenderOptions carries environment-map
 * knobs that nothing reads).  Without an environment such a ray ends its path with nothing.
 * The environment is a square OCTAHEDRAL map of size x size RGB float texels, a 3x3 matrix and an RGB scale.  The map's +z is the centre
 * texel and -z the four corners; row 0 is the lowest py.  For a ray direction d, every line one IEEE float32 operation in the written
 * order under DESIGN.md §3's rules (no contraction):
 *   e    = (R[0].d, R[1].d, R[2].d)           each (r0*d.x + r1*d.y) + r2*d.z;  R = rotation, rows, world -> map
 *   s    = (|e.x| + |e.y|) + |e.z|            not (s > 0), or s not finite: the radiance is 0, done
 *   px   = e.x / s;  py = e.y / s
 *   if e.z < 0:  (px, py) = ((1 - |py|) * sgn(px), (1 - |px|) * sgn(py))      from the OLD px, py; sgn(x) = x < 0 ? -1 : 1
 *   fx   = (px * 0.5 + 0.5) * size - 0.5;  fy likewise
 *   i0   = floor(fx), tx = fx - i0;  j0 = floor(fy), ty = fy - j0;  i1 = i0 + 1, j1 = j0 + 1
 *   tap(i, j):  if i < 0: (i, j) = (0, size-1-j)   else if i > size-1: (i, j) = (size-1, size-1-j)
 *               then if j < 0: (i, j) = (size-1-i, 0)   else if j > size-1: (i, j) = (size-1-i, size-1)
 *               then both clamped to [0, size-1]                 (the octahedral edge identification: the filter has no seam)
 *   c    = (tap(i0,j0)*(1-tx) + tap(i1,j0)*tx)*(1-ty) + (tap(i0,j1)*(1-tx) + tap(i1,j1)*tx)*ty        per channel
 *   E(d) = c * scale                                                                                    per channel
 * Integrator rule: when a path's closest-hit ray misses in segment k, the path adds T * E(d) and ends; T is the throughput it carries into
 * that segment, d that ray's direction, and the weight is 1 for every path, specular or not.  Nothing samples the environment from a
 * surface (no environment NEE: a small bright sun is noisy), and misses are disjoint from the emitters of the light table, so the estimator
 * is unbiased as it stands.  The addition is made in segment order, as the path's last, behind every earlier segment's emitter and NEE
 * terms.  With CRT_ENV_HIDE_FROM_CAMERA segment 0's misses add nothing: the environment lights the scene without showing as a backdrop.
 * Nothing else about a frame changes — rays, RNG stream, NEE, MIS, materials, resolve —, and with no environment set every frame is what
 * it was, through the same launches.
 * Works on flat scenes and on crt_scene_create_instanced[_lit] scenes, with crt_set_devices (every device gets the map; a refused call
 * leaves every device's previous environment in place), crt_set_shard and option "streams".  Scene state like the camera: it survives
 * crt_reset, and changing it does not clear the sum (the caller resets, as after crt_set_camera).  env == NULL removes it.
 * A frame with an environment runs as a chain of queue-fed segments behind a ray-generation launch, k_env_miss between each segment's
 * closest-hit launch and its shade-only pass, every segment's shadow rays deferred (crt_debug_launch_info bit 5); a pinhole camera
 * renders crt_render_frames one sample per chain, a lens keeps its chains of up to 8.  It takes no part in the adaptive tile order.
 * CRT_ERR_INVALID, crt_last_error names the field, nothing stored: null scene; null texels; size outside 1..4096; a texel, scale or
 * rotation entry that is not finite; a negative texel or scale; unknown flags bits; non-zero reserved; a scene in the BVH2 frame mode
 * (option "accel" not 0).
 * Out of scope: importance-sampled environment NEE with MIS; a fused environment arm in the first-segment kernels; environment-aware
 * feature buffers or denoiser guides; HDR file decoding (crt_image_decode keeps refusing .hdr); batched pinhole samples in one chain; any
 * environment in the C oracle or the BVH2 frame mode. */
#define CRT_ENV_HIDE_FROM_CAMERA 1u
typedef struct crt_environment {
    const float* texels;      /* size*size*3 floats, RGB, row 0 first */
    uint32_t size;            /* 1..4096 */
    uint32_t flags;           /* CRT_ENV_HIDE_FROM_CAMERA or 0; other bits refused */
    float rotation[9];        /* rows; world -> map */
    float scale[3];
    uint32_t reserved[2];     /* must be 0 */
} crt_environment;
int crt_set_environment(crt_scene* s, const crt_environment* env);
/* Frames along the CALLER's camera rays: replaces the shader's ray set-up, path_trace.fs:1026-1047, with rays read from memory (no reference
 * counterpart: the shader has the one pinhole).  For a panorama, an orthographic or fisheye view, a stereo pair, a cube face,
 * radiance at lightmap texels or probe directions (a probe or a bake is a scene of width = n, height = 1), or the caller's own sub-pixel
 * filter: everything behind the primary ray — integrator, RNG, materials, lights, environment — stays the library's.
 *   `rays` holds width*height entries of crt_ray (32 bytes); the entry of pixel (px, py) is at py*width + px, rows as crt_read_sum's.
 *   The call COPIES the entries into a buffer the scene owns: allocated by the first call, reused by later ones, freed with the scene.
 *   Both set entries wait for the scene's stream(s) before the copy and for the copy after it: the caller's memory is free on return, and
 *   a frame enqueued earlier keeps the rays it was enqueued with.  crt_clear_camera_rays waits the same way.
 * While camera rays are set, crt_render_frame[s][_async] takes the primary ray of pixel-sample (px, py) as
 *   o = entry.o;  d = entry.d;  tmax = 1e9f
 * AS GIVEN: d is not normalised (the caller supplies unit directions; a non-unit d gives what the arithmetic gives), entry.tmax and
 * entry.pad are not read.  The path's RNG state is the pixel's initial state (px + 0.5, py + 0.5) with NO draw consumed, whatever option
 * "jitter" says — the state the pinhole's ray set-up leaves with "jitter" 0 —, and every sample of a chain uses the same rays with its own
 * rv = rx*ry.  The path starts as every path does: L = 0, pdf = 1, T = 1, the specular flag.  The camera's position, basis, fov, aperture
 * and focal_dist are not read by such a frame: crt_set_camera still stores them and changes no byte of it, and need not have been called.  Camera rays equal to the
 * pinhole's "jitter" 0 rays give the pinhole's "jitter" 0 frames, bit for bit.
 * An entry WITHOUT A PATH: if any component of o or d is not finite, or d == (0, 0, 0), that pixel-sample emits no ray, adds +0 to the
 * pixel's sum and counts in no ray statistic (crt_frame_stats.closest_rays of such a frame counts segment 0's emitted rays).  The outside
 * of a fisheye circle, uncovered lightmap texels, garbage in device memory that no host check can see.
 * crt_clear_camera_rays is always allowed; the next frame is the camera's again: the fused first-segment path, with a fresh scene's launch
 * form and bytes.
 * A frame along camera rays runs as a chain of queue-fed segments behind a ray-generation launch, as a lens frame does, up to 8 samples per
 * chain (crt_debug_launch_info bit 6; bits 0-4 clear), on flat and instanced scenes, with crt_set_shard, option "streams", an environment,
 * and every option that does not change a lens frame's sums; it takes no part in the adaptive tile order.  The rays win over aperture > 0.
 * CRT_ERR_INVALID, crt_last_error names the field, nothing stored, an earlier ray set stays in force: null scene; null rays;
 * n != width*height; a scene on several devices (crt_set_devices with more than one) — and while camera rays are set, crt_set_devices with
 * more than one device is refused too.
 * The calls that see the scene through the pinhole — crt_render_aov, crt_render_ao, crt_render_fog, crt_denoise (its guides are those
 * buffers) and crt_temporal (it reprojects through the camera) — are refused with CRT_ERR_INVALID ("camera rays") while camera rays are
 * set, and leave their earlier images untouched: a panorama filtered against pinhole guides would be a silent wrong answer.
 * crt_ao_points*, crt_fog_segments*, crt_trace*, crt_resolve*, crt_display, crt_bloom, crt_fog_composite, refit, rebuild and deform are
 * unaffected.
 * Out of scope: feature buffers, AO and fog view modes, denoising and temporal accumulation along camera rays; a per-entry tmax; borrowing
 * the caller's buffer instead of copying; several devices; a fused first-segment arm; batched samples for instanced frames; any of it in
 * the C oracle. */
int crt_set_camera_rays(crt_scene* s, const crt_ray* rays, size_t n);          /* host pointer */
int crt_set_camera_rays_device(crt_scene* s, const void* d_rays, size_t n);    /* device pointer, same layout */
int crt_clear_camera_rays(crt_scene* s);
/* replaces the path_trace draw in Scene::Render, Scene.h:1208-1213: adds ONE sample
 * per pixel to the device-resident RGB32F sum buffer; (rx,ry) = randomVector. */
int crt_render_frame(crt_scene* s, float rx, float ry);
/* same, without the final stream synchronise: frames queue back to back on the scene's
 * stream; crt_sync (or any read-back call) waits for them. */
int crt_render_frame_async(crt_scene* s, float rx, float ry);
/* n consecutive frames: exactly what n calls of crt_render_frame with (rx[i], ry[i]) add to the sum buffer, bit for bit.
 * With the shadow rays walked in place (the default) up to 8 of them share a launch: on a one-segment path (max_depth 1)
 * each lane renders its pixel's samples one after the other — or, where the launch has too few waves to fill the GPU (a shard
 * from crt_set_shard, a small frame), the samples run side by side on the waves of a workgroup and are added in frame order
 * (option "wave_samples"); on longer paths every sample keeps its own path state and
 * queue entries, all samples' rays go through each segment's launch together, and a last kernel adds the samples'
 * radiance to the sum in frame order (the extra buffers, ~250 B per pixel and frame of the batch, are allocated by the
 * first such call).  That saves the launch gaps and kernel tails between frames (1 M triangles: 0.246 -> 0.235 ms per
 * frame at max_depth 1, 1.78 -> 1.45 ms at max_depth 4).  Otherwise (shadow queue, bounce pools, counting frames) the
 * frames are simply queued one by one.  crt_get_frame_stats then describes the last launch (ray and visit counts summed
 * over the samples it rendered). */
int crt_render_frames(crt_scene* s, uint32_t n, const float* rx, const float* ry);
int crt_render_frames_async(crt_scene* s, uint32_t n, const float* rx, const float* ry);
int crt_sync(crt_scene* s);
/* Options (name, value).  Results never depend on the tuning options: every combination is bit-identical.
 * A frame with an environment (crt_set_environment) has one launch form: "inplace_shadow", "bounce_refill" and "ray_bins" are accepted and
 * do not apply to it, and "accel" other than 0 is refused while an environment is set.
 *   behaviour
 *     "jitter"            0/1 tent-filter jitter of path_trace.fs:1030-1037 (default 1)
 *     "accel"             what crt_render_frame walks: 0 = the CWBVH (default); 1 = the BVH2 exactly as the shipped
 *                         shader walks it (path_trace.fs:511-819, first visited triangle wins a tie); 2 = the BVH2 with
 *                         the lowest-id tie rule; 1 and 2 need desc.bvh
 *   telemetry
 *     "count_visits"      0/1: traversal launches also count node fetches / triangle tests (crt_frame_stats), frame by frame; 2: counting
 *                         frames may share a launch in the form the timed launches have (crt_render_frames of four frames: four samples
 *                         of a 4x4 pixel quadrant in the lanes of a wave) — what the uniform node steps see depends on which rays share a wave
 *     "adaptive_tiles"    1 (default): the order in which the tiles of the frame (16x16 pixels unless crt_set_shard says otherwise) are handed to the GPU follows their
 *                         measured cost, most expensive first (one frame per new view is timed, tile by tile); 0: centre-out
 *                         order only.  Which pixel lands where — in the image and in the sum buffer — does not depend on it.
 *     "timing"            HIP events behind crt_frame_stats.ms_* and n_trace_launches: 0 = none (default: the fields stay 0), 1 = closest-hit
 *                         launches only, 2 = every traversal launch.  The events ride on the dispatches; a timed dispatch costs ~5 us
 *                         of stream time because it cannot overlap its neighbours (8 % of a 1080p frame of the 32-triangle box)
 *     "timing_accumulate" n > 0: keep the spans of the next n launches instead of restarting every frame
 *                         (crt_frame_stats.ms_* are then sums over n_trace_launches launches); 0: per frame
 *   tuning
 *     "inplace_shadow"    the NEE shadow rays (path_trace.fs:968): 1 = walked inside the segment kernel; 2 = the first segment's in
 *                         place, the bounce segments' DEFERRED: they wait in the frame's NEE queue with the index of a contribution
 *                         slot (segment, path), ONE any-hit launch behind the last segment walks them all in full waves, an occluded
 *                         ray clears its slot, and a last kernel adds every path's slots in segment order — the additions the in-place
 *                         form makes, in the same order; 0 = every segment's deferred (frames then render one by one); 3 (default) = 2
 *                         for trees of 64+ nodes, else 1.  BVH2 frames ("accel") always walk in place.
 *     "shadow_pool"       rays per pool of that launch: 64, 128, 256 (default), 512: a lane whose ray has finished takes the pool's next
 *                         ray once "shadow_refill_min" (1..64, default 16; 65 = never: lock-step batches of 64) lanes are idle; the
 *                         pool's last eight rays get eight lanes each ("lanes_per_ray")
 *     "persistent"        1 (default): the pool launches (k_shadow_deferred, k_closest_queue) are PERSISTENT grids — as many single-wave
 *                         workgroups as the chip holds waves, each reserving chunks of "shadow_pool" / "refill_pool" rays from the
 *                         sub-queues through one cursor per queue until all are dry (one returning atomic per chunk), so the launch
 *                         ends on one drain phase instead of one per pool; 0: one workgroup per pool.  "shadow_waves" (1..8,
 *                         default 6): waves per SIMD k_shadow_deferred's grid is sized for (the kernel fits 8; the grids of the
 *                         shards on "streams" share the chip)
 *     "bounce_refill"     segments >= 1: 0 = closest hit, shading and emission fused in one lock-step kernel (default); 1 = closest hits
 *                         through pools of "refill_pool" (64 / 128 / 256 (default) / 512) rays per wave with lane refill at "refill_min"
 *                         idle lanes (k_closest_queue), then a shade-only pass (k_segment<PRETRACED>)
 *     "tri_min"           vote ratio of the closest-hit traversal loop (default 2); 0 = plain per-lane loop, which
 *                         trees under 64 nodes get anyway
 *     "lanes_per_ray"     8 (default) or 1: a lock-step batch starts with one ray per lane and ends on its longest rays (1 M triangles,
 *                         bounce segments: 37 % of the closest-hit node steps run with at most 8 of the 64 lanes enabled, 41 % of
 *                         the any-hit ones).  In the bounce segments' closest-hit and in-place shadow walks, once at most 8 rays of a
 *                         wave are still alive each of them is given 8 adjacent lanes: the 8 child tests of a node (independent,
 *                         cwbvh.fs:376-446) run one per lane, the pending triangles of a leaf side by side (4 segments: 5,420 ->
 *                         6,021 Mray/s; 8 M triangles 3,464 -> 3,909).  1 = one lane per ray throughout.
 *     "ray_bins"          bounce rays regrouped between segments (BASELINE configs[3], "sorting stress"): 0 (default) = per-group
 *                         sub-queues in emission order; 1 = the rays a segment emits are appended to 4096 bins keyed by (direction
 *                         octant, 8^3 cell of the origin) whose places in the queue follow the previous frame's counts, so the next
 *                         segment's 64-ray batches hold rays that start together and head the same way (wave-level traversal steps
 *                         -10 % on the 1 M-triangle frame; the append costs more than that saves: frame time +3.6 %); 2 / 3 = variants
 *                         of the append (one atomic per ray); 4 = the rays of a wave that share a bin find each other by ranking through a
 *                         wave-private LDS table (one ds_add_rtn per ray, one global atomic per bin); 5 = 1 for the first segment's
 *                         emission (a handful of bins per wave) and 4 for the bounce segments'
 *     "wave_samples"      crt_render_frames, first segment: where the samples of a launch run.  0 = one after the other in the wave
 *                         that owns the 8x8 pixel batch; 1 = side by side on the 2 to 4 waves of one workgroup, added to the sum in
 *                         sample order through LDS; 3 = four samples of a 4x4 pixel quadrant in the lanes of one wave (lane = sample x 16
 *                         + pixel; launches of 4 or 8 samples on trees of 64+ nodes, else 0), added in sample order through lane
 *                         shuffles: a wave's rays leave a quarter of the area, so they agree on their nodes like the rays of a frame of
 *                         twice the resolution (1 M triangles: +8.5 % / +12 % at 4 / 8 samples per launch); 2 (default) = 3 where it
 *                         applies, otherwise 1 when the launch would be bound by its longest waves — a shard of a frame, a small
 *                         frame — as judged from the measured tile costs, else 0.  The same bits every way.
 *     "wide_first"        which build of the first-segment kernel a launch runs: 0 = compiled for 5 waves per SIMD (96 VGPRs),
 *                         1 = for 6 (80 VGPRs), 2 (default) = 6 where the launch is bound by throughput, 5 where its longest
 *                         waves set its length (the same measure as "wave_samples"); the 6-wave build exists for the batched
 *                         launches of crt_render_frames on Lambert scenes
 *     "last_build"        1 (default) or 0: a one-pass launch of crt_render_frames (four samples in the lanes of a wave) that is the path's
 *                         last segment runs a build compiled as one — no bounce sampling, next-ray queue or path state in its code
 *                         (measured in profiles/r06_experiments.md); 0 = the build that finds out at run time.
 *                         The same operations either way: sums and visit counters keep their bits.
 *     "lean_build"        1 (default) or 0: such a last-segment launch (never a counting one) runs the LEAN form of its build where the
 *                         launch is what the form has compiled in — a tree that passed crt_scene_create's validator (stack pushes without
 *                         the overflow check), "tri_min" 2 and "lanes_per_ray" 8, no frame of tile-cost measurement —
 *                         with the RNG's sine in a form of fewer double-precision-rate instructions and the same bits (DESIGN.md
 *                         section 5; profiles/r07_experiments.md); 0 = the build without it.  The same sums either way.
 *     "denoise_form"      0 (default), 1 or 2: which form of its pass kernel crt_denoise runs: 0 = at each tap spacing the one measured
 *                         faster there, 1 = the taps staged in LDS, 2 = the taps read from global memory, at every
 *                         spacing.  The same bytes either way.
 *     "temporal_form"     0 (default), 1 or 2: how a crt_temporal call with CRT_TEMPORAL_CLAMP reads the 3 x 3 neighbourhood: 0 = the form
 *                         measured faster, 1 = staged in LDS once per 16 x 16 block, 2 = read from global memory by
 *                         every lane.  The same bytes either way.
 *     "streams"           1 (default) .. 4, or 0 = pick for me (3 for scenes of a few nodes, 2 for max_depth > 1, else 1): that many tile shards of the frame rendered side by side on streams of their own on this one GPU
 *                         (own queues and path state, the scene buffers shared).  A multi-segment frame is a chain of dependent
 *                         launches; another shard's launches fill their tails: 1 M triangles, 4 segments, 2 streams +6 %, 8 M triangles
 *                         +4 %; a one-segment frame gains nothing.  It is crt_set_devices with this GPU listed k times: the accumulated
 *                         sum restarts, crt_read_sum / crt_resolve / crt_sum_device assemble the frame.  A scene that renders a shard
 *                         (crt_set_shard, one process per GPU) can split that shard the same way — set the option after crt_set_shard;
 *                         its tiles are dealt to the streams and crt_packed_info / crt_read_packed / crt_copy_packed_device hand out the
 *                         shard's packed buffer assembled from the streams' parts (an eighth of the 4K frame, 4 segments: 88 -> 99 % of
 *                         perfect division).  crt_set_shard and crt_set_devices take the split away again.
 *     "trace_pool"        crt_trace / crt_trace_device: rays per wave, 64 (default: one lock-step batch per single-wave workgroup, the
 *                         finest grain for the dispatcher — 2.07 M primary rays of the 1 M-triangle scene 0.153 ms against 0.346),
 *                         128 or 256 (a pool: a lane whose ray has finished takes the pool's next ray once "refill_min" lanes
 *                         (default 8, 1..64; 65 = never while a lane is busy) are idle; worth 4 % on incoherent bounce rays, tools/refill_probe.py)
 *     "gather_transport"  scenes on several devices (crt_set_devices): 0 = RCCL send / recv (default when librccl.so loads and the
 *                         devices are distinct), 1 = hipMemcpyPeerAsync
 *   experimental (a library built with `make EXPERIMENTS=1`, crt_has_experiments() != 0; otherwise only the default value is
 *   accepted) — variants that lost every measurement and are kept for re-measurement, bit-identical like the rest:
 *     "oversubscribe"     0 = one 64-ray batch per workgroup, the hardware dispatcher balances (default); k >= 1 =
 *                         persistent grid of k x the resident workgroups with a static schedule, then
 *                         "trace_occupancy" = workgroups per CU
 *     "waves_per_workgroup" 1 (default), 2 or 4, per scene */
int crt_set_option(crt_scene* s, const char* name, int value);
/* replaces the camera-moved clear, Scene.h:1160-1172 */
int crt_reset(crt_scene* s);
/* path_trace_texture read-back: n_floats must be width*height*3 (bottom row first).
 * With a shard set, returns this rank's pixels only (others 0). */
int crt_read_sum(crt_scene* s, float* rgb, size_t n_floats);
/* the same frame left where the reference keeps it — in device memory, as the texture the output pass samples
 * (Scene.h:1226-1230): width*height*3 floats, bottom row first, on the scene's (first) device; with several devices this
 * is the gather + un-tile without the copy to the host.  The pointer stays valid until the next read-back call. */
int crt_sum_device(crt_scene* s, const float** d_rgb);
/* replaces the output pass, Shader/output.fs:9-20 + Scene.h:1226-1230:
 * rgba8 = pow(tonemap(sum*inv_count), 1/2.2), alpha 255; n_bytes = width*height*4 */
int crt_resolve(crt_scene* s, float inv_count, uint8_t* rgba, size_t n_bytes);
/* the same image left where the reference's output pass leaves it — in device memory (the default framebuffer, Scene.h:1226-1230): RGBA8,
 * width*height*4 bytes, bottom row first, on the scene's (first) device; un-tile and tone map in one pass over the packed tile buffers, no
 * copy to the host.  sync = 0: enqueued on the scene's stream (crt_sync waits for it).  The pointer stays valid until the next resolve.
 * The gamma is pinned (the byte = how many of 255 precomputed thresholds the tone-mapped value has reached), so the bytes of
 * crt_resolve / crt_resolve_device equal the CPU oracle's exactly. */
int crt_resolve_device(crt_scene* s, float inv_count, const uint8_t** d_rgba, int sync);
/* closest-/any-hit over an explicit HOST ray buffer (test/bench entry).
 * stats may be NULL.  For CRT_TRACE_ANY, hit.tri >= 0 iff occluded (t,u,v = 0). */
int crt_trace(crt_scene* s, const crt_ray* rays, size_t n, crt_hit* hits, int mode, crt_ray_stats* stats);
/* same with DEVICE pointers (rays/hits/stats already resident in HBM); asynchronous
 * on the scene's stream unless sync != 0. */
int crt_trace_device(crt_scene* s, const void* d_rays, size_t n, void* d_hits, int mode, void* d_stats, int sync);

/* First-hit feature buffers (AOVs) of the scene's current view, flat and instanced scenes (no reference counterpart): what
 * a denoiser, a picker or an id mask needs of the pixel's FIRST hit, bit for bit what the integrator computes there.  The rays are the
 * primary rays of crt_render_frame(s, rx, ry): the scene's camera, its "jitter" option, tmax 1e9f.  Every channel is 16 bytes per pixel
 * in linear pixel order (py * width + px, rows as crt_read_sum has them), allocated by the first call that asks for it, freed with the scene:
 *   HIT       crt_hit: (t, u, v, tri) of the closest hit (a flat scene: crt_trace's closest hit, lowest-id ties; an instanced scene: what
 *             crt_instances_trace gives, tri = the id within the mesh; with option "instance_masks" 1 the masked walk with
 *             "mask_primary", as segment 0 of a frame); a miss, or a pixel another shard rank owns: (1e9f, 0, 0, -1)
 *   IDS       int32[4]: (instance, mesh, material, flags); (-1, -1, -1, 0).  A flat scene reports instance = mesh = 0.  material: the index
 *             the integrator reads, triangles[..].v[3] plus the instance's material_offset.  flags: bit 0 the normal was flipped (dot(d, n)
 *             > 0 before the flip), bit 1 the material is emissive (emission.w != -1), bit 2 the albedo came from a texture
 *   NORMAL    float[4]: (n, 0), the shading normal as the integrator holds it after the face-forward flip: the flat triangle normal when
 *             vn.w == 0, else the interpolated one; through a non-identity instance by item 4 of crt_scene_create_instanced; NOT
 *             normalised (it keeps the file's length); zeros
 *   ALBEDO    float[4]: (rgb, 0), what the Lambert branch multiplies into the throughput: materials[4 m].xyz, or the filtered texture at
 *             the interpolated texcoord through pow(c, 2.2f) where the frame would use the texture; also for emissive materials; zeros
 *   EMISSION  float[4]: (materials[4 m + 1].xyz, 0) of an emissive material, else zeros
 * crt_render_aov is enqueued on the scene's stream behind any *_async frames (sync = 0 returns at once; crt_sync, crt_read_aov and later
 * frames are ordered behind it) and renders the channels named; a channel not named keeps its contents.  It leaves the sum, the frame
 * count, crt_get_frame_stats, the launch times and every frame's path and RNG state as they are.  An instanced scene reads its handle's
 * live arrays at enqueue, as a frame does: a set / refit / update_meshes before the call is seen, without crt_reset.  crt_set_shard works
 * (a rank fills its own pixels); option "streams" is ignored.  CRT_ERR_INVALID, nothing written: channels 0 or with other bits; option
 * "accel" not 0; a scene on several devices (crt_set_devices); crt_read_aov / crt_aov_device with a channel never rendered, more than
 * one bit, or n_bytes other than width*height*16.  crt_aov_device waits for the stream and leaves the array on the device; the pointer
 * stays valid until the scene is destroyed.
 * The view is the PINHOLE through the camera's position whatever its aperture: every channel is byte for byte independent of
 * crt_camera.aperture and focal_dist.  Behind a lens the buffers are therefore sharper than the image: they show the surface on the
 * central ray of each pixel, not the mix of surfaces an out-of-focus pixel gathers (lens-aware feature buffers are out of scope).
 * An environment (crt_set_environment) changes no channel: the call is unaware of it and miss pixels keep the values they have without. */
enum { CRT_AOV_HIT = 1, CRT_AOV_IDS = 2, CRT_AOV_NORMAL = 4, CRT_AOV_ALBEDO = 8, CRT_AOV_EMISSION = 16, CRT_AOV_ALL = 31 };
int crt_render_aov(crt_scene* s, float rx, float ry, uint32_t channels, int sync);
int crt_read_aov(crt_scene* s, uint32_t channel, void* dst, size_t n_bytes);
int crt_aov_device(crt_scene* s, uint32_t channel, const void** d_ptr);

/* Ambient occlusion of the scene's current view, or of points the caller names, flat and instanced scenes (no reference counterpart;
 * DESIGN.md §32): how open a surface point is to its surroundings.  K cosine-distributed rays leave each point; the result is the share
 * that escapes and the sum of the escaping directions (the caller normalises it for a bent normal).  The rays are built on the device where
 * they are walked and never stored; the count is an integer, so the result is defined bit for bit:
 * every line below is ONE IEEE float32 operation in the written order under DESIGN.md §3 (no contraction); dot, normalize, the correctly
 * rounded sqrt, pinned_sin and pinned_cos are the bounce sampler's.  F(x) = x rounded to float32.
 *
 * An AO POINT is crt_ao_point: (p[3], seed_x, n[3], seed_y), 32 bytes, laid out like crt_ray.  crt_ao_params: samples K in 1..256; radius
 * finite and > 0, 1e9f meaning "unbounded" as the integrator's tmax; offset finite and >= 0 (0.0002f is the integrator's hit-point offset);
 * flags = 0; reserved = 0.  NULL params mean {16, 0, 1e9f, 0.0002f}.  rv = rx * ry, as in a frame.  Per point:
 *   1. Normal.  l2 = dot(n, n).  If l2 is not > 0, or l2 or any component of p is not finite, the result is (0, 0, 0, -1) and no ray is
 *      traced.  Otherwise nn = n * (1 / sqrt(l2)).
 *   2. Origin.  o = p + nn * offset, per component F(p.k + F(nn.k * offset)).
 *   3. Basis, a correct Frisvad basis (NOT the integrator's onb(), which keeps path_trace.fs:56-57 as the reference wrote them):
 *      if nn.z < -0.9999999f: bu = (0, -1, 0), bv = (-1, 0, 0); otherwise a = 1 / (1 + nn.z); b = (-nn.x * nn.y) * a;
 *      bu = (1 - (nn.x*nn.x)*a, b, -nn.x); bv = (b, 1 - (nn.y*nn.y)*a, -nn.y).
 *   4. Random numbers, by index.  rand_at(j), j = 1, 2, ...: ax = seed_x - F(F(j) * rv); ay = seed_y - F(F(j) * rv);
 *      d = F(ax*12.9898f) + F(ay*78.233f); v = pinned_sin(d) * 43758.5453f; the value is v - floor(v).  j = 1 is the shader's first draw
 *      from that seed.  Sample k (0-based) uses u1 = rand_at(2k+1) and u2 = rand_at(2k+2).
 *   5. Direction.  r = sqrt(u1); phi = 6.2831853f * u2; sx = r*cos(phi); sy = r*sin(phi); sz = sqrt(1 - u1);
 *      sd = (bu*sx + bv*sy) + nn*sz.  Ray k is crt_ray{o, tmax = radius, d = sd}.
 *   6. Occlusion.  Ray k is occluded iff crt_trace(.., CRT_TRACE_ANY) reports a hit for that crt_ray; an instanced scene:
 *      crt_instances_trace(.., CRT_TRACE_ANY) on the scene's handle as it is at enqueue, with option "instance_masks" 1
 *      | CRT_TRACE_INSTANCE_MASK with the ray mask "mask_shadow".
 *   7. Result.  V = the number of unoccluded rays.  b = (+0, +0, +0); for k = 0 .. K-1 in that order, b = b + sd_k for each unoccluded k.
 *      The output float[4] is (b.x, b.y, b.z, F(V) / F(K)).
 *
 * VIEW MODE, crt_render_ao(s, rx, ry, params, sync): the points are the first hits of crt_render_aov(s, rx, ry, ..): the same rays (the
 * scene's camera, the "jitter" option, the pinhole through `position` whatever the aperture, the masked walk with "mask_primary" where that
 * applies); p = o_cam + d * t per component F(o.k + F(d.k * t)), in world space; n = the NORMAL channel's value (face-forwarded, through
 * the instance's transform, not normalised); (seed_x, seed_y) = the pixel's RNG state BEHIND the primary ray's draws: the pixel centre
 * (px + 0.5, py + 0.5) with "jitter" 0, the state after the two jitter draws with "jitter" 1.  A miss pixel holds (0, 0, 0, -1).  The image
 * is width*height float[4] in linear pixel order, rows as crt_read_sum has them, allocated by the first call and freed with the scene.
 * POINTS MODE, crt_ao_points (host pointers; returns when `out`, n x float[4], is written) and crt_ao_points_device (device pointers):
 * the same bytes as view mode gives for the same points.  n = 0 succeeds and writes nothing.
 * crt_read_ao wants n_floats = width*height*4.  crt_ao_device waits for the stream; the pointer stays valid until the scene is destroyed.
 *
 * The calls are enqueued on the scene's stream behind any *_async frames (sync = 0 returns at once); later frames and reads are ordered
 * behind them.  The sum, the frame count, crt_get_frame_stats, the launch times, every AOV channel and every frame's path and RNG state stay as
 * they are.  An instanced scene reads its handle's live arrays at enqueue.  An environment changes nothing.
 * CRT_ERR_INVALID, crt_last_error names the field, nothing written and an earlier AO image untouched: a null scene; a null points or out
 * pointer with n > 0; samples outside 1..256; a radius not finite or <= 0; an offset not finite or < 0; flags or reserved not 0; n * K or
 * width*height*K >= 2^32; option "accel" not 0; a shard of a frame (crt_set_shard with world > 1); a scene on several devices or streams
 * (crt_set_devices, option "streams"); crt_read_ao / crt_ao_device before any crt_render_ao, or n_floats of another size.
 * Out of scope: accumulating AO over calls (the caller averages); AO as a source of crt_denoise / crt_temporal / crt_display; lens-aware
 * points; shards and several devices; distance falloff; any AO in the C oracle. */
typedef struct crt_ao_point { float p[3]; float seed_x; float n[3]; float seed_y; } crt_ao_point;
typedef struct crt_ao_params { uint32_t samples; uint32_t flags; float radius; float offset; uint32_t reserved[4]; } crt_ao_params;
int crt_render_ao(crt_scene* s, float rx, float ry, const crt_ao_params* params, int sync);
int crt_read_ao(crt_scene* s, float* dst, size_t n_floats);
int crt_ao_device(crt_scene* s, const float** d_ptr);
int crt_ao_points(crt_scene* s, const crt_ao_point* points, size_t n, float rx, float ry, const crt_ao_params* params, float* out);
int crt_ao_points_device(crt_scene* s, const void* d_points, size_t n, float rx, float ry, const crt_ao_params* params, void* d_out, int sync);

/* Denoise a low-sample frame on the device, guided by the feature buffers (no reference counterpart): an edge-avoiding
 * a-trous wavelet filter over the scene's running sum, flat and instanced scenes.  Inputs: the sum, un-tiled as crt_sum_device has it and
 * scaled by inv_count, and the channels HIT, IDS, NORMAL and ALBEDO as the most recent crt_render_aov left them.  Keeping those channels in
 * step with the view and the geometry is the CALLER's duty, as inv_count already is: after a camera change, a refit or an instance move,
 * call crt_render_aov again before crt_denoise.  `passes` passes of a 5 x 5 B3-spline kernel, tap spacing 2^i in pass i; a tap counts by
 * the normals' cosine raised to 2^normal_power_log2, by its depth difference against sigma_depth * t * (tap distance), by its colour
 * difference against sigma_color / 2^i (0 = no colour term), and not at all across instances, misses, emitters seen directly or
 * degenerate normals: such pixels keep their own mean.  CRT_DENOISE_DEMODULATE filters radiance / max(albedo, 1e-3) and multiplies the
 * albedo back, so texture detail passes through.  Every step is one IEEE float32 operation in a fixed order: DESIGN.md §22 is the
 * definition, and the result is the same bytes on every build.  Non-finite radiance in the sum gives unspecified values in the pixels
 * whose taps reach it.
 * crt_denoise is enqueued on the scene's stream behind any *_async frames and crt_render_aov calls (sync = 0 returns at once; crt_sync, the
 * read calls below and later frames are ordered behind it).  It leaves the sum, the frame count, crt_get_frame_stats, the launch times,
 * every AOV channel, every frame's path and RNG state and crt_resolve_device's buffer as they are.  It does rewrite the un-tiled sum that
 * crt_sum_device's pointer names, as every crt_read_sum / crt_sum_device does: that array then holds the sum as of this call.  Its own
 * buffers are allocated by a scene's first crt_denoise and freed with the scene.  params NULL = {5, CRT_DENOISE_DEMODULATE, 4.0f, 0.05f, 7}.
 * crt_read_denoised: width*height*3 floats, rows as crt_read_sum has them, MEAN radiance (not a sum).  crt_denoised_device waits for the
 * stream and leaves that image on the device; the pointer stays valid until the scene is destroyed.  crt_resolve_denoised /
 * crt_resolve_denoised_device: crt_resolve's tone map and pinned gamma on that image (inv_count 1), the latter into a buffer of its own:
 * crt_resolve_device's pointer and bytes stay valid.
 * CRT_ERR_INVALID, nothing written: null scene; inv_count not finite or <= 0; passes outside 1..6; unknown flag bits; non-zero reserved;
 * a sigma outside its range or not finite; normal_power_log2 > 10; one of the four channels never rendered; a shard of a frame
 * (crt_set_shard with world > 1) or a scene on several devices (a filter needs its neighbours); a read, device or resolve call before any
 * successful crt_denoise, or with a wrong size.
 * A camera with an aperture: the guides are crt_render_aov's, i.e. the pinhole view through the camera's position.  Out-of-focus regions
 * are therefore filtered against guides sharper than the image: the edge-stopping terms hold the blur back at edges the pinhole sees.
 * A stated limitation; lens-aware guides are out of scope.
 * An environment (crt_set_environment): the filter is unaware of it.  Miss pixels keep the guide values they have without one, so the
 * backdrop is filtered as one region of equal guides. */
enum { CRT_DENOISE_DEMODULATE = 1 };
typedef struct crt_denoise_params {      /* 32 bytes */
    uint32_t passes;             /* 1..6; pass i (from 0) has tap spacing s = 2^i */
    uint32_t flags;              /* CRT_DENOISE_DEMODULATE or 0; other bits refused */
    float    sigma_color;        /* 0 = no colour term; else finite, in [1e-6, 1e6]; halves every pass */
    float    sigma_depth;        /* finite, in [1e-6, 1e6] */
    uint32_t normal_power_log2;  /* 0..10: normal weight = max(0, dot of the unit normals)^(2^k) by k squarings */
    uint32_t reserved[3];        /* must be 0 */
} crt_denoise_params;
int crt_denoise(crt_scene* s, float inv_count, const crt_denoise_params* p, int sync);
int crt_read_denoised(crt_scene* s, float* rgb, size_t n_floats);
int crt_denoised_device(crt_scene* s, const float** d_rgb);
int crt_resolve_denoised(crt_scene* s, uint8_t* rgba, size_t n_bytes);
int crt_resolve_denoised_device(crt_scene* s, const uint8_t** d_rgba, int sync);

/* Accumulate displayed frames across camera and instance motion (no reference counterpart: the reference restarts its sum while
 * camera.isMoving): temporal accumulation by reprojection, flat and instanced scenes.  Per displayed frame: move things,
 * crt_reset, crt_render_frames (k samples), crt_render_aov, optionally crt_denoise, crt_temporal, crt_resolve_temporal_device.  crt_reset
 * does not touch the history: that is the point.
 * Per pixel: the first-hit point (the recorded view's primary ray at the pixel times HIT's t) is carried into the previous call's view,
 * through the instance's previous object_to_world where that changed; the previous result is gathered bilinearly from the up to four
 * pixels around it that show the same surface (the same instance, unit normals with a cosine of at least normal_min, a stored depth within
 * sigma_depth * t' of the reprojected one); with N' the gathered history length, N = min(N' + 1, max_history) and the result is
 * previous + (source - previous) / N.  A pixel without such a tap, one whose point lies behind or outside the previous view, one of an
 * instance index the previous call did not have, a miss, an emitter seen directly or a degenerate normal starts again at N = 1 with the
 * source.  CRT_TEMPORAL_DEMODULATE accumulates source / max(albedo, 1e-3) and multiplies the albedo back, so texture detail is not
 * smeared by the resampling; CRT_TEMPORAL_CLAMP clamps the gathered value to the source's range over the pixel and its eight neighbours of
 * the same instance (against ghosting when lighting changes).  max_history 1 gives the source itself.  Every step is one IEEE float32
 * operation in a fixed order: DESIGN.md §23 is the definition, and the result is the same bytes on every build.  Non-finite radiance in
 * the source gives unspecified values where it is blended in.
 * The source is crt_sum_device's image times inv_count (CRT_TEMPORAL_SOURCE_SUM), or crt_denoise's image as it is
 * (CRT_TEMPORAL_SOURCE_DENOISED; inv_count is then ignored but still checked).
 * The current view is the one the most recent crt_render_aov that rendered HIT was given, recorded on the host when that call was
 * enqueued: the camera, the aspect and field-of-view factors, rx * ry and the "jitter" option.  As for crt_denoise, keeping HIT, IDS,
 * NORMAL and ALBEDO in step with the view and the geometry is the CALLER's duty, and so is not moving instances between crt_render_aov
 * and crt_temporal: an instanced scene reads the handle's live object_to_world / world_to_object when crt_temporal is enqueued, as a
 * frame does, and keeps a copy of object_to_world (and the instance count) as "previous" for the next call.  The camera basis is assumed
 * orthonormal, as crt_camera_look_at makes it.  The previous normal is in the previous frame's world space and is not rotated: a spinning
 * instance loses its history once one call's rotation exceeds the normal_min cosine.
 * Out of scope: deforming geometry.  After crt_update_vertices, crt_rebuild_vertices, crt_instances_update_meshes or a mesh replace the
 * surface point is assumed not to have moved in object space; the depth and normal tests catch large moves, and a caller that deforms a
 * lot calls crt_temporal_reset.  No previous-vertex copy is kept.
 * crt_temporal is enqueued on the scene's stream behind any *_async frames, crt_render_aov and crt_denoise calls (sync = 0 returns at
 * once; crt_sync, the read calls below and later frames are ordered behind it).  It leaves the sum, the frame count, crt_get_frame_stats,
 * the launch times, every AOV channel, crt_denoise's buffers, crt_resolve_device's buffer and every frame's path and RNG state as they
 * are (source SUM rewrites the un-tiled sum that crt_sum_device's pointer names, as every crt_read_sum does).  Its own buffers are
 * allocated by a scene's first crt_temporal and freed with the scene; later calls allocate nothing.
 * The next call is history-less (every pixel N = 1) when it is the first, after crt_temporal_reset, and after a change of the DEMODULATE
 * bit between two calls.  params NULL = {CRT_TEMPORAL_DEMODULATE, CRT_TEMPORAL_SOURCE_SUM, 32, 0.1f, 0.9f}.
 * crt_read_temporal: width*height*3 floats, rows as crt_read_sum has them, MEAN radiance.  crt_read_temporal_history: width*height
 * floats, N per pixel.  crt_temporal_device waits for the stream and leaves the image on the device; the pointer stays valid until the
 * scene is destroyed.  crt_resolve_temporal / crt_resolve_temporal_device: crt_resolve's tone map and pinned gamma on that image
 * (inv_count 1), into a buffer of their own.
 * CRT_ERR_INVALID, nothing written and the history unchanged: null scene; inv_count not finite or <= 0; unknown flag bits; source > 1;
 * max_history outside 1..4096; sigma_depth or normal_min out of range or not finite; non-zero reserved; HIT, IDS or NORMAL never rendered,
 * or ALBEDO with CRT_TEMPORAL_DEMODULATE; source DENOISED before any successful crt_denoise; a shard of a frame (crt_set_shard with
 * world > 1) or a scene on several devices; a read, device or resolve call before any successful crt_temporal, or with a wrong size.
 * A camera with an aperture: the reprojection and its guides keep the pinhole view through the camera's position (crt_render_aov's), so
 * out-of-focus regions are reprojected and tested against guides sharper than the image.  A stated limitation; lens-aware motion
 * vectors are out of scope.
 * An environment (crt_set_environment): the reprojection is unaware of it; miss pixels keep the guide values they have without one. */
enum { CRT_TEMPORAL_DEMODULATE = 1, CRT_TEMPORAL_CLAMP = 2 };
enum { CRT_TEMPORAL_SOURCE_SUM = 0, CRT_TEMPORAL_SOURCE_DENOISED = 1 };
typedef struct crt_temporal_params {   /* 32 bytes */
    uint32_t flags;        /* the two bits above; others refused */
    uint32_t source;       /* SUM: crt_sum_device's image * inv_count; DENOISED: crt_denoise's image (inv_count ignored but still checked) */
    uint32_t max_history;  /* 1..4096; 1 = output equals the source */
    float    sigma_depth;  /* relative depth tolerance, finite, in [1e-6, 1e6] */
    float    normal_min;   /* finite, in [-1, 1]: smallest cosine between the two unit normals */
    uint32_t reserved[3];  /* must be 0 */
} crt_temporal_params;    /* NULL = {DEMODULATE, SUM, 32, 0.1f, 0.9f} */
int crt_temporal(crt_scene* s, float inv_count, const crt_temporal_params* p, int sync);
int crt_temporal_reset(crt_scene* s);                               /* drop the history; the buffers stay */
int crt_read_temporal(crt_scene* s, float* rgb, size_t n_floats);   /* w*h*3, mean radiance */
int crt_read_temporal_history(crt_scene* s, float* n, size_t n_floats); /* w*h: N per pixel */
int crt_temporal_device(crt_scene* s, const float** d_rgb);
int crt_resolve_temporal(crt_scene* s, uint8_t* rgba, size_t n_bytes);
int crt_resolve_temporal_device(crt_scene* s, const uint8_t** d_rgba, int sync);

/* The display transform on the device (no reference counterpart beyond output.fs's fixed curve): one call turns one of the
 * scene's three float images (the running sum, crt_denoise's image, crt_temporal's image) into RGBA8 in device memory, at an exposure that
 * is given or metered on the device from the image's luminance histogram and adapted over calls, through one of four tone curves and then
 * the pinned 2.2 gamma of crt_resolve.  A frame loop may end in crt_display in place of crt_resolve_device.
 * The definition.  Each line is one IEEE float32 operation in the written order, no contraction; integers are exact.
 *   Input pixel.  c = image * inv_count per channel for source SUM; c = image for DENOISED and TEMPORAL (inv_count is checked and then
 *     ignored).  L = (0.3f*c.x + 0.6f*c.y) + 0.1f*c.z.
 *   Meter (only with CRT_DISPLAY_AUTO_EXPOSURE; integer arithmetic throughout, so neither the order of atomics nor the launch shape can
 *     change a bit).  A pixel counts iff L is finite and L >= 0x1p-16f: NaN, +-inf, zero, negatives and pixels owned by another shard rank
 *     do not count.  Its bin is k = min((bits(L) >> 20) - (111 << 3), 255): 256 bins, 8 per octave, from 2^-16 upward, piecewise-linear in
 *     each octave.  h[k] are uint32 counts, N = sum of h.  lo = floor(N*low_permille/1000), hi = floor(N*high_permille/1000) in 64-bit
 *     arithmetic; with the counted pixels ordered by bin, ranks [lo, hi) are kept; M = hi - lo; S = the sum of the kept pixels' bin indices
 *     (uint64).  M == 0: nothing is metered; the exposure keeps the adapted value it had, or takes params.exposure if it had none, and
 *     `calls` does not advance.  Otherwise Q = floor(S*256 / M) + 128 (the mean bin in 1/256ths, moved to the bin's centre);
 *     L_avg = float_from_bits(((111 << 3) << 20) + (Q << 12)); E_target = min(max(key / L_avg, exposure_min), exposure_max), one IEEE
 *     division; the first metered call after create or crt_display_reset, or any call with adapt == 1: E = E_target; otherwise
 *     E = E_prev + (E_target - E_prev) * adapt, E_prev the E of the previous metered call.
 *     Without the flag E = params.exposure; no histogram is made and the adaptation (E_prev, calls) is left alone.
 *   Curve.  x = c * E per channel, lum = (0.3f*x0 + 0.6f*x1) + 0.1f*x2.
 *     REFERENCE: k = 1 / (1 + lum / 2); y = x * k.  At E = 1 this is crt_resolve's arithmetic.
 *     REINHARD:  w2 = white*white (once, on the host, in float32); k = (1 + lum / w2) / (1 + lum); y = x * k.
 *     ACES (Narkowicz's rational fit, per channel): n = x * (2.51f*x + 0.03f); d = x * (2.43f*x + 0.59f) + 0.14f; y = n / d.
 *     CLAMP: y = x.
 *   The byte is the number of thresholds of crt_resolve's pinned gamma that y has reached; NaN and negatives give 0; alpha is 255.
 * crt_display_state: exposure = E of the last call; metered = L_avg, or 0 when nothing was metered (every manual call); counted = N;
 * q = Q; calls = metered calls (M > 0) since create or the last crt_display_reset.  crt_display_get_state waits for the stream and
 * reports the state as of the last call.  crt_read_display_histogram: the bins of the last call with CRT_DISPLAY_AUTO_EXPOSURE, before
 * trimming.  crt_display_reset drops the adaptation (in stream order) and keeps the buffers.  crt_read_display: width*height*4 bytes, rows
 * as crt_resolve has them.  crt_display_device waits for the stream; the pointer stays valid until the scene is destroyed.
 * The exposure lives in device memory and the display kernel reads it from there: a sync = 0 call never waits for the GPU.
 * crt_display is enqueued on the scene's stream behind any *_async frames, crt_render_aov, crt_denoise and crt_temporal calls.  It leaves
 * the sum, the frame count, crt_get_frame_stats, the launch times, every AOV channel, every other stage's buffers and the three
 * crt_resolve*_device buffers as they are.  Its own buffers are allocated by a scene's first crt_display and freed with the scene; later
 * calls allocate nothing.  Source SUM runs on the packed tiles: crt_set_devices works (the histogram takes the gathered peers' slices), and
 * a shard rank (crt_set_shard) sees its own pixels only: other ranks' bytes are 0 and are not counted.  DENOISED and TEMPORAL keep the
 * refusals of the image they name.
 * CRT_ERR_INVALID, nothing written and the exposure state unchanged: null scene; inv_count not finite or <= 0; an unknown source, curve
 * or flag bits; non-zero reserved; a field out of its range or not finite (with AUTO unset the meter's fields are not looked at); a source
 * image that does not exist; a read, device, state or histogram call before any successful crt_display, or with a wrong size; a histogram
 * call when no call has metered.
 * Out of scope (bloom is crt_bloom's, below; crt_display_bloom displays its image): colour grading, output transfer functions other than the pinned 2.2 gamma, a float HDR output, spot or
 * centre-weighted metering, time-based adaptation (adapt is per call; the host scales it by frame time). */
enum { CRT_DISPLAY_SOURCE_SUM = 0, CRT_DISPLAY_SOURCE_DENOISED = 1, CRT_DISPLAY_SOURCE_TEMPORAL = 2 };
enum { CRT_DISPLAY_CURVE_REFERENCE = 0, CRT_DISPLAY_CURVE_REINHARD = 1, CRT_DISPLAY_CURVE_ACES = 2, CRT_DISPLAY_CURVE_CLAMP = 3 };
enum { CRT_DISPLAY_AUTO_EXPOSURE = 1 };
typedef struct crt_display_params {   /* 48 bytes; NULL = {SUM, REFERENCE, 0, 1.0f, 4.0f, 0.18f, 1.0f, 1e-6f, 1e6f, 0, 1000, 0}: crt_resolve's bytes */
    uint32_t source, curve, flags;
    float exposure;                     /* manual E; with AUTO the value used until something has been metered; finite, [1e-9, 1e9] */
    float white;                        /* REINHARD only; finite, [1e-3, 1e6] */
    float key;                          /* AUTO: the luminance the metered mean is mapped to; finite, [1e-6, 1e6] */
    float adapt;                        /* AUTO: share of the way to E_target per call; finite, (0, 1] */
    float exposure_min, exposure_max;   /* AUTO: finite, [1e-9, 1e9], min <= max */
    uint32_t low_permille, high_permille;   /* AUTO: 0 <= low < high <= 1000 */
    uint32_t reserved;                  /* 0 */
} crt_display_params;
typedef struct crt_display_state { float exposure, metered; uint32_t counted, q, calls, reserved[3]; } crt_display_state;
int crt_display(crt_scene* s, float inv_count, const crt_display_params* p, int sync);
int crt_read_display(crt_scene* s, uint8_t* rgba, size_t n_bytes);
int crt_display_device(crt_scene* s, const uint8_t** d_rgba);
int crt_display_get_state(crt_scene* s, crt_display_state* out);
int crt_read_display_histogram(crt_scene* s, uint32_t hist[256]);
int crt_display_reset(crt_scene* s);

/* Bloom on the device (no reference counterpart): what an HDR display chain puts between the float image and the tone
 * curve.  One call takes the light of the bright parts of one of the scene's three float images (the running sum, crt_denoise's image,
 * crt_temporal's image), spreads it over an image pyramid and puts it back on the image: a fourth float image, the bloomed one, which is
 * read, exposed and resolved like the others and displayed by crt_display_bloom.
 * The definition.  Each line is one IEEE float32 operation in the written order, no contraction; the one division is IEEE.
 *   Input pixel.  c as in crt_display: image * inv_count per channel for source SUM; the image as it is for DENOISED and TEMPORAL
 *     (inv_count is checked and then ignored).  L = (0.3f*c.x + 0.6f*c.y) + 0.1f*c.z.
 *   Level sizes.  w_0 = width, h_0 = height, w_k = (w_{k-1} + 1) >> 1, h_k = (h_{k-1} + 1) >> 1.
 *   Level count.  n = the largest n <= levels such that every level k = 1..n has a parent with min(w_{k-1}, h_{k-1}) >= 2.  n == 0 (a
 *     frame one pixel wide or high): the result is c, copied.
 *   Bright pass (level 0 only).  Lc = clamp == 0 ? L : min(L, clamp); k = max(Lc - threshold, 0) / max(L, 0x1p-16f); k = 0 where not
 *     (L > 0); b = c * k per channel.
 *   Down(a), from level k-1 (w x h) to level k, per channel.  Horizontal first, on the parent's rows:
 *     r(x) = ((a[x0-1] + a[x0+2]) + 3.0f * (a[x0] + a[x0+1])) * 0.125f with x0 = 2x, every index clamped to [0, w-1]; then the same
 *     formula vertically over r at rows 2y-1 .. 2y+2, clamped to [0, h-1].  D_1 = Down(b), D_k = Down(D_{k-1}).
 *   Up(a, w, h), from level k+1 (ws x hs) to the size of level k, per channel.  Horizontal: near = x >> 1; far = (x & 1) ? near + 1 :
 *     near - 1, clamped to [0, ws-1]; r = a[near]*0.75f + a[far]*0.25f.  Then the same vertically.
 *   The way back up.  U_n = D_n; for k = n-1 .. 1: U_k = D_k + (Up(U_{k+1}) - D_k) * scatter.
 *   Glare.  G = Up(U_1, w_0, h_0).
 *   Result.  With CRT_BLOOM_CONSERVE: out = c + (G - c) * strength.  Without: out = c + G * strength.
 *   Non-finite input gives non-finite or unspecified values in the pixels its taps reach; which pixels those are is defined by the
 *     arithmetic above, only a NaN's payload is unspecified.
 * crt_read_bloom: width*height*3 floats of mean radiance, rows as crt_read_sum has them.  crt_bloom_device waits for the stream; the
 * pointer stays valid until the scene is destroyed.  crt_resolve_bloom*: crt_resolve's curve and pinned gamma at inv_count 1, in a
 * buffer of the stage's own.  crt_display_bloom is crt_display with the bloomed image as its input pixel: the same meter, adaptation
 * state, RGBA8 buffer, state block, histogram and refusals; p->source must be 0 and names nothing; there is no inv_count, the image is
 * a mean.
 * crt_bloom is enqueued on the scene's stream behind any *_async frames, crt_render_aov, crt_denoise and crt_temporal calls; sync = 0
 * returns at once.  It leaves the sum, the frame count, crt_get_frame_stats, the launch times, every AOV channel, every other stage's
 * buffers and the crt_resolve*_device buffers as they are: it writes only its own buffers and, for SUM, the un-tiled copy every
 * crt_read_sum rewrites.  Its buffers (the pyramid, the output, its RGBA8) are allocated by a scene's first crt_bloom and freed with
 * the scene; later calls allocate nothing.  Source SUM works with crt_set_devices (the un-tiling gathers the peers); a shard of a frame
 * (crt_set_shard with world > 1) is refused: a filter needs its neighbours.  DENOISED and TEMPORAL keep the refusals of the image they
 * name.
 * CRT_ERR_INVALID, nothing written, crt_last_error names the field: null scene; inv_count not finite or <= 0; an unknown source or
 * unknown flag bits; levels outside 1..8; a field out of its range or not finite; non-zero reserved; a source image that does not
 * exist; a read, device, resolve or display call before any successful crt_bloom, or with a wrong size.
 * Out of scope: lens flares and streaks, a spectral or per-channel kernel, a temporal stabiliser, bloom on a shard. */
enum { CRT_BLOOM_SOURCE_SUM = 0, CRT_BLOOM_SOURCE_DENOISED = 1, CRT_BLOOM_SOURCE_TEMPORAL = 2 };
enum { CRT_BLOOM_CONSERVE = 1 };
typedef struct crt_bloom_params {   /* 32 bytes; NULL = {SUM, 6, CONSERVE, 0.0f, 0.0f, 0.7f, 0.05f, 0} */
    uint32_t source;      /* which float image; others refused */
    uint32_t levels;      /* 1..8 pyramid levels asked for */
    uint32_t flags;       /* CRT_BLOOM_CONSERVE or 0; other bits refused */
    float    threshold;   /* luminance below which nothing blooms; finite, [0, 1e6] */
    float    clamp;       /* 0 = none; else finite, [1e-6, 1e9]: a pixel feeds the pyramid as if its luminance were at most this (fireflies) */
    float    scatter;     /* finite, [0, 1]: share taken from the coarser level at each step up */
    float    strength;    /* finite; [0, 1] with CONSERVE, [0, 1e3] without */
    uint32_t reserved;    /* 0 */
} crt_bloom_params;
int crt_bloom(crt_scene* s, float inv_count, const crt_bloom_params* p, int sync);
int crt_read_bloom(crt_scene* s, float* rgb, size_t n_floats);           /* w*h*3, mean radiance, rows as crt_read_sum */
int crt_bloom_device(crt_scene* s, const float** d_rgb);
int crt_resolve_bloom(crt_scene* s, uint8_t* rgba, size_t n_bytes);      /* crt_resolve's curve + pinned gamma, inv_count 1 */
int crt_resolve_bloom_device(crt_scene* s, const uint8_t** d_rgba, int sync);
int crt_display_bloom(crt_scene* s, const crt_display_params* p, int sync);

/* Homogeneous fog with shadowed single scattering ("light shafts") between the camera and the surfaces of the scene's current view, or
 * along segments the caller names, flat and instanced scenes (no reference counterpart).  Each eye segment is cut into K
 * strata; one jittered point per stratum aims one shadow ray at a sampled point of the scene's area lights, as the integrator's next-event
 * estimation does from a surface.  The rays are built on the device where they are walked and never stored; which of them arrive is a bit
 * per ray, so the result is defined bit for bit: every line below is ONE IEEE float32 operation in the written order under DESIGN.md §3
 * (no contraction); dot, normalize, the correctly rounded sqrt and 1/x, pinned_sin and rand_at(j) (crt_render_ao's step 4) are the
 * library's.  F(x) = x rounded to float32.
 *
 * A FOG SEGMENT is crt_fog_segment: (o[3], seed_x, e[3], seed_y), 32 bytes, laid out like crt_ray: o is where the eye ray starts, e the
 * vector to where it ends.  crt_fog_params (64 bytes): samples K in 1..256; flags = 0; density sigma (extinction per world unit) finite,
 * in [0, 1e6]; albedo[3] each finite, in [0, 1]; anisotropy g finite, in [-0.99, 0.99]; max_distance finite and > 0; ambient[3] each
 * finite and >= 0 (a uniform in-scattered radiance that needs no rays); reserved = 0.  NULL params mean
 * {16, 0, 0.05f, {1, 1, 1}, 0.0f, 100.0f, {0, 0, 0}}.  rv = rx * ry, as in a frame.  Per segment:
 *   1. Length.  D2 = dot(e, e).  If D2 is not > 0, or D2 or any component of o is not finite, the result is (0, 0, 0, -1) and no ray is
 *      traced.  Otherwise D = sqrt(D2); dir = e * (1 / D); h = D / F(K) (IEEE division).
 *   2. Transmittance to the end.  TD = exp_neg(F(sigma * D)).
 *   3. Sample j (0-based) uses four draws: u0 = rand_at(4j+1), r0 = rand_at(4j+2), r1 = rand_at(4j+3), r2 = rand_at(4j+4);
 *      s = F(F(j) + u0) * h; x = o + dir * s, per component F(o.k + F(dir.k * s)).
 *   4. Light sample (path_trace.fs:940, :849-854).  li = min((int)F(r0 * F(n_lights)), n_lights - 1); sq = sqrt(r1); b0 = 1 - sq;
 *      b1 = r2 * sq; pos = (p + u*b0) + v*b1 of light li; ld = pos - x; ln = length(ld); ld = ld * (1 / ln); cos_light = dot(ld, n_light).
 *      The light table is the one a frame reads at enqueue; for a scene from crt_scene_create_instanced_lit, the world table that
 *      crt_scene_read_lights returns.  A sample whose cos_light is not < 0 is DARK: no ray, nothing added.  With n_lights == 0 every
 *      sample is dark.
 *   5. Occlusion.  The ray is crt_ray{x, tmax = ln - 1e-4f, d = ld}.  It is occluded iff crt_trace(.., CRT_TRACE_ANY) reports a hit for
 *      that crt_ray; an instanced scene: crt_instances_trace(.., CRT_TRACE_ANY) on the scene's handle as it is at enqueue, with option
 *      "instance_masks" 1 | CRT_TRACE_INSTANCE_MASK with the ray mask "mask_shadow".
 *   6. Contribution of an unoccluded sample.  pdf = F(F(F(ln*ln) / F(area * -cos_light)) * pdf_choice) (path_trace.fs:986);
 *      ct = dot(dir, ld); den = F(F(1 + F(g*g)) - F(F(2*g) * ct)); ph = F(F(F(1 - F(g*g)) * 0.07957747f) / F(den * sqrt(den)))
 *      (Henyey-Greenstein; g = 0 gives 1 / 4 pi); att = exp_neg(F(sigma * F(s + ln))); w = F(F(F(att * ph) * F(sigma * h)) / pdf);
 *      per channel c: F(F(emission.c * albedo.c) * w).
 *      exp_neg(xf), xf a float that is never negative here, is e^-x in double with ONE rounding to float32, plain multiplies and adds,
 *      nothing fused: x = (double)xf; the value is +0.0f unless x < 104.0; k = rint(x * 0x1.71547652b82fep+0);
 *      r = (x - k * 0x1.62e42feep-1) - k * 0x1.a39ef35793c76p-33; q = -r; p = 1/13!; then p = p*q + 1/i! for i = 12, 11, .. 1 and
 *      p = p*q + 1 (each 1/i! the double nearest to the quotient); the value is (float)(p * 2^-k), 2^-k exact.  It is within 1 ulp of
 *      the correctly rounded e^-x, exactly 1 at 0, and never increases with x.
 *   7. Result.  Per channel A.c = F(F(ambient.c * albedo.c) * F(1 - TD)); b = A; for j = 0 .. K-1 in that order, b = b + contribution_j
 *      for each unoccluded (and not dark) j.  The output float[4] is (b.x, b.y, b.z, TD): the in-scattered radiance S and the
 *      transmittance of whatever lies at the segment's end.
 *
 * VIEW MODE, crt_render_fog(s, rx, ry, params, sync): the segments come from the primary rays of crt_render_aov(s, rx, ry, ..): the same
 * rays (the scene's camera, the "jitter" option, the pinhole through `position` whatever the aperture, the masked walk with
 * "mask_primary" where that applies).  o = the ray's origin; t = the HIT channel's t, 1e9f for a miss; Dv = min(t, max_distance);
 * e = d * Dv per component; (seed_x, seed_y) = the pixel's RNG state BEHIND the primary ray's draws, as in crt_render_ao.  A miss pixel
 * marches to max_distance; it is no special case.  The image is width*height float[4] in linear pixel order, rows as crt_read_sum has
 * them, allocated by the first call and freed with the scene; the first hits go into a buffer of the fog state's own.
 * SEGMENTS MODE, crt_fog_segments (host pointers; returns when `out`, n x float[4], is written) and crt_fog_segments_device (device
 * pointers): the same bytes as view mode gives for the same segments.  n = 0 succeeds and writes nothing.
 * crt_read_fog wants n_floats = width*height*4.  crt_fog_device waits for the stream; the pointer stays valid until the scene is destroyed.
 * COMPOSITE, crt_fog_composite(s, inv_count, source, sync): per pixel and channel out.c = F(F(c.c * TD) + S.c), c being crt_display's
 * input pixel of `source` (CRT_DISPLAY_SOURCE_SUM: the sum times inv_count; _DENOISED, _TEMPORAL: the image as it is) and (S, TD) the
 * pixel of the most recent crt_render_fog; a pixel whose fog word 3 is -1 copies c.  The result is a fifth float image, width*height*3
 * floats of mean radiance: crt_read_fogged, crt_fogged_device (as crt_read_bloom, crt_bloom_device), and crt_display_fogged, which is
 * crt_display with the fogged image as its input pixel: the same meter, adaptation state, RGBA8 buffer, state block, histogram and
 * refusals as crt_display_bloom; p->source must be 0 and names nothing; there is no inv_count.  There is no crt_resolve_fogged.
 *
 * The calls are enqueued on the scene's stream behind any *_async frames (sync = 0 returns at once); later frames and reads are ordered
 * behind them.  The sum, the frame count, crt_get_frame_stats, the launch times, every AOV channel, the AO image, every other stage's
 * buffers and every frame's path and RNG state stay as they are (the composite of SUM rewrites the un-tiled copy every crt_read_sum
 * rewrites).  An instanced scene reads its handle's live arrays and its live light table at enqueue.  An environment and a lens change
 * no byte.
 * CRT_ERR_INVALID, crt_last_error names the field, nothing written and earlier images untouched: a null scene; a null segments or out
 * pointer with n > 0; samples outside 1..256; flags or reserved not 0; density, albedo, anisotropy, max_distance or ambient outside the
 * ranges above or not finite; n * K or width*height*K >= 2^32; option "accel" not 0; a shard of a frame (crt_set_shard with world > 1);
 * a scene on several devices or streams (crt_set_devices, option "streams"); crt_render_fog before crt_set_camera; crt_fog_composite
 * before a successful crt_render_fog, with an inv_count not finite or <= 0, or of a source that is unknown or does not exist;
 * crt_read_fog / crt_fog_device before any crt_render_fog, crt_read_fogged / crt_fogged_device / crt_display_fogged before any
 * crt_fog_composite, or n_floats of another size.
 * Out of scope: fog on bounce segments or inside the integrator; heterogeneous density or a coloured extinction; the environment as a
 * fog light; accumulation over calls (the caller averages S over frames); fog as a source of crt_denoise / crt_temporal / crt_bloom;
 * shards and several devices; any fog in the C oracle. */
typedef struct crt_fog_segment { float o[3]; float seed_x; float e[3]; float seed_y; } crt_fog_segment;
typedef struct crt_fog_params {     /* 64 bytes; NULL = {16, 0, 0.05f, {1, 1, 1}, 0.0f, 100.0f, {0, 0, 0}, 0} */
    uint32_t samples;      /* K: 1..256 strata, one shadow ray each at most */
    uint32_t flags;        /* 0 */
    float    density;      /* sigma: extinction per world unit; finite, [0, 1e6] */
    float    albedo[3];    /* scattering albedo; each finite, [0, 1] */
    float    anisotropy;   /* g of Henyey-Greenstein; finite, [-0.99, 0.99] */
    float    max_distance; /* finite, > 0: where a view segment ends at the latest */
    float    ambient[3];   /* uniform in-scattered radiance; each finite, >= 0 */
    uint32_t reserved[5];  /* 0 */
} crt_fog_params;
int crt_render_fog(crt_scene* s, float rx, float ry, const crt_fog_params* params, int sync);
int crt_read_fog(crt_scene* s, float* dst, size_t n_floats);             /* w*h*4: (S.rgb, TD) */
int crt_fog_device(crt_scene* s, const float** d_ptr);
int crt_fog_segments(crt_scene* s, const crt_fog_segment* segments, size_t n, float rx, float ry, const crt_fog_params* params, float* out);
int crt_fog_segments_device(crt_scene* s, const void* d_segments, size_t n, float rx, float ry, const crt_fog_params* params, void* d_out, int sync);
int crt_fog_composite(crt_scene* s, float inv_count, uint32_t source, int sync);   /* source: CRT_DISPLAY_SOURCE_* */
int crt_read_fogged(crt_scene* s, float* rgb, size_t n_floats);          /* w*h*3, mean radiance, rows as crt_read_sum */
int crt_fogged_device(crt_scene* s, const float** d_rgb);
int crt_display_fogged(crt_scene* s, const crt_display_params* p, int sync);

/* Animated geometry (no reference counterpart: the reference uploads its scene once, Scene.h:1000-1062; DXR / OptiX call this an
 * update build).  New positions for the scene's vertices; triangles, materials, textures and the tree topology are unchanged.
 * n_vertices must equal the count given at create; normals (n_normals == create's) and lights (n_lights == create's) may be NULL =
 * unchanged.  Refits the CWBVH (node8 boxes re-quantised), the BVH2 if the scene kept one, the intersection records of both walks
 * and the float planes if they exist, on the scene's device, one launch per tree level; clears the accumulated sum like crt_reset and
 * has the tile order measured again.  Every coordinate is checked first (finite, |x| <= 1e18, as crt_scene_create): a bad one or a
 * wrong count returns CRT_ERR_INVALID and leaves the scene as it was.  The tree keeps its topology, so its quality decays as the
 * geometry moves away from the positions it was built for ("Refit"; crt_rebuild_vertices builds it again, crt_get_tree_cost measures it).  crt_triangle.vn with w == 0 (the loader's
 * truncated geometric normal, Scene.h:849-852) is caller data and stays as given.  Under crt_set_devices every replica follows:
 * replicas on this GPU share the refitted buffers, replicas on other GPUs receive them by peer copy.  The first call allocates
 * the refit's own state (~2.7 MB at 1 M triangles plus the host form's vertex buffer); a scene that never calls it has none. */
int crt_update_vertices(crt_scene* s, const float* vertices, size_t n_vertices,
                        const float* normals, size_t n_normals, const crt_light* lights, size_t n_lights);
/* the same with the positions already in HBM on the scene's device (e.g. written by the caller's skinning kernel); waits once on the
 * host for the check of the coordinates, then runs asynchronously on the scene's stream unless sync != 0 (d_vertices must stay valid
 * until then) */
int crt_update_vertices_device(crt_scene* s, const void* d_vertices, size_t n_vertices, int sync);
/* device ms of the last update's refit kernels and host wall ms of the call (CRT_ERR_INVALID before the first update); after a
 * crt_rebuild_vertices* the two describe that call (device ms: stream time from the first builder launch to the last assembly kernel) */
int crt_last_update_ms(crt_scene* s, float* device_ms, float* wall_ms);
/* Animated geometry, the other remedy (DXR / OptiX call this a rebuild): new positions AND a new tree, in place.
 * Arguments, checks and refusals are crt_update_vertices': the counts equal the create's, every coordinate finite and within 1e18
 * (checked on the device first), normals and lights optional.  The tree is then built again from the new positions with the builder
 * the scene was created with, by crt_scene_create's own build-on-device chain (BVH2 -> CWBVH -> leaf-order triangles and records), so
 * every debug read, every crt_get_bvh_info field other than the times, every walk (per-ray counts included) and every frame are those
 * of a crt_scene_create from the same arrays with the linear and the binned-SAH builder (PLOC merges in an order its atomics decide,
 * as at create: hits and sums are equal, the tree's bytes need not be).  Only the positions cross PCIe; camera, options, shard,
 * streams and frame buffers stay.
 *   - Scenes built on the device only (crt_bvh_info.built_on_device): a scene created from host arrays and an instanced scene
 *     return CRT_ERR_INVALID, and so does a scene with a replica on ANOTHER GPU (crt_set_devices).  Replicas on the scene's own GPU
 *     (option "streams", or crt_set_devices naming it again) share the rebuilt buffers and have them before the call returns.
 *   - All or nothing: the tree is built into new buffers and published last.  A failed check (CRT_ERR_INVALID), a CWBVH deeper than
 *     the traversal stack (CRT_ERR_LIMIT) or a failed allocation (CRT_ERR_NOMEM) leaves everything a walk or a frame reads, every
 *     debug read and every crt_get_bvh_info field as it was.
 *   - A success replaces the node8s, both record arrays, the leaf-order triangles, the BVH2 (kept or dropped by create's depth
 *     rule), the float planes where they exist, the stack sizes, the node counts, depths and the two device build times of
 *     crt_bvh_info, and drops the refit state (the next crt_update_vertices finds the new tree's levels); the accumulated sum is
 *     cleared as by crt_reset and the tile order is measured again.
 *   - The first rebuild scatters the leaf-order triangle array back to source order (create threw that array away) and keeps it,
 *     48 B per triangle, beside the host form's vertex staging; a scene that never rebuilds allocates and launches nothing for this.
 *   - The builders wait on the host, so both forms return when the rebuild is done; sync is accepted for symmetry.
 * There is no automatic choice between refit and rebuild: crt_get_tree_cost, taken after a refit and after a rebuild of the same
 * positions, is the number to build a policy on. */
int crt_rebuild_vertices(crt_scene* s, const float* vertices, size_t n_vertices,
                         const float* normals, size_t n_normals, const crt_light* lights, size_t n_lights);
int crt_rebuild_vertices_device(crt_scene* s, const void* d_vertices, size_t n_vertices, int sync);

/* Deformation on the device (no reference counterpart: the reference's meshes never move): linear blend skinning with
 * four influences per element, and morph targets on the positions.  A crt_deformer holds the rest pose, the influences and the morph
 * targets in HBM, uploaded once; a pose is n_bones 3x4 matrices and n_targets weights, a few hundred bytes, and one kernel writes the
 * deformed positions and normals into buffers the deformer owns, from where they go into crt_update_vertices_device,
 * crt_rebuild_vertices_device, crt_instances_update_meshes_device, or, with the normals, through crt_deform_scene.
 * The definition.  Each line is one IEEE float32 operation in the written order, no contraction; square root and division are
 * correctly rounded.  A bone B[b] is a 3x4 row-major float[12] like crt_instance.object_to_world: the skinning matrix (bone-to-world
 * times inverse bind), composed by the caller.  An element (a vertex or a normal) has four (b_k, w_k), k = 0..3.
 *   Morph (positions only).  p = rest[v].  Then for every target t, in ascending t, that lists vertex v with delta d:
 *     p.c = p.c + mw[t] * d.c for c = x, y, z.  A NULL morph_weights means all zeros, and the arithmetic still applies.
 *   Blend, for j = 0..11.  M_j = w_0 * B[b_0][j]; then for k = 1, 2, 3: if w_k != 0, M_j = M_j + w_k * B[b_k][j].  A zero weight
 *     after the first contributes nothing.  Weights are used as given, not normalised.
 *   Position.  out.x = ((M_0*p.x + M_1*p.y) + M_2*p.z) + M_3; out.y and out.z likewise with M_4..7 and M_8..11.
 *   Normal (its own four influences; not morphed).  q.x = (M_0*n.x + M_1*n.y) + M_2*n.z, q.y and q.z likewise with rows 1 and 2.
 *     l2 = (q.x*q.x + q.y*q.y) + q.z*q.z.  If l2 >= 0x1p-126f and l2 is finite: out = q / sqrtf(l2) (three divisions).  Otherwise
 *     out = q.  This is the linear part of the blended matrix, not its inverse transpose: exact for rigid and uniformly scaled
 *     bones, an approximation under non-uniform scale or shear.
 * crt_deformer_create copies every array of the desc (all host pointers) and allocates everything the deformer ever holds: 36 B per
 * element for rest pose and influences, 12 B per element of output, 16 B per morph entry + 4 B per vertex where there are targets,
 * 48 B per bone + 4 B per target of pose on the device and pinned on the host, one stream, five events.  The per-target lists become
 * one list per vertex in target order, so a thread sums its own deltas: there are no floating-point atomics and two poses with the
 * same input give the same bits.  The kernel reads the palette from a copy in LDS up to 256 bones and through the vector cache above;
 * CRT_DEFORM_PALETTE=global in the environment at create takes the second way at any count; the bits are the same.
 * CRT_ERR_INVALID (nothing allocated): a null or inconsistent desc (normal_bones / normal_weights
 * are required exactly when n_normals > 0); n_vertices 0; n_vertices, n_normals or the number of morph entries >= 2^31; n_bones
 * outside 1..65536; n_targets above 65535; a rest position, rest normal, weight or delta that is not finite; |rest position| > 1e18;
 * a bone index >= n_bones; a morph vertex >= n_vertices; target_first not starting at 0 or descending; vertex indices within one
 * target not strictly ascending; no such device.  The desc is checked first, then the device: CRT_ERR_NO_DEVICE without a GPU.
 * crt_deformer_pose: bones (12 * n_bones floats) and morph_weights (n_targets floats or NULL) are host arrays, checked finite on the
 * host (CRT_ERR_INVALID, the outputs as they were), copied, and the kernel runs on the deformer's own stream; sync = 0 returns at
 * once.  The outputs are NOT checked: a pose can produce non-finite or huge coordinates, which the calls that take them refuse.
 * crt_deformer_vertices_device / crt_deformer_normals_device: n_vertices x 3 / n_normals x 3 floats (NULL for a deformer without
 * normals); valid for the deformer's life.  Before handing them to another handle the caller waits (sync != 0 or crt_deformer_sync):
 * that handle reads them on a stream of its own.  crt_deformer_read copies the last pose's outputs to the host (normals may be NULL;
 * CRT_ERR_INVALID before the first pose or with wrong sizes).  crt_deformer_last_ms: stream time of the last pose's kernel.
 * crt_deform_scene is the whole per-frame step of a flat scene, enqueued on the SCENE's stream: the pose; the coordinate check of
 * crt_update_vertices_device, and the same check over the new normals; the new normals copied device to device into the scene's
 * normal buffer; the refit.  With CRT_DEFORM_REBUILD the tree is rebuilt instead, under every rule and refusal of
 * crt_rebuild_vertices_device.  CRT_DEFORM_KEEP_NORMALS (and a deformer without normals) leaves the scene's normals alone.  The
 * result is that of crt_update_vertices(s, V, n_vertices, N, n_normals, NULL, 0) (or crt_rebuild_vertices) with V, N the definition's
 * output: every debug read, every walk, every frame.  The one host wait is the check's, as in crt_update_vertices_device; sync = 0
 * returns with the refit enqueued.  The call orders itself behind the deformer's own stream and the deformer's next pose behind it.
 * CRT_ERR_INVALID, the scene as it was: a null argument; unknown flag bits; a deformer on another device; an instanced scene or a
 * replica; n_vertices differing from the scene's; n_normals differing from the scene's unless KEEP_NORMALS or the deformer has none;
 * a pose that is not finite; an output coordinate or normal component that is not finite or exceeds 1e18 (the deformer's outputs
 * then hold that pose).  Lights stay as they are: a deforming emissive mesh keeps the lights of its create.
 * crt_deform_host [host] runs the same checks and the same arithmetic (csrc/host/deform_math.hpp, which the kernel includes) on the
 * CPU: out_vertices 3 * n_vertices floats, out_normals 3 * n_normals floats or NULL.  desc->device is ignored.  A refusal writes
 * nothing.
 * Out of scope: normals recomputed from the deformed triangles, morph deltas for normals, dual-quaternion blending, more than four
 * influences, moved lights of a deforming emissive mesh, the shading normals of an instanced scene's meshes (the ray-query handle
 * is served through the raw pointers only), and removing the one host wait of the coordinate check. */
enum { CRT_DEFORM_REBUILD = 1, CRT_DEFORM_KEEP_NORMALS = 2 };     /* crt_deform_scene's flags */
typedef struct crt_deformer_desc {
    uint32_t abi_version;                 /* CRT_ABI_VERSION */
    const float*    rest_vertices;        /* 3 * n_vertices */
    size_t          n_vertices;
    const uint16_t* vertex_bones;         /* 4 * n_vertices */
    const float*    vertex_weights;       /* 4 * n_vertices */
    const float*    rest_normals;         /* 3 * n_normals, or NULL */
    size_t          n_normals;
    const uint16_t* normal_bones;         /* 4 * n_normals; required exactly when n_normals > 0 */
    const float*    normal_weights;       /* 4 * n_normals; likewise */
    uint32_t        n_bones;              /* 1..65536 */
    uint32_t        n_targets;            /* 0..65535 */
    const uint32_t* target_first;         /* n_targets + 1: target t owns entries [target_first[t], target_first[t + 1]) */
    const uint32_t* target_vertex;        /* per entry: the vertex, strictly ascending within one target */
    const float*    target_delta;         /* 3 per entry */
    int32_t         device;
} crt_deformer_desc;
typedef struct crt_deformer crt_deformer;
int crt_deformer_create(const crt_deformer_desc* desc, crt_deformer** out);
int crt_deformer_destroy(crt_deformer* d);
int crt_deformer_pose(crt_deformer* d, const float* bones, const float* morph_weights, int sync);
int crt_deformer_sync(crt_deformer* d);
int crt_deformer_vertices_device(crt_deformer* d, const float** d_vertices);
int crt_deformer_normals_device(crt_deformer* d, const float** d_normals);
int crt_deformer_read(crt_deformer* d, float* vertices, size_t n_floats_v, float* normals, size_t n_floats_n);
int crt_deformer_last_ms(crt_deformer* d, float* device_ms);
int crt_deform_scene(crt_scene* s, crt_deformer* d, const float* bones, const float* morph_weights, uint32_t flags, int sync);
int crt_deform_host(const crt_deformer_desc* desc, const float* bones, const float* morph_weights, float* out_vertices,
                    float* out_normals);                                                                    /* [host] */

/* The SAH cost of a CWBVH.  For every node8 of a range and every slot with meta != 0 the slot's corners are decoded as
 * the walk decodes them, lo = p + q_lo * 2^(e-127) and hi likewise, each rounded once to fp32, then widened to double:
 * A = (dx*dy + dy*dz) + dz*dx, half the slot's surface area.  inner_area sums A over the inner (imask) slots; leaf_area sums
 * A * items over the others, items = popcount(meta >> 5); root_area is A of the union of the used slots of the root node;
 * cost = (233 * (root_area + inner_area) + 71 * leaf_area) / root_area, 0 when root_area is 0: the expected price of a random ray
 * that hits the root box, in the instruction counts of a general node step and a triangle test (profiles/isa_counts.json).  The
 * device computes every slot's A to the host's bits; the sums may differ by the order of the additions (no floating-point atomics:
 * two calls on one tree return the same bits).  The cost of a tree grows when its geometry spreads out, whatever its quality:
 * compare two trees over the SAME positions (a refit against a rebuild), not a tree with its own past.  For a TLAS the leaf items are
 * instances, whose price is not a triangle test's: its cost compares two TLASes over the same instances and nothing else. */
typedef struct crt_tree_cost {
    double root_area, inner_area, leaf_area;   /* half-areas; leaf_area = sum of A(slot) * items(slot) */
    uint64_t n_nodes8, n_inner_slots, n_leaf_slots, n_leaf_items;
    double cost;
} crt_tree_cost;
/* the live CWBVH of a scene (nodes [0, n_nodes8), root 0), computed on its device; synchronous.  An instanced scene returns
 * CRT_ERR_INVALID: its trees belong to its handle (crt_instances_tree_cost) */
int crt_get_tree_cost(crt_scene* s, crt_tree_cost* out);
/* test hook: the device-resident tree and records as the walks see them, unpadded: which 0 = node8 (80 B each), 1 = records in
 * CWBVH order (48 B), 2 = BVH2 FlatNodes (32 B; none when the scene has no BVH2), 3 = records in slot order (48 B).
 * dst may be NULL to query the count. */
int crt_debug_read_accel(crt_scene* s, int which, void* dst, size_t cap_bytes, size_t* n_out);

/* the duration in ms of every launch that carried events since the spans were last restarted (options "timing", "timing_accumulate"),
 * in launch order; ms may be NULL to query the count */
int crt_get_launch_times(crt_scene* s, float* ms, size_t cap, size_t* n_out);
/* test hook: read back a ray queue of the last rendered frame (which: 0 = path rays entering
 * `segment`, 2 = that segment's shadow rays).  dst may be NULL to query the count.  (0, 0) after a frame of a flat scene through a lens
 * (crt_camera.aperture > 0): the lens primary rays, tmax 1e9f, pad = the path's id, at every max_depth. */
int crt_debug_read_queue(crt_scene* s, int which, uint32_t segment, crt_ray* dst, size_t cap, size_t* n_out);
/* measurement aid: the same n_frames (rxy = n_frames pairs) queued `reps` times on the stream and replayed `reps`
 * times as one captured hipGraph; device milliseconds per frame of either way ("hipGraph") */
int crt_debug_time_graph(crt_scene* s, uint32_t n_frames, const float* rxy, uint32_t reps, float* ms_stream, float* ms_graph);
/* test hook: how the last launch of crt_render_frame(s) ran the samples of its first segment: *form = 0 one sample, or several
 * one after the other in each wave; 1 = side by side on the waves of a workgroup (option "wave_samples") */
int crt_debug_launch_form(crt_scene* s, int32_t* form);
/* test hook: the same launch in full: info[0] = form as above (2 = four samples of a 4 x 4 pixel quadrant in the lanes of a wave),
 * info[1] = bit 0: the first segment ran its 6-waves-per-SIMD build (option "wide_first"), bit 1: a one-pass build (no sample loop), bit 2: that
 * build compiled as a last segment (option "last_build"), bit 3: that build's LEAN form (option "lean_build"), bit 4: segment 0 was fed by the
 * lens ray generator (crt_camera.aperture > 0: every segment ran in its queue-fed form; info[0] is then 0 and bits 0-3 are clear),
 * bit 5: the frame ran with an environment (crt_set_environment: k_env_miss behind every segment's closest-hit launch; bits 0-3 clear),
 * bit 6: segment 0 was fed by the caller's camera rays (crt_set_camera_rays: every segment ran in its queue-fed form; bits 0-4 clear),
 * info[2] = samples per pixel of the launch (a lens frame or one along camera rays: of the launch chain),
 * info[3] = tile shards rendering side by side (option "streams" / crt_set_devices) */
int crt_debug_launch_info(crt_scene* s, int32_t info[4]);
/* measurement aid: hist[130] receives, for the counting frames ("count_visits") rendered since the previous call, how many node steps ran
 * with k of the wave's 64 lanes enabled — closest-hit walks in hist[k], any-hit walks in hist[65 + k] — and the collection (re)starts;
 * hist = NULL stops it.  Process-wide; tools/lane_hist.py prints the distribution behind the lane-utilisation figures.  With option
 * "step_hist_mode" 1 (set before the call that starts the collection) the index is the number of DISTINCT (node, octant) keys among the
 * step's enabled lanes instead — 1 = a uniform step — i.e. the steps a packet walk would need. */
int crt_debug_step_hist(crt_scene* s, unsigned long long* hist);

/* Multi-GPU tile sharding (no reference counterpart).  The framebuffer is
 * cut into tile x tile squares dealt round-robin in Morton order to `world` ranks;
 * this scene renders only rank's tiles.  Call before the first crt_render_frame.  tile: a multiple of 8 in
 * 8..1024; a scene that never calls this is rank 0 of 1 with 16 x 16 tiles.  The tile is also the unit of the launch
 * schedule (option "adaptive_tiles"): smaller tiles schedule finer (1 M triangles, 1080p: 0.273 / 0.261 / 0.257 / 0.254 ms
 * per frame at 64 / 32 / 16 / 8). */
int crt_set_shard(crt_scene* s, uint32_t rank, uint32_t world, uint32_t tile);
/* Several GPUs behind ONE handle, one process, one frame loop — the shape of the reference (main.cpp:262-300 calls
 * Scene::update / Scene::Render once per frame, Scene.h:1158-1231) with the tile sharding and the gather done inside
 * the library ("Outputs": "multi-GPU gather happens inside these").  `devices` lists n_devices HIP device
 * ids; devices[0] must be the device the scene lives on.  The scene's device buffers are copied to every other device
 * over the fabric (hipMemcpyPeer: nothing is re-uploaded from the host, and a scene built on the device is replicated
 * as built), the tiles (tile x tile pixels, Morton order) are dealt round-robin to the devices exactly as crt_set_shard
 * deals them to ranks, and from then on every entry point acts on all of them: crt_set_camera / crt_set_option /
 * crt_reset fan out, crt_render_frame[s][_async] enqueues the frame on each device's own stream (the devices run side
 * by side), crt_sync waits for all, crt_get_frame_stats adds the counts up (times: the slowest device).  crt_read_sum
 * and crt_resolve gather the packed per-tile radiance of devices 1..n-1 to device 0 — grouped RCCL send / recv over
 * xGMI, one slice per link, librccl.so loaded on first use; hipMemcpyPeerAsync when RCCL cannot be loaded or option
 * "gather_transport" is 1 — and un-tile the whole frame there.  Sums are bit-identical to one device rendering the whole
 * frame (a pixel's samples depend on its coordinates and the frame's randomVector only).  n_devices = 1 returns to a
 * single device.  The same id may appear more than once ("virtual devices": separate streams and shards on one GPU,
 * gathered by copies) — that is how the path is tested on a one-GPU machine.  crt_set_shard is refused on such a scene;
 * crt_trace*, crt_packed_info / crt_read_packed act on device 0 alone.  One process per GPU with crt_set_shard and the
 * caller's own collective (caitlynrenderer_amd/tiles.py, bench.py --gpus N) remains the other way to use several GPUs. */
int crt_set_devices(crt_scene* s, const int32_t* devices, uint32_t n_devices, uint32_t tile);
/* [host] Which tiles logical device `device` of `n_devices` renders when those devices divide shard `rank` of `world` of a width x height
 * frame among themselves: tile_xy receives (x, y) pairs in the order of the device's packed buffer (up to `capacity` pairs), *n_tiles the
 * count.  crt_set_shard is (rank, world, 0, 1); crt_set_devices (0, 1, k, n); option "streams" on a shard (rank, world, k, streams).
 * No GPU needed: the bookkeeping of SURVEY 8e can be checked on any machine. */
int crt_shard_tiles(uint32_t width, uint32_t height, uint32_t tile, uint32_t rank, uint32_t world, uint32_t device, uint32_t n_devices,
                    uint32_t* tile_xy, size_t capacity, size_t* n_tiles);
/* what crt_set_devices left: the device list (up to `capacity` entries), how the gather travels (0 RCCL, 1 peer copies)
 * and the host milliseconds the last gather took (enqueue to completion on device 0); any pointer may be NULL */
int crt_get_devices(crt_scene* s, uint32_t* n_devices, int32_t* devices, uint32_t capacity, int32_t* transport, float* last_gather_ms);
/* packed tile-major sum buffer of this rank: n_local_tiles * tile*tile*3 floats. */
int crt_packed_info(crt_scene* s, uint32_t* n_local_tiles, uint32_t* tile, size_t* n_floats);
int crt_read_packed(crt_scene* s, float* dst_host, size_t n_floats);
int crt_copy_packed_device(crt_scene* s, void* d_dst, size_t n_floats, int sync);

/* Telemetry of the last crt_render_frame / crt_trace_device (hipEvent timings on the
 * scene's own stream, ray counts).  SURVEY 8d. */
typedef struct crt_frame_stats {
    uint64_t closest_rays, any_rays;     /* traversals executed                  */
    float ms_total;                      /* raygen..accumulate, device time      */
    float ms_trace_closest, ms_trace_any;/* summed over bounces                  */
    float ms_shade, ms_raygen;
    uint32_t n_trace_launches;
    /* visit totals of the frame's traversal launches; filled only when the option
     * "count_visits" is on (the counting kernels are slower: never time such a frame) */
    uint64_t nodes_closest, tris_closest, nodes_any, tris_any;
    /* traversal-stack pushes dropped since the scene was created.  crt_scene_create sizes the LDS stack from the
     * validated depth of the tree, so this is 0 for every scene it accepts.  tests/test_walk_ref.py asserts it after every
     * crt_trace mode, frame form, crt_ao_points and crt_fog_segments call on trees whose walks fill that stack to the last
     * entry (DESIGN.md "The walks as tested"); tests/test_lean_build.py, test_camera_rays.py and test_instances_oracle.py
     * assert it on their own scenes */
    uint32_t stack_overflows;
    /* with "count_visits": how many times a WAVE executed the node block / the triangle block of the closest-hit and the
     * any-hit walks (each execution offers 64 lane slots), so nodes_closest / (64 * wave_steps_closest_nodes) is the lane
     * utilisation of that block — the quantity the traversal loops are tuned for */
    uint64_t wave_steps_closest_nodes, wave_steps_closest_tris, wave_steps_any_nodes, wave_steps_any_tris;
    /* with "count_visits": closest-hit rays of the frame that hit something, i.e. the lanes that ran the shading code
     * (path_trace.fs:872-1018); bench.py's instruction model charges the shading instructions to these only */
    uint64_t closest_hits;
    /* with "count_visits": the part of nodes_closest / nodes_any that was visited in UNIFORM node steps — every enabled lane of the
     * wave asked for the same node and shared the direction octant, so the node came through the scalar cache and its decode ran on
     * the scalar unit (first-segment walks; rt_kernels.hip "uniform node steps") */
    uint64_t nodes_closest_uniform, nodes_any_uniform;
} crt_frame_stats;
int crt_get_frame_stats(crt_scene* s, crt_frame_stats* out);
/* structural facts about the device-resident CWBVH */
typedef struct crt_bvh_info {
    uint64_t n_nodes8, n_tris8, n_bvh2_nodes, max_depth8;
    /* build-on-device scenes (CRT_BUILD_LBVH_ON_DEVICE): wall milliseconds of crt_scene_create and of its parts (upload of
     * the input arrays; LBVH and CWBVH conversion as device time); zero for scenes created from host-built arrays */
    uint32_t built_on_device, bvh2_depth;   /* bvh2_depth: deepest leaf level of the BVH2 the scene was given or built, root = 0 */
    float build_wall_ms, build_upload_ms, build_lbvh_device_ms, build_convert_device_ms;
} crt_bvh_info;
int crt_get_bvh_info(crt_scene* s, crt_bvh_info* out);
int crt_device_count(void);
/* Optional, once per process and device (the current HIP device), synchronous: creates the HIP context, loads the library's code
 * objects (traversal kernels, GPU builders, CWBVH converter, scene assembly) and runs the HIP runtime's own first-use set-up (first
 * stream, first copy, first dispatch), so that the first crt_scene_create does not pay for them.  Without it the first
 * crt_scene_create of a process starts a thread that loads the code objects while the scene is uploaded (HIP loads a code object at
 * the first use of one of its kernels: 12.5 ms for the builders', more than the build of a million triangles that follows).  The
 * reference pays the equivalent in Scene::gpu_data, where its shaders are compiled before the first frame (Scene.h:1080-1083,
 * Shader.h:18-97). */
int crt_warmup(void);
/* 1 when the library carries the experimental kernel variants (built with -DCRT_EXPERIMENTS), else 0 */
int crt_has_experiments(void);

/* ------------------------------------------- instanced scenes (needs GPU) -- */

/* Many copies of a mesh and rigid objects that move (no reference counterpart; DXR / Vulkan RT / OptiX call the two levels BLAS and
 * TLAS).  A crt_instances handle is separate from crt_scene: it answers ray queries; frames of it come from a crt_scene bound to it
 * (crt_scene_create_instanced, below).
 *
 * A mesh as a bottom-level structure: positions and triangles in SOURCE order (a triangle's id is its index); only crt_triangle.v[0..2]
 * are read. */
typedef struct crt_blas_desc { const float* vertices; size_t n_vertices; const crt_triangle* triangles; size_t n_triangles; } crt_blas_desc;
/* One instance: world = A * p + t, object_to_world row-major 3x4 (m[r*4 + c], column 3 = t); mesh = index into the create's meshes;
 * mask bits 0..7 = the instance's visibility mask, read by CRT_TRACE_INSTANCE_MASK traces and by the frames of a bound scene whose
 * option "instance_masks" is 1 (bits 8..31 and reserved are ignored); material_offset = what the frames of a bound scene add to the
 * material index of every triangle of the instance's mesh (crt_scene_create_instanced, contract item 3, and its validation rule; ray
 * queries never read it).  64 bytes, mask at offset 52, material_offset at 56. */
typedef struct crt_instance { float object_to_world[12]; uint32_t mesh; uint32_t mask; uint32_t material_offset; uint32_t reserved; } crt_instance;
typedef struct crt_instances crt_instances;
typedef struct crt_instances_info {
    uint32_t n_meshes, n_instances, capacity;
    uint32_t stack_entries;                   /* traversal-stack entries a ray may use: TLAS depth + deepest BLAS depth */
    uint32_t tlas_nodes8, tlas_depth8, max_blas_depth8;
    uint32_t stack_overflows;                 /* dropped stack pushes since create (0 unless something is wrong) */
    uint64_t blas_nodes8, blas_tris;          /* every mesh once, whatever the instance count */
    uint64_t blas_bytes, tlas_bytes, instance_bytes;   /* device bytes: BLAS nodes + records; TLAS region for `capacity`; per-instance buffers */
    uint64_t tlas_build_bytes;                /* device bytes kept for the sets: the TLAS builder's temporaries and node staging for `capacity` */
    float set_device_ms, set_wall_ms;         /* the last create / set / refit: device time of its kernels, host wall time of the call */
    float create_wall_ms, reserved_f;
} crt_instances_info;

/* Builds every mesh ONCE on the device with crt_scene_create's build-on-device path (build_flags: CRT_BUILD_* as crt_scene_desc; the
 * CRT_BUILD_LBVH_ON_DEVICE bit is implied), packs all BLAS node8s behind a TLAS region sized for `capacity` (0 = n_instances) into one
 * array and all triangle records into another, then sets the n_instances instances (crt_instances_set).  n_instances may be 0: every
 * ray then misses.  One mesh shared by many instances costs the memory of one. */
int crt_instances_create(const crt_blas_desc* meshes, uint32_t n_meshes, const crt_instance* instances, uint32_t n_instances,
                         uint32_t capacity, uint32_t build_flags, crt_instances** out);
/* crt_instances_create's build_flags only (bits 0..15 are crt_scene_desc's): keep the state crt_instances_update_meshes needs.  Without
 * it a handle allocates nothing for updates and every update returns CRT_ERR_INVALID. */
enum { CRT_INSTANCES_UPDATABLE = 1u << 16 };
/* New instances (n <= capacity; the count may change, 0 allowed).  Every instance is checked on the device first: a non-finite matrix,
 * a singular one or one whose inverse is not finite, a mesh index out of range, a world box beyond 1e18, or n > capacity returns
 * CRT_ERR_INVALID and leaves the previous instances tracing exactly as before.  Then per instance: world_to_object, the world box and
 * the record; the TLAS is rebuilt on the device from the world boxes (binned SAH, then the CWBVH converter).  TLAS depth + deepest BLAS
 * depth beyond the walk's stack (40 entries) returns CRT_ERR_LIMIT, also leaving the previous state.  Synchronous. */
int crt_instances_set(crt_instances* s, const crt_instance* instances, uint32_t n_instances);
/* the same with the crt_instance array in HBM on the handle's device (e.g. written by the caller's animation kernel); the check runs
 * on the device, the host waits once for its verdict.  Returns when the set is done (sync is accepted for symmetry with the other
 * *_device calls). */
int crt_instances_set_device(crt_instances* s, const void* d_instances, uint32_t n_instances, int sync);
/* Moving instances without a TLAS rebuild (the top-level update of DXR / Vulkan RT / OptiX): n_instances must equal the
 * live count, and each instance may change its matrix and its mesh.  The TLAS keeps its topology (the same node8s, the same leaf slots,
 * each leaf slot the same instance index); only the node8 origins, exponents and quantised boxes are refitted, on the device, to the new
 * world boxes.  The checks are those of a set, run on the device first (finite and non-singular matrix, finite inverse, mesh in range,
 * world box within 1e18): a failed one, a count other than the live count or a null pointer returns CRT_ERR_INVALID, and nothing the
 * walk reads has changed.  CRT_ERR_LIMIT cannot happen (the stack bound is TLAS depth + deepest BLAS, and a refit changes neither).
 * world_to_object, the world boxes and the instance records are the bits a crt_instances_set of the same array produces; closest hits
 * (t, u, v, tri, instance) equal those of such a set bit for bit, the grazing-margin exception of crt_instances_trace aside, since the
 * closest hit does not depend on the tree.  Per-ray node counts may differ, and the walk slows as the instances move away from the
 * placement the TLAS was built for: call crt_instances_set to rebuild.  An updatable handle keeps the refitted array as its live
 * instances (crt_instances_update_meshes starts from it).  The first refit after a create, set or update finds the TLAS's levels (one
 * more host wait and a temporary allocation); later refits allocate nothing.  Synchronous, with one host wait for the verdict; the
 * device form's sync is accepted for symmetry.  crt_instances_info's set_device_ms / set_wall_ms then describe the refit. */
int crt_instances_refit(crt_instances* s, const crt_instance* instances, uint32_t n_instances);
int crt_instances_refit_device(crt_instances* s, const void* d_instances, uint32_t n_instances, int sync);
/* crt_instances_trace's mode bit (instanced traces only; crt_trace refuses it): instance visibility masks (as DXR /
 * Vulkan RT / OptiX).  The low 8 bits of a ray's pad word are its mask; an instance is visible to the ray iff (mask & ray mask) != 0,
 * so an instance of mask 0 is never hit by a masked ray and a ray of mask 0 hits nothing. */
enum { CRT_TRACE_INSTANCE_MASK = 8 };
/* Closest- or any-hit queries (mode CRT_TRACE_CLOSEST or CRT_TRACE_ANY, optionally | CRT_TRACE_INSTANCE_MASK; anything else is
 * CRT_ERR_INVALID) over host rays.
 * hits[i].tri = the triangle id within the mesh of instance_of_hit[i] (-1 and -1 on a miss); instance_of_hit and stats may be NULL.
 * Numerical contract (tests/test_instances.py holds the kernel to it bit for bit):
 *   - world_to_object (crt_instance_inverse) is computed in double and rounded once to float: the adjugate of A divided by det(A),
 *     det expanded along the first row in the order written, translation 0 - (W_A . t) from the unrounded entries (0 -, so that the
 *     identity maps to the identity bits).  Written out, with A = (a b c / d e f / g h i), every operation one IEEE double operation:
 *     c00 = e*i - f*h, c01 = f*g - d*i, c02 = d*h - e*g; det = (a*c00 + b*c01) + c*c02; the adjugate's rows are
 *     (c00, c*h - b*i, b*f - c*e), (c01, a*i - c*g, c*d - a*f), (c02, b*g - a*h, a*e - b*d); W_A = each entry / det (a division, not a
 *     multiplication by 1 / det); translation of row (x y z): 0 - ((x*t0 + y*t1) + z*t2) (tests/instanced_ref.py restates it).
 *   - the object ray, each component in fp32 without fma: o'_r = ((W_r0*o.x + W_r1*o.y) + W_r2*o.z) + W_r3,
 *     d'_r = (W_r0*d.x + W_r1*d.y) + W_r2*d.z; d' is NOT renormalised, so t is the same parameter in both spaces and tmax carries over.
 *     An instance whose object_to_world is bitwise the identity uses o' = o, d' = d (signs of zeros kept: exactly a flat trace).
 *   - inside a mesh the crt_trace contract holds unchanged (CWBVH walk, Moller-Trumbore, clamped slab directions); an origin that is not
 *     finite, in world or in object space, hits nothing there.
 *   - closest hit = the minimum of (t, instance index, triangle id), lexicographically, over all hits with 0 <= t < tmax: independent of
 *     the order the TLAS visits instances.  EXCEPTION (equal t only): once a hit at t is held, a BLAS box whose computed entry distance
 *     rounds above t is culled, so an equal-t hit inside it (coincident geometry in two instances) is not compared and the instance
 *     found first keeps the hit.  Any hit: tri = 0 / -1 as crt_trace, instance_of_hit = SOME instance with a hit in [0, tmax).
 *   - world boxes: the 8 corners of the mesh's float vertex box through object_to_world in double, widened by 2^-16 of the largest
 *     absolute coordinate and rounded outward (crt_instance_world_box; DESIGN.md §11 sizes the margin).  The TLAS tests the WORLD ray
 *     against these boxes while the hit is found on the rounded OBJECT ray, so the margin must cover that rounding.  It does when
 *     cond_inf(A) * (2 |o|_inf + B + |t|_inf) <= 51 B, B = the largest absolute coordinate of the instance's exact world box, t its
 *     translation.  EXCEPTION: beyond that bound (a ray from far away relative to B, e.g. a small instance near the origin seen from
 *     ~1000x its size, or a badly conditioned A) a grazing hit within a few ulps of the box's surface can be culled by the TLAS, and
 *     the closest / any hit above then misses it.
 *   - stats: nodes = TLAS + BLAS node8 steps, tris = triangle tests, each clamped at 65535.
 * With CRT_TRACE_INSTANCE_MASK the rules above hold over the instances visible to each ray only: the closest hit is the minimum of
 * (t, instance index, triangle id) over the visible instances, an any hit reports some visible instance, and the grazing-margin exception
 * applies unchanged.  A TLAS child whose instances are all hidden from the ray is not entered, and a hidden instance is skipped before
 * its ray is transformed: stats count only the steps actually taken.  Without the bit, masks are ignored and the results, instance ids
 * and stats are those of the same call before masks existed.  Sets, refits (e.g. the same matrices with new masks: showing and hiding
 * instances without a TLAS rebuild) and updates (which keep the live masks) all carry them; the first masked trace after any of them
 * first recomputes the TLAS's per-child masks on the handle's stream (two small kernels, no host wait). */
int crt_instances_trace(crt_instances* s, const crt_ray* rays, size_t n, crt_hit* hits, int32_t* instance_of_hit, int mode, crt_ray_stats* stats);
/* the same with DEVICE pointers; asynchronous on the handle's stream unless sync != 0 */
int crt_instances_trace_device(crt_instances* s, const void* d_rays, size_t n, void* d_hits, void* d_instance_of_hit, int mode, void* d_stats, int sync);
int crt_instances_get_info(crt_instances* s, crt_instances_info* out);
/* Moving meshes under an updatable handle (CRT_INSTANCES_UPDATABLE): new positions for n DISTINCT meshes in one call,
 * vertices[k] = float xyz of mesh mesh_ids[k] in the create's order, n_vertices[k] = the create's count.  The topology is kept: within
 * each updated BLAS the node8 boxes are re-quantised (byte-identical to crt_cwbvh_refit of that BLAS with its bases un-rebased) and the
 * records get new v0, e1, e2 (make_record's fp32 subtractions; the w words stay).  The mesh box becomes the box of the vertices its
 * triangles reference, under the total order of the floats (-0 below +0, for lo and hi alike; create keeps the value seen first of two
 * equal zeros, so the two agree whenever the mesh box has no signed-zero tie).  Every instance of an updated mesh gets its new world box
 * (crt_instance_world_box), and the TLAS is rebuilt from all boxes as crt_instances_set does; instances, world_to_object and the other
 * meshes stay.  All or nothing: a coordinate that is not finite or exceeds 1e18 (any of the n arrays' vertices), a wrong count, a mesh
 * index out of range or repeated, a null pointer, a handle without CRT_INSTANCES_UPDATABLE, or a world box beyond 1e18 returns
 * CRT_ERR_INVALID; TLAS depth + deepest BLAS beyond the walk's 40 entries returns CRT_ERR_LIMIT.  Either way nothing the walk reads has
 * changed and the previous geometry traces on bit for bit.  Closest hits after an update to V equal those of a fresh crt_instances_create
 * from V (the minimum of (t, instance, id) does not depend on the tree), the grazing-margin exception above aside.  Synchronous. */
int crt_instances_update_meshes(crt_instances* s, const uint32_t* mesh_ids, uint32_t n, const float* const* vertices, const size_t* n_vertices);
/* the same with the positions in HBM on the handle's device (mesh_ids, n_vertices and the pointer array itself are host memory).  Returns
 * when the update is done; sync is accepted for symmetry. */
int crt_instances_update_meshes_device(crt_instances* s, const uint32_t* mesh_ids, uint32_t n, const void* const* d_vertices, const size_t* n_vertices,
                                       int sync);
/* device ms and host wall ms of the last update (CRT_ERR_INVALID before the first one) and the device bytes the refit state holds
 * (filled for an updatable handle even then; 0 otherwise).  Any pointer may be NULL. */
int crt_instances_last_update(crt_instances* s, float* device_ms, float* wall_ms, uint64_t* state_bytes);
/* Changing which geometry a live handle holds.  Both calls are synchronous, may allocate and free device memory (they
 * are not per-frame calls), build with the builder given at create, and leave the packed arrays as crt_instances_create lays them out
 * for the resulting mesh list: the TLAS region, then the BLASes in mesh index order without gaps, child and triangle bases rebased;
 * records likewise.  Each mesh is checked as create checks it, before any device work: non-null and non-empty, every vertex index in
 * range, every referenced coordinate finite and within 1e18 (CRT_ERR_INVALID), fewer than 2^28 triangles (CRT_ERR_LIMIT).  A packed
 * node or record array of 4 GiB or more, or TLAS depth + deepest BLAS beyond the walk's 40 entries, returns CRT_ERR_LIMIT.  All or
 * nothing: after any refusal (CRT_ERR_NOMEM included) nothing the walk reads, no debug read and no crt_instances_get_info field other
 * than the times has changed, and the previous geometry traces on bit for bit.  n == 0 is CRT_OK and changes nothing.  Hits after either
 * call equal those of a fresh crt_instances_create from the resulting mesh list and the live instances (the minimum of (t, instance, id)
 * does not depend on the tree), the grazing-margin exception above aside.  crt_instances_info's set_device_ms / set_wall_ms then
 * describe the call.
 *
 * crt_instances_add_meshes appends n meshes; *first_id (may be NULL) receives the index of the first, the others follow.  Instances, the
 * TLAS and every existing BLAS stay as they are and where they are: debug reads 0, 1, 2, 3 and 6 are byte for byte what they were, reads
 * 4 and 5 keep their old content as a prefix, and every trace returns the same bits and per-ray stats.  The next set / refit may name
 * the new meshes.  Any handle; an updatable one accepts the new meshes in crt_instances_update_meshes at once. */
int crt_instances_add_meshes(crt_instances* s, const crt_blas_desc* meshes, uint32_t n, uint32_t* first_id);
/* crt_instances_replace_meshes gives n DISTINCT existing meshes new geometry (vertex and triangle counts may differ from before): each
 * listed BLAS is rebuilt from scratch (the remedy for a BLAS that crt_instances_update_meshes has deformed far from the placement its
 * tree was built for), the meshes behind a resized one shift, the mesh boxes become those of the new geometry, and the live instances
 * get new records (the new BLAS roots), new world boxes and a rebuilt TLAS as after crt_instances_update_meshes; instances, their masks
 * and world_to_object stay.  CRT_INSTANCES_UPDATABLE handles only (the world boxes are recomputed from the live instances, which only
 * such a handle keeps).  Also CRT_ERR_INVALID: a mesh index out of range or repeated, a null pointer, a handle without the flag, a
 * world box beyond 1e18. */
int crt_instances_replace_meshes(crt_instances* s, const uint32_t* mesh_ids, uint32_t n, const crt_blas_desc* meshes);
/* test hook: which 0 = world_to_object (12 floats per instance, instance order), 1 = world boxes (6 floats: lo, hi), 2 = TLAS node8s
 * (80 B), 3 = instance records in TLAS leaf order (64 B: world_to_object rows, then BLAS root node, instance index, identity flag, mask & 0xff),
 * 4 = every BLAS node8 (80 B; the packed region after the TLAS region, bases rebased), 5 = every BLAS record (48 B), 6 = the TLAS child
 * masks (8 B per TLAS node8, byte i = the OR of the masks & 0xff of every instance under meta slot i; recomputed first if stale), 7 = the
 * live object_to_world (12 floats per instance, instance order, as the last successful set / refit gave them; read by the light tables of
 * DESIGN.md §18, never by ray queries).
 * dst may be NULL to query the count. */
int crt_instances_debug_read(crt_instances* s, int which, void* dst, size_t cap_bytes, size_t* n_out);
/* crt_tree_cost (above) of the handle's live trees, computed on its device: mesh = -1 the TLAS (nodes [0, tlas_nodes8), root 0; all
 * zeros for a handle with 0 instances), mesh = m the BLAS of mesh m (its slice of the packed node array, its own root); any other mesh
 * is CRT_ERR_INVALID.  Any handle.  Waits for the handle's stream and for bound scenes' queued frames; synchronous.  After
 * crt_instances_refit compare the TLAS's cost with that of a crt_instances_set of the same array, after crt_instances_update_meshes a
 * BLAS's with that of a crt_instances_replace_meshes: "as the tree ages" in the comments above means this ratio. */
int crt_instances_tree_cost(crt_instances* s, int32_t mesh, crt_tree_cost* out);
int crt_instances_destroy(crt_instances* s);

/* ---- frames of an instanced scene ----
 *
 * A crt_scene whose geometry is a LIVE crt_instances handle.  Every frame-side entry point (crt_set_camera, crt_render_frame[s][_async],
 * crt_sync, crt_reset, crt_read_sum, crt_sum_device, crt_resolve[_device], crt_set_shard, the crt_packed_* calls, crt_get_frame_stats,
 * crt_get_launch_times, crt_debug_read_queue) works on it as on any scene.
 *
 * What the shading reads of one mesh, in the handle's mesh order; copied.  triangles: n_triangles == the mesh's triangle count, in SOURCE
 * order (a hit's id indexes it); v[3] = material, vn / vt as in crt_scene_desc, indexing THIS mesh's normals / texcoords (object space). */
typedef struct crt_mesh_shading {
    const crt_triangle* triangles; size_t n_triangles;
    const float* normals;   size_t n_normals;
    const float* texcoords; size_t n_texcoords;
} crt_mesh_shading;
typedef struct crt_instanced_scene_desc {
    uint32_t abi_version;                                /* CRT_ABI_VERSION */
    crt_instances* instances;                            /* BORROWED: must outlive the scene */
    const crt_mesh_shading* meshes; uint32_t n_meshes;   /* == the handle's mesh count */
    const crt_material* materials; size_t n_materials;   /* shared by all meshes, as crt_scene_desc */
    const crt_light* lights; size_t n_lights;            /* WORLD space */
    const uint8_t* albedo_textures; uint32_t tex_width, tex_height, n_textures;
    uint32_t width, height, max_depth;
} crt_instanced_scene_desc;
/* Checks are crt_scene_create's for the same arrays, each per mesh (CRT_ERR_INVALID): the counts, the vn indices where vn.w != 0, the vt
 * indices of textured materials, the material indices, finite normals.
 *
 * Binding:
 *   - The scene reads the handle's LIVE arrays when a frame is enqueued: crt_instances_set / _refit / _update_meshes (and their device
 *     forms) between frames change what the next frame sees.  Call crt_reset as after a camera move: the sum is not cleared for them.
 *     Each of these mutators, on a handle with a bound scene, first waits for that scene's stream, so a frame queued with *_async never
 *     reads arrays a mutator is rewriting.
 *   - While a scene is bound, crt_instances_destroy, crt_instances_add_meshes and crt_instances_replace_meshes return CRT_ERR_INVALID and
 *     change nothing (the scene's per-mesh tables would go stale).  crt_scene_destroy unbinds.  A handle without a bound scene behaves
 *     exactly as before.
 *   - On such a scene these return CRT_ERR_INVALID (crt_last_error says why): crt_trace* (use crt_instances_trace), crt_update_vertices*,
 *     crt_debug_read_accel, crt_debug_time_graph, crt_set_devices with more than one entry, option "streams" other than 0 / 1, option
 *     "accel" other than 0.  "jitter", "count_visits" (0 / 1) and "timing" work; the other tuning options are accepted and have no effect
 *     (results never depend on them); "adaptive_tiles" is treated as 0 (the per-tile clock lives in the fused first-segment kernel, which
 *     this path does not run).  crt_get_bvh_info reports the TLAS + BLAS totals of the handle's crt_instances_get_info.
 *
 * Numerical contract (tests/test_instances_frames.py holds the kernels to it):
 *   1. Primary rays, RNG, NEE, MIS, materials, textures, the sum and the resolve are the flat frame path's, bit for bit (the shading is
 *      the same source).
 *   2. The closest hit of every path ray and the occlusion of every shadow ray are crt_instances_trace's (CRT_TRACE_CLOSEST /
 *      CRT_TRACE_ANY on the same ray, tmax = the flat path's: 1e9 for path rays, distance to the light sample - 1e-4 for shadow rays):
 *      the minimum of (t, instance, id), with the equal-t and grazing-margin exceptions documented there.  With option "instance_masks"
 *      0 (the default) without the mask bit; with 1, | CRT_TRACE_INSTANCE_MASK with the ray mask of the ray's class: "mask_primary" for
 *      the path rays of segment 0, "mask_bounce" for those of every later segment, "mask_shadow" for every NEE shadow ray.  Visibility
 *      is (instance.mask & ray mask) != 0, so with the option on an instance of mask 0 is in no picture.
 *   3. The material is triangles[id].v[3] of the hit instance's mesh + the instance's material_offset, an index into the scene's one
 *      material table; everything that follows from a material (emission and its light index, type, texture, Disney parameters) follows
 *      from that sum.  u, v, t are used as returned; hit_point = (o + d*t) + n*0.0002f on the WORLD ray.
 *   4. The normal: n_obj is what the flat path computes from that mesh's vn / normals (interpolated, or the truncated geometric normal;
 *      not normalised).  An instance whose record carries the identity flag: n = n_obj.  Otherwise, with W_r the rows of world_to_object,
 *      in fp32 without fma: m_c = (W_0c*n_obj.x + W_1c*n_obj.y) + W_2c*n_obj.z (the inverse transpose of A applied to n_obj), then
 *      n = m * (|n_obj| / |m|), |x| = sqrt((x.x*x.x + x.y*x.y) + x.z*x.z), IEEE sqrt and division, and n = m when |m| is 0 or not finite.
 *      A shading normal so keeps its file's length whatever the instance's scale, as in a flat scene, and a matrix that is numerically
 *      the identity gives n_obj back bit for bit.
 *
 * Material offsets, never an out-of-range read.  With lo / hi the least / greatest v[3] of a mesh's triangles, an instance
 * with a non-zero material_offset is acceptable to a scene iff material_offset < 2^31 and hi + material_offset < n_materials, and either
 * every triangle's vt of its mesh indexes that mesh's texcoords or no material in [lo + offset, hi + offset] is textured (texture layer
 * other than -1).  Offset 0 is exempt: the per-triangle checks above cover it.  crt_scene_create_instanced applies the rule to the
 * handle's live instances; crt_instances_set* / crt_instances_refit* on a handle with bound scenes apply it for every bound scene, on the
 * device, to the instances they are given, before anything is published: a refused call returns CRT_ERR_INVALID (crt_last_error names
 * the instance and the rule) and has changed nothing.  A handle without a bound scene stores any offset unchecked.
 *
 * Visibility masks, options of an instanced scene (crt_set_option; refused on any other scene like an unknown name, and
 * for a value out of range, CRT_ERR_INVALID): "instance_masks" 0 (default: frames ignore masks) / 1, "mask_primary", "mask_bounce",
 * "mask_shadow" 0..255 (default 255).  Call crt_reset after changing one, as after a camera move.  With "count_visits" the node and
 * triangle totals of a masked frame count the steps taken: a culled TLAS child and a hidden instance cost nothing.
 *
 * Not offered: per-ray masks inside a class, several devices or streams, several samples per launch.  Lights that
 * follow an emissive instance: crt_scene_create_instanced_lit, below. */
int crt_scene_create_instanced(const crt_instanced_scene_desc* desc, crt_scene** out);

/* ---- lights that follow emissive instances ----
 *
 * desc->lights are world-space constants.  A mesh may carry lights of its own, in OBJECT space (copied): every instance of the mesh then
 * has them, moved by its object_to_world, and crt_instances_set / _refit / _update_meshes (and their device forms) move them with the
 * instance.  The scene's WORLD light table holds desc->lights first (n_static, as given), then, instance by instance in instance order,
 * the lights of that instance's mesh in the mesh's order; first[i] = n_static + the lights of the instances before i.  The table is
 * rebuilt on the device, on the scene's stream, from the handle's live matrices: lazily, when a frame is enqueued or crt_scene_read_lights
 * is called after a successful mutator of the handle (or crt_scene_set_mesh_lights), with one small device-to-host read for the total.
 * Call crt_reset after a mutator, as ever.
 *
 * One transformed light, fp32 without fma, A | t the rows of object_to_world, W the handle's world_to_object (crt_instance_inverse):
 *   p'_r = ((A_r0*p.x + A_r1*p.y) + A_r2*p.z) + t_r;  u'_r = (A_r0*u.x + A_r1*u.y) + A_r2*u.z, v' likewise;
 *   m_c = (W_0c*n.x + W_1c*n.y) + W_2c*n.z (contract item 4's inverse transpose: the light's side follows the shading normal, mirrors
 *   included), n' = m * (1 / sqrt((m.x*m.x + m.y*m.y) + m.z*m.z)), IEEE square root and division;  e copied;
 *   area' = sqrt(dot(c, c)), c = u' x v' (each component a*b - c*d, both products rounded);  area_pdf[2] = 0.
 *   An instance whose matrix is bitwise the identity copies all 18 floats, area included.
 * The pdf column is recomputed for the WHOLE table (a static light's given area_pdf[1] is ignored once a scene has mesh lights):
 *   a_k = the light's area, or +0 when that is not a finite positive float;  S = the pairwise tree sum of a_0 .. a_{n-1} (padded with +0
 *   to a power of two, a_j <- a_{2j} + a_{2j+1} until one is left);  area_pdf[1] = a_k * (1.0f / S) when S > 0, else 0.
 * crt_instance_lights and crt_lights_finish are this arithmetic on the host, bit for bit.
 *
 * Shading.  NEE samples the table.  An emitter hit looks its light up by ew = (int)material.emission[3] of the hit's material (contract
 * item 3): when the hit instance's mesh has nl > 0 lights, ew is MESH-LOCAL and the light is first[instance] + min(ew, nl - 1); on any
 * other mesh it is min(ew, total - 1), a table index (a static light when ew < n_static); with an empty table the hit's MIS weight is 1.
 * The clamp only keeps a material offset from causing an out-of-range read: the area cancels in the light's pdf, so a clamped index
 * changes the rounding alone.
 *
 * Lights are not geometry: an instance hidden by a visibility mask ("instance_masks") still lights the scene.
 *
 * crt_scene_create_instanced_lit: mesh_lights = desc->n_meshes entries (n_lights may be 0, lights then ignored), or NULL, or every entry
 * empty = crt_scene_create_instanced exactly (nothing new is allocated or launched, the frames keep their bits).  Besides that call's
 * checks, CRT_ERR_INVALID and nothing created for: a light field (static or mesh) that is not finite; an emissive material with
 * ew < 0 or ew >= max(n_static, the greatest nl); a triangle of a light-bearing mesh whose own material is emissive with ew >= nl; a
 * triangle of a light-less mesh whose own material is emissive with ew >= n_static. */
/* (a struct TAG only, written `struct crt_mesh_lights`: the loader's accessor crt_mesh_lights() below already owns the plain name) */
struct crt_mesh_lights { const crt_light* lights; size_t n_lights; };   /* OBJECT space, copied */
int crt_scene_create_instanced_lit(const crt_instanced_scene_desc* desc, const struct crt_mesh_lights* mesh_lights, crt_scene** out);
/* replaces ONE mesh's object-space lights (n_lights == the count given at create), e.g. after crt_instances_update_meshes deformed the
 * lamp; the table is rebuilt before the next frame; call crt_reset.  CRT_ERR_INVALID and nothing changed: a scene without mesh lights
 * (flat scenes included), a mesh out of range, another count, a field that is not finite, a null pointer with n_lights > 0. */
int crt_scene_set_mesh_lights(crt_scene* s, uint32_t mesh, const crt_light* lights, size_t n_lights);
/* the scene's CURRENT world light table (rebuilt first if stale): *n_out = its count, up to cap lights copied to dst (dst may be NULL to
 * query the count; cap below the count with dst given is CRT_ERR_INVALID).  Instanced scenes only; one without mesh lights returns
 * desc->lights as given.  Synchronous. */
int crt_scene_read_lights(crt_scene* s, crt_light* dst, size_t cap, size_t* n_out);

/* --------------------------------------------------- host side ([host]) ----- */

/* Caitlyn/Camera.h:7-19 Camera(pos, lookAt, fovDeg) + updateCamera :48-58 [host] */
int crt_camera_look_at(const float pos[3], const float look_at[3], float fov_deg, crt_camera* out);
/* The instance arithmetic of crt_instances_* on the host, bit for bit what the device computes: world_to_object of object_to_world
 * (CRT_ERR_INVALID for a non-finite or singular matrix or a non-finite inverse), and the world box (lo[3], hi[3]) of an object box. */
int crt_instance_inverse(const float object_to_world[12], float world_to_object[12]);
int crt_instance_world_box(const float object_to_world[12], const float box[6], float out[6]);
/* The light arithmetic of crt_scene_create_instanced_lit on the host, bit for bit what the device computes [host].  crt_instance_lights:
 * n object-space lights through object_to_world (its inverse as crt_instance_inverse, CRT_ERR_INVALID where that refuses): out's area is
 * set, area_pdf[1] = area_pdf[2] = 0; a matrix that is bitwise the identity copies the lights.  in and out may be the same array.
 * crt_lights_finish: fills area_pdf[1] of a whole table by the tree-sum rule. */
int crt_instance_lights(const float object_to_world[12], const crt_light* in, size_t n, crt_light* out);
int crt_lights_finish(crt_light* lights, size_t n);

/* Caitlyn/Rnd.h:21-40 PCG_Hash / randf2 (state starts at 1, Rnd.h:7) [host] */
uint32_t crt_pcg_hash(uint32_t x);
float    crt_randf2(uint32_t* state);

/* SBVH builder, Caitlyn/sbvh.h:99-153 SBVH(trs, vertices) [host].
 * Reorders into leaf order with spatial-split duplicates.  flags bit0: disable spatial
 * splits (pure SAH sweep, "SAH BVH" of config 1).  A node for which no split is priced below the builder's 1e20 "no split yet" value
 * (a scene some 10^9 units wide: area times count reaches it) is split at the median of its widest axis; the reference's rule gave such
 * a node an empty left child and itself as the right one, without end.  A node whose references all have the same box
 * (coincident triangles) takes the object split even with spatial splits on: no plane separates them, and clipping every one into both
 * children doubled the references level by level (300 coincident triangles: more than 2^24 nodes).  References that only nearly
 * coincide are still duplicated down to the reference's overlap threshold (1e-5 of the root's area): on the order of a thousand references each. */
typedef struct crt_sbvh crt_sbvh;
int crt_sbvh_build(const crt_triangle* tris, size_t n_tris, const float* vertices, size_t n_vertices,
                   uint32_t flags, crt_sbvh** out);
size_t crt_sbvh_num_nodes(const crt_sbvh*);            /* flat_nodes.size()        */
size_t crt_sbvh_num_slots(const crt_sbvh*);            /* triangle_indices.size()  */
const crt_flatnode* crt_sbvh_nodes(const crt_sbvh*);   /* sbvh.h:570-609 BFS order */
const int32_t*      crt_sbvh_triangle_indices(const crt_sbvh*); /* slot -> original triangle */
const crt_triangle* crt_sbvh_triangles(const crt_sbvh*);        /* reordered trs, sbvh.h:130-139 */
void crt_sbvh_free(crt_sbvh*);

/* GPU BVH construction (needs a GPU).  A linear BVH (Morton codes, device radix sort, Karras'
 * radix tree, bottom-up refit) in the same FlatNode/leaf-order layout, returned through the same handle as
 * crt_sbvh_build so either builder can feed crt_scene_desc.bvh / crt_cwbvh_convert.  Not the reference's
 * SBVH: no SAH and no spatial splits — a different, lower-quality tree built ~100x faster. */
/* flags = 0: linear BVH.  flags = CRT_GPU_BUILD_PLOC | (radius << 8): parallel locally-ordered clustering (Meister & Bittner
 * 2018) over the same Morton order — mutual nearest neighbours within `radius` cluster positions (1..64, 0 = 16) merge
 * bottom-up; a SAH-quality tree for a few more milliseconds of device time. */
enum { CRT_GPU_BUILD_PLOC = 2,
       /* flags = CRT_GPU_BUILD_SAH: top-down surface-area-heuristic build, the GPU counterpart of the reference's sweep
        * (sbvh.h:338-378) without spatial splits: 16 bins per axis breadth-first down to `t` triangles per node (bits 8..15,
        * 8..32, 0 = 8), the exact sweep over all three axes below.  Tree quality of the host SBVH (node visits per ray
        * within 1 %) in ~5 ms of device time at 1 M triangles instead of seconds */
       CRT_GPU_BUILD_SAH = 4 };
int  crt_lbvh_build(const crt_triangle* tris, size_t n_tris, const float* vertices, size_t n_vertices,
                    uint32_t flags, crt_sbvh** out);
void crt_lbvh_last_build_ms(float* device_ms, float* total_ms);

/* CWBVH converter, Caitlyn/cwbvh.h:58-73 CWBVH::convert(SBVH&) with the defects of
 * SURVEY 8a corrected (appendix C) [host].  Defined rule by rule in DESIGN.md §24.  The cost tables are formed from extents scaled by a
 * power of two taken from the root box, so the result does not depend on the scale of the scene: coordinates times 2^k give the same
 * tree with p times 2^k and e + k.  Cost domain: with every box inside the root's, no summed cost exceeds 12 * 3 * 2^24; an array in
 * which one reaches 1e20 (a box some 10^5 root extents wide) is refused, CRT_ERR_INVALID "boxes out of the cost range".  Also
 * CRT_ERR_INVALID: a leaf of more than 3 triangles, a leaf range outside n_slots, a child link that is not beyond its node and inside the
 * array, slots not covered exactly once.  Children must follow their parents; the device form below also requires breadth-first order
 * and returns CRT_ERR_LIMIT beyond 64 node8 levels or 4096 BVH2 levels, which this one accepts. */
typedef struct crt_cwbvh crt_cwbvh;
int crt_cwbvh_convert(const crt_flatnode* bvh2, size_t n_nodes, size_t n_slots, crt_cwbvh** out);
/* The same conversion on the GPU (needs a GPU): byte-identical node, triangle-slot and child arrays
 * (the per-node arithmetic is shared source, host/cwbvh_core.hpp), returned through the same handle. */
int  crt_cwbvh_convert_device(const crt_flatnode* bvh2, size_t n_nodes, size_t n_slots, crt_cwbvh** out);
void crt_cwbvh_last_convert_ms(float* device_ms, float* total_ms);
size_t crt_cwbvh_num_nodes(const crt_cwbvh*);
size_t crt_cwbvh_num_tris(const crt_cwbvh*);
const crt_node8* crt_cwbvh_nodes(const crt_cwbvh*);
const int32_t*   crt_cwbvh_tri_slots(const crt_cwbvh*);  /* CWBVH order -> BVH2 leaf slot */
/* 8 entries per node8: the BVH2 node each child slot stands for (-1 = empty); for validators */
const int32_t*   crt_cwbvh_child_bvh2(const crt_cwbvh*);
uint32_t crt_cwbvh_depth(const crt_cwbvh*);
void crt_cwbvh_free(crt_cwbvh*);

/* Host refits [host]: in place, new boxes from new vertex positions, topology unchanged — the reference implementation the
 * device refit of crt_update_vertices is compared with (same bytes).  BVH2: leaf boxes are the unions of the full vertex boxes
 * of their slots' triangles (spatial-split duplicates get the full box), inner boxes the union of their two children.  CWBVH:
 * leaf slots likewise from tri_slots, inner slots from their child node8; every node8 is re-encoded with the converter's
 * pick_exponent / quant_lo / quant_hi against the union of its slot boxes; meta, imask and both base indices stay.
 * leaf_tris are the triangles in BVH2 leaf order (crt_sbvh_triangles).  Non-finite vertices -> CRT_ERR_INVALID, nothing written. */
int crt_bvh2_refit(crt_flatnode* nodes, size_t n_nodes, const crt_triangle* leaf_tris, size_t n_slots,
                   const float* vertices, size_t n_vertices);
int crt_cwbvh_refit(crt_node8* nodes, size_t n_nodes8, const int32_t* tri_slots, size_t n_tris8,
                    const crt_triangle* leaf_tris, size_t n_slots, const float* vertices, size_t n_vertices);
/* crt_tree_cost (defined with crt_get_tree_cost) of the node8s [first, first + count) of a host array, `root` among them [host]:
 * the reference of the device kernel.  count == 0 returns all zeros; a null pointer or a root outside the range is CRT_ERR_INVALID. */
int crt_cwbvh_cost(const crt_node8* nodes, size_t first, size_t count, size_t root, crt_tree_cost* out);

/* OBJ/MTL loader, Caitlyn/Scene.h:742-926 Read_Object (+ ReadMtl :507-596; textures
 * not loaded) [host].  Applies the -vertex_min translation (:915-925) to vertices,
 * light origins and *camera_position (may be NULL). */
typedef struct crt_mesh crt_mesh;
int crt_load_obj(const char* path, float camera_position[3], crt_mesh** out);
size_t crt_mesh_counts(const crt_mesh*, size_t* n_vertices, size_t* n_normals, size_t* n_texcoords,
                       size_t* n_triangles, size_t* n_materials, size_t* n_lights);
const float*        crt_mesh_vertices(const crt_mesh*);
const float*        crt_mesh_normals(const crt_mesh*);
const float*        crt_mesh_texcoords(const crt_mesh*);
const crt_triangle* crt_mesh_triangles(const crt_mesh*);
const crt_material* crt_mesh_materials(const crt_mesh*);
const crt_light*    crt_mesh_lights(const crt_mesh*);
const float*        crt_mesh_vertex_min(const crt_mesh*);   /* pre-translation minimum */
/* map_Kd textures of the .mtl as the RGB8 array the reference uploads (Scene.h:597-710, :1065-1078): n_layers
 * layers of height x width x 3 bytes, layer = crt_material.tex_ind[0]; NULL when the scene has none.  Feeds
 * crt_scene_desc.albedo_textures / tex_width / tex_height / n_textures. */
const uint8_t*      crt_mesh_albedo_textures(const crt_mesh*, int32_t* width, int32_t* height, int32_t* n_layers);
void crt_mesh_free(crt_mesh*);

/* Texture files [host].  crt_image_decode: what `stbi_load(name, &w, &h, 0, 3)` hands the reference (Scene.h:619)
 * for PNG, BMP, TGA, binary PNM and JPEG (baseline and progressive): 8-bit RGB, top row first, byte for byte what
 * the reference's vendored stb_image returns (tests/golden/stb_decodes.npz).  Call with rgb = NULL to get the size;
 * GIF/PSD/PIC/HDR and damaged files are refused (CRT_ERR_INVALID).
 * crt_texture_to_array_bytes: the reference's bilinear resize to the texture-array size and its float -> byte
 * truncation (Scene.h:321-371, :648-662, :688-710); out holds out_w * out_h * 3 bytes. */
int crt_image_decode(const uint8_t* file_bytes, size_t n_bytes, int32_t* width, int32_t* height, uint8_t* rgb, size_t rgb_capacity);
/* Image file of a resolved frame [host] (the step after the path; the reference only shows the texture on
 * screen, Scene.h:1224-1230).  crt_image_encode_png: PNG (8-bit, colour type 2 or 6) of `height` rows of `width` pixels,
 * `channels` = 3 or 4 bytes each; bottom_up != 0: the first row in memory is the bottom row (crt_resolve's orientation).
 * Call with file = NULL to get the size an upper bound needs; *file_size returns the bytes written. */
int crt_image_encode_png(const uint8_t* pixels, int32_t width, int32_t height, int32_t channels, int32_t bottom_up,
                         uint8_t* file, size_t file_capacity, size_t* file_size);
int crt_texture_to_array_bytes(const uint8_t* rgb, int32_t width, int32_t height, int32_t out_w, int32_t out_h, uint8_t* out);

const char* crt_last_error(void);
uint32_t    crt_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* CRT_H_ */
