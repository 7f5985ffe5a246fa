// Instanced scenes (include/crt.h crt_instances_*): one bottom-level CWBVH per mesh, built once on the device by the
// scene builders (lbvh.hip, cwbvh_device.hip, scene_build.hip), and a top-level CWBVH over the instances' world boxes, rebuilt on the
// device (binned SAH over boxes, then the same converter) at create and at every set, or refitted in place by crt_instances_refit
// (DESIGN.md §13).  All node8s live in ONE array (the TLAS region first,
// sized for `capacity`, then every BLAS with its child / triangle bases rebased) and all triangle records in ONE array, so the walk
// (instances.hip k_trace_instances) addresses any node with one 32-bit index off one base.  crt_instances_add_meshes and
// crt_instances_replace_meshes change the mesh list of a live handle: new arrays in the same layout, swapped in last.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/crt.h"
#include "crt_error.hpp"
#include "device_build.hpp"
#include "host/instance_math.hpp"
#include "host/light_math.hpp"
#include "host/refit_core.hpp"
#include "instances.hpp"
#include "instances_bind.hpp"
#include "rt_kernels.hpp"

using crt::dev_alloc;
using crt::fail;
using crt::gpu_flags_of;
using crt::require_device;

#define IHIPCHK(expr)                                                                            \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return fail(CRT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));         \
    } while (0)

static_assert(sizeof(crt_instance) == 64, "crt_instance is 64 bytes");

// What crt_instances_update_meshes keeps (CRT_INSTANCES_UPDATABLE handles only).  Nothing here is read by the walk.
struct InstUpdateState {
    std::vector<uint32_t> nv, nt, tri_off;            // per mesh: vertices, triangles, first triangle in the index / record arrays
    std::vector<uint64_t> v_off;                      // per mesh: first vertex of its host-form staging
    std::vector<std::vector<uint32_t>> level;         // per mesh, per level (+ end): position in d_order of the level's first node8
    std::vector<float> mesh_box;                      // host copy of d_mesh_box
    std::vector<float> box_stage;                     // the staged mesh boxes of the call in progress
    std::vector<uint8_t> table;                       // the call's tables (RefitMesh, chunk starts, segments), uploaded at once
    uint32_t max_levels = 0;
    uint32_t* d_order = nullptr;                      // every BLAS node8 (global index), per mesh, level by level from the root
    float* d_box8 = nullptr;                          // 6 floats per BLAS node8: its float box, which its parent's slot reads
    int32_t* d_src_idx = nullptr;                     // 3 vertex indices per triangle, source order, mesh after mesh
    uint32_t* d_live = nullptr;                       // the last accepted crt_instance array (capacity x 64 B)
    float* d_mesh_box_stage = nullptr;                // 6 floats per mesh
    float* d_vstage = nullptr;                        // the host form's positions, every mesh
    uint32_t* d_check = nullptr;                      // 8 words per mesh of a call
    uint32_t* h_check = nullptr;                      // pinned
    uint8_t* d_table = nullptr;
    size_t table_cap = 0;
    uint64_t bytes = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool have_times = false;
    float device_ms = 0.f, wall_ms = 0.f;

    ~InstUpdateState() {
        void* bufs[] = {d_order, d_box8, d_src_idx, d_live, d_mesh_box_stage, d_vstage, d_check, d_table};
        for (void* p : bufs) if (p) (void)hipFree(p);
        if (h_check) (void)hipHostFree(h_check);
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
    }
};

// what a repack needs to know of a packed BLAS (crt_instances_add_meshes / crt_instances_replace_meshes)
struct MeshSlot { uint32_t n8 = 0, n_tris = 0, depth8 = 0; };

struct crt_instances {
    int device = 0;
    hipStream_t stream = nullptr;
    uint32_t n_meshes = 0, capacity = 0, n_instances = 0;
    uint32_t gpu_flags = 0;               // the builder given at create: added and replaced meshes are built with it
    std::vector<MeshSlot> mesh;           // per mesh, in the order of the packed arrays
    uint32_t tlas_cap_nodes = 0, n_tlas8 = 0, tlas_depth8 = 0, max_blas_depth8 = 0, stack_entries = 2;
    uint64_t blas_nodes8 = 0, blas_tris = 0;
    uint4* d_nodes = nullptr;             // TLAS region (tlas_cap_nodes) + every BLAS
    float4* d_tris = nullptr;             // every BLAS's records
    float4* d_inst = nullptr;             // live instance records in TLAS leaf order (capacity x 4 rows)
    float* d_w2o = nullptr;               // live world_to_object, instance order (capacity x 12)
    float* d_wbox = nullptr;              // live world boxes, instance order (capacity x 6)
    uint2* d_mesh_of = nullptr;           // live, instance order: (mesh index, bit 31 = identity matrix; material offset): what a bound scene's shading reads
    float* d_mesh_box = nullptr;          // 6 per mesh
    uint32_t* d_mesh_root = nullptr;      // BLAS root node per mesh
    // a set's staging: nothing here is read by the walk, so a refused set leaves the scene as it was
    uint32_t* d_in = nullptr;             // host-given instances (capacity x 16 words)
    float4* d_rec = nullptr;              // records in instance order
    float* d_box = nullptr;
    float* d_w2o_stage = nullptr;
    uint2* d_mesh_of_stage = nullptr;
    // object_to_world as the last successful set / refit gave it (debug read 7), staged by the prep like world_to_object: d_in belongs to
    // the last ATTEMPTED call.  Ray queries never read it; the light tables of bound scenes do
    float* d_o2w = nullptr;
    float* d_o2w_stage = nullptr;
    uint64_t mutations = 0;               // successful publishes, refits and mesh updates so far: what a bound scene's light table is dated by
    crt_node8* d_t8_stage = nullptr;      // the converter's output (tlas_cap_nodes)
    uint32_t* d_flag = nullptr;           // the verdict of a call's device checks: [0] what failed, [1] the first instance a bound scene refuses
    uint32_t* d_overflow = nullptr;
    crt::DeviceArena arena;               // TLAS build: BVH2, leaf order, CWBVH slots, builder temporaries (sized for capacity)
    crt_flatnode* d_flat = nullptr;
    uint32_t* d_tri_order = nullptr;
    int32_t* d_tri_slots = nullptr;
    size_t arena_mark = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    float set_device_ms = 0.f, set_wall_ms = 0.f, build_wall_ms = 0.f;
    // crt_instances_refit: the live TLAS as a refit mesh over d_box.  Its levels are found at the first refit after each
    // TLAS build; the rest is reserved at create, so that later refits allocate nothing
    bool tlas_levels_ok = false;
    std::vector<uint32_t> tlas_level;     // per level, root first (+ end): position in d_tlas_order of its first node8
    uint32_t* d_tlas_order = nullptr;     // the live TLAS's node8s level by level (discover_levels)
    float* d_tlas_box8 = nullptr;         // 6 floats per TLAS node8: its float box, which its parent's slot reads
    int32_t* d_box_idx = nullptr;         // (2i, 2i + 1, 2i) per instance: instance i's world box as a triangle of d_box
    uint8_t* d_tlas_table = nullptr;      // the TLAS's RefitMesh, then one RefitSeg per level
    std::vector<uint8_t> tlas_table;
    // masked traces: 8 B per TLAS node8, byte i = OR of the masks under meta slot i.  Stale after every publish and refit;
    // the next masked trace, debug read or masked frame of a bound scene recomputes them on the stream (ensure_child_masks), ALWAYS this
    // handle's: ev_cmask, recorded behind each pass, is what a bound scene's stream waits for.  Reserved at create
    bool cmask_ok = false;
    uint64_t cmask_gen = 0;               // passes enqueued so far
    hipEvent_t ev_cmask = nullptr;
    uint2* d_cmask = nullptr;             // tlas_cap_nodes x 8 B
    uint32_t* d_cm_parent = nullptr;      // tlas_cap_nodes: (parent node << 3 | meta slot) of each TLAS node8
    uint32_t* d_cm_leaf = nullptr;        // capacity: (node << 3 | meta slot) of the leaf slot holding each instance record
    // crt_instances_trace's device copies of the host rays
    void* d_t_rays = nullptr; void* d_t_hits = nullptr; void* d_t_inst = nullptr; void* d_t_stats = nullptr;
    size_t t_cap = 0;
    std::unique_ptr<InstUpdateState> upd;     // CRT_INSTANCES_UPDATABLE only
    // scenes that render this handle (crt_scene_create_instanced), by their streams: while there is one, every mutator
    // first waits for them (wait_bound), and destroy / add_meshes / replace_meshes are refused
    struct Bound { hipStream_t stream; crt::InstOffsetRule rule; };
    std::vector<Bound> bound;

    ~crt_instances() {
        void* bufs[] = {d_nodes, d_tris, d_inst, d_w2o, d_wbox, d_mesh_box, d_mesh_root, d_in, d_rec, d_box, d_w2o_stage, d_flag, d_overflow,
                        d_t8_stage, d_t_rays, d_t_hits, d_t_inst, d_t_stats, d_tlas_order, d_tlas_box8, d_box_idx, d_tlas_table, d_cmask, d_cm_parent,
                        d_cm_leaf, d_mesh_of, d_mesh_of_stage, d_o2w, d_o2w_stage};
        if (stream) (void)hipStreamSynchronize(stream);
        upd.reset();
        for (void* p : bufs) if (p) (void)hipFree(p);
        arena.release();
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (ev_cmask) (void)hipEventDestroy(ev_cmask);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace {

// One mesh: LBVH / PLOC / SAH BVH2 -> CWBVH -> records, as crt_scene_create's build-on-device path.  *d_nodes8 and *d_recs are the
// caller's to free.
int build_blas(const crt_blas_desc& m, uint32_t gpu_flags, hipStream_t st, const std::string& who, crt_node8** d_nodes8, float4** d_recs, uint32_t* n8,
               uint32_t* depth8) {
    const uint32_t n = (uint32_t)m.n_triangles, n2 = 2u * n - 1u;
    crt::DeviceArena arena;                       // the mesh's vertices, triangles and BVH2 too: one allocation per BLAS
    auto P = crt::DeviceArena::padded;
    hipError_t he = arena.reserve(P(m.n_vertices * 12) + P((size_t)n * sizeof(crt_triangle)) + P((size_t)n2 * sizeof(crt_flatnode)) +
                                  crt::device_tree_tmp_bytes(n, gpu_flags));
    if (he != hipSuccess) return fail(CRT_ERR_NOMEM, who + "hipMalloc: " + hipGetErrorString(he));
    float* d_verts = arena.take<float>(m.n_vertices * 3);
    crt_triangle* d_in = arena.take<crt_triangle>(n);
    crt_flatnode* d_flat = arena.take<crt_flatnode>(n2);
    IHIPCHK(hipMemcpyAsync(d_verts, m.vertices, m.n_vertices * 12, hipMemcpyHostToDevice, st));
    IHIPCHK(hipMemcpyAsync(d_in, m.triangles, (size_t)n * sizeof(crt_triangle), hipMemcpyHostToDevice, st));
    crt::DeviceTree tree;
    const int rc = crt::build_device_tree(d_in, d_verts, n, gpu_flags, arena, d_flat, crt::kBlasTree, st, who, &tree);
    if (rc) return rc;
    IHIPCHK(hipStreamSynchronize(st));                // before the arena goes
    IHIPCHK(hipGetLastError());
    *d_nodes8 = reinterpret_cast<crt_node8*>(tree.nodes); *d_recs = tree.tris; *n8 = tree.n8; *depth8 = tree.depth8;
    tree.nodes = nullptr; tree.tris = nullptr;
    return CRT_OK;
}

// The TLAS of n instances (crt_instance array in DEVICE memory) into staging: the prep kernel (the host waits once for its verdict) against
// the mesh boxes d_mesh_box, the SAH build over the world boxes, the converter into the node staging buffer, the stack bound.  Nothing the
// walk reads changes here.  `who` prefixes the messages.
struct TlasStage {
    crt_instances* s = nullptr;
    crt_node8* d_t8 = nullptr;
    uint32_t n8 = 0, depth8 = 0, stack = 2;
    ~TlasStage() { if (s && d_t8 && d_t8 != s->d_t8_stage) (void)hipFree(d_t8); }
};

// n >= 1 instances (DEVICE memory) through the prep kernel against the mesh boxes d_mesh_box and BLAS roots d_mesh_root of n_meshes
// meshes (the live ones, or a call's staged ones), into the set's staging (d_rec, d_box, d_w2o_stage), and the host's one wait for its
// verdict.  Shared by sets, updates, refits and replaces; the walk reads none of it.
struct MeshTables { const float* d_box; const uint32_t* d_root; uint32_t n_meshes, max_depth8; };
MeshTables live_tables(const crt_instances* s) { return MeshTables{s->d_mesh_box, s->d_mesh_root, s->n_meshes, s->max_blas_depth8}; }

// Before a mutator enqueues anything: the frames a bound scene has queued (crt_render_frame*_async) have read the live arrays
int wait_bound(crt_instances* s) {
    for (const auto& b : s->bound) IHIPCHK(hipStreamSynchronize(b.stream));
    return CRT_OK;
}

// a bound scene's refusal of a material offset, from the verdict words
std::string offset_refusal(const uint32_t flag[2]) {
    return "instance " + std::to_string(flag[1]) +
           ((flag[0] & 8u) ? ": material_offset is 2^31 or more, or moves its mesh's greatest material index past a bound scene's material table"
                           : ": material_offset moves a mesh whose vt do not all index its texcoords onto a textured material of a bound scene");
}

// the rule of one bound scene against n (mesh, offset) words, into d_flag.  Enqueued only
void check_offsets(crt_instances* s, const crt::InstOffsetRule& rule, const uint2* d_words, uint32_t n, uint32_t n_meshes) {
    crt::InstOffsetCheckArgs ca{};
    ca.mesh_of = d_words; ca.n = n; ca.n_meshes = n_meshes; ca.rule = rule; ca.flag = s->d_flag;
    crt::launch_instance_offsets(ca, s->stream);
}

int prep_instances(crt_instances* s, const void* d_src, uint32_t n, const MeshTables& mt, const std::string& who) {
    hipStream_t st = s->stream;
    IHIPCHK(hipMemsetAsync(s->d_flag, 0, 4, st));
    IHIPCHK(hipMemsetAsync(s->d_flag + 1, 0xff, 4, st));
    crt::InstPrepArgs pa{};
    pa.in = static_cast<const uint32_t*>(d_src); pa.n = n; pa.n_meshes = mt.n_meshes; pa.mesh_box = mt.d_box; pa.mesh_root = mt.d_root;
    pa.rec = s->d_rec; pa.box = s->d_box; pa.w2o = s->d_w2o_stage; pa.flag = s->d_flag; pa.mesh_of = s->d_mesh_of_stage;
    pa.o2w = s->d_o2w_stage;
    crt::launch_instance_prep(pa, st);
    // every bound scene's rule for material offsets against the STAGED words, into the same verdict: still one wait
    for (const auto& b : s->bound) check_offsets(s, b.rule, s->d_mesh_of_stage, n, mt.n_meshes);
    uint32_t flag[2] = {0u, 0u};
    IHIPCHK(hipMemcpyAsync(flag, s->d_flag, 8, hipMemcpyDeviceToHost, st));
    IHIPCHK(hipStreamSynchronize(st));
    IHIPCHK(hipGetLastError());
    if (flag[0] & 7u)
        return fail(CRT_ERR_INVALID, who + ((flag[0] & 1u) ? "a matrix is not finite, or singular, or its inverse is not finite"
                                            : (flag[0] & 2u) ? "a mesh index is out of range" : "a world box exceeds 1e18"));
    if (flag[0]) return fail(CRT_ERR_INVALID, who + offset_refusal(flag));
    return CRT_OK;
}

int stage_tlas(crt_instances* s, const void* d_src, uint32_t n, const MeshTables& mt, const std::string& who, TlasStage& ts) {
    hipStream_t st = s->stream;
    ts.s = s;
    int rc = prep_instances(s, d_src, n, mt, who);
    if (rc) return rc;
    // the TLAS over the world boxes
    s->arena.used = s->arena_mark;
    float ms = 0.f;
    if (n == 1) {
        crt::launch_single_leaf(s->d_box, s->d_flat, s->d_tri_order, st);
    } else {
        uint32_t depth2 = 0;
        rc = crt::sah_build_from_boxes_on_device(s->d_box, n, CRT_GPU_BUILD_SAH, s->arena, s->d_flat, s->d_tri_order, &depth2, &ms, st);
        if (rc) return fail(rc, who + "TLAS build failed: " + crt_last_error());
        s->arena.used = s->arena_mark;
    }
    // into the staging node buffer sized for `capacity` at create: no allocation (and no device-wide hipFree) per set
    rc = crt::cwbvh_convert_on_device(s->d_flat, n == 1 ? 1u : 2u * n - 1u, n, s->arena, s->d_tri_slots, &ts.d_t8, nullptr, &ts.n8, &ts.depth8, &ms, st,
                                      s->d_t8_stage, s->tlas_cap_nodes);
    if (rc) return fail(rc, who + "TLAS BVH2 -> CWBVH failed: " + crt_last_error());
    ts.stack = std::max<uint32_t>(2u, ts.depth8 + mt.max_depth8);
    if (ts.stack > CRT_INST_STACK_ENTRIES)
        return fail(CRT_ERR_LIMIT, who + "TLAS depth + deepest BLAS exceed the walk's stack (" + std::to_string(ts.stack) + " > " +
                                       std::to_string(CRT_INST_STACK_ENTRIES) + " entries)");
    if (ts.n8 > s->tlas_cap_nodes) return fail(CRT_ERR_HIP, who + "TLAS larger than its region");
    return CRT_OK;
}

// everything checked: publish the staged TLAS (it starts at node 0, its leaves index the instance records: no rebase), records, matrices
// and boxes; an updatable handle keeps the instances themselves (d_src, when it is not that copy already) for its updates.  Enqueued only.
int publish_tlas(crt_instances* s, const void* d_src, uint32_t n, const TlasStage& ts) {
    hipStream_t st = s->stream;
    s->tlas_levels_ok = false;                    // a new topology: the next refit finds its levels
    s->cmask_ok = false;
    IHIPCHK(hipMemcpyAsync(s->d_nodes, ts.d_t8, (size_t)ts.n8 * sizeof(crt_node8), hipMemcpyDeviceToDevice, st));
    crt::launch_gather_instances(s->d_rec, s->d_tri_order, s->d_tri_slots, n, s->d_inst, st);
    IHIPCHK(hipMemcpyAsync(s->d_w2o, s->d_w2o_stage, (size_t)n * 48, hipMemcpyDeviceToDevice, st));
    IHIPCHK(hipMemcpyAsync(s->d_wbox, s->d_box, (size_t)n * 24, hipMemcpyDeviceToDevice, st));
    IHIPCHK(hipMemcpyAsync(s->d_mesh_of, s->d_mesh_of_stage, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
    IHIPCHK(hipMemcpyAsync(s->d_o2w, s->d_o2w_stage, (size_t)n * 48, hipMemcpyDeviceToDevice, st));
    if (s->upd && d_src != s->upd->d_live)
        IHIPCHK(hipMemcpyAsync(s->upd->d_live, d_src, (size_t)n * sizeof(crt_instance), hipMemcpyDeviceToDevice, st));
    return CRT_OK;
}

// Validate + prepare n instances from DEVICE memory, then rebuild the TLAS.  Nothing the walk reads changes before every check passed.
int set_impl(crt_instances* s, const void* d_src, uint32_t n) {
    const auto t0 = std::chrono::steady_clock::now();
    if (n > s->capacity) return fail(CRT_ERR_INVALID, "crt_instances_set: more instances than the capacity given at create");
    hipStream_t st = s->stream;
    { const int wrc = wait_bound(s); if (wrc) return wrc; }
    IHIPCHK(hipEventRecord(s->ev0, st));
    if (n > 0) {
        TlasStage ts;
        int rc = stage_tlas(s, d_src, n, live_tables(s), "crt_instances_set: ", ts);
        if (rc) return rc;
        if ((rc = publish_tlas(s, d_src, n, ts))) return rc;
        IHIPCHK(hipStreamSynchronize(st));            // the publication is done when the call returns
        s->n_tlas8 = ts.n8; s->tlas_depth8 = ts.depth8; s->stack_entries = ts.stack;
    } else {
        s->n_tlas8 = 0; s->tlas_depth8 = 0; s->stack_entries = 2;
    }
    s->n_instances = n;
    ++s->mutations;
    IHIPCHK(hipEventRecord(s->ev1, st));
    IHIPCHK(hipGetLastError());
    IHIPCHK(hipEventSynchronize(s->ev1));
    IHIPCHK(hipEventElapsedTime(&s->set_device_ms, s->ev0, s->ev1));
    s->set_wall_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return CRT_OK;
}

// The levels of the live TLAS (n_instances >= 1), once per TLAS build, and its refit tables: the TLAS is a RefitMesh over the staged
// world boxes (2 vertices per instance, the triples of d_box_idx) whose records, the instance records, name their instance in row 3 .y.
int find_tlas_levels(crt_instances* s) {
    hipStream_t st = s->stream;
    if (s->d_tlas_order) { (void)hipFree(s->d_tlas_order); s->d_tlas_order = nullptr; }
    const crt::RefitTree tree{s->d_nodes, false, 5u, s->n_tlas8, 0u};
    std::vector<std::vector<uint32_t>> level;
    int rc = crt::discover_levels(&tree, 1, st, &s->d_tlas_order, level);
    if (rc) return rc;
    if (level[0].size() - 1 > 255) return fail(CRT_ERR_HIP, "crt_instances_refit: TLAS deeper than 255 levels");
    s->tlas_level = level[0];
    const uint32_t n = s->n_instances, levels = (uint32_t)s->tlas_level.size() - 1u;
    s->tlas_table.assign(sizeof(crt::RefitMesh) + levels * sizeof(crt::RefitSeg), 0);
    *reinterpret_cast<crt::RefitMesh*>(s->tlas_table.data()) = crt::RefitMesh{s->d_box, s->d_box_idx, 3u, n, 13u, 2u * n};
    auto* seg = reinterpret_cast<crt::RefitSeg*>(s->tlas_table.data() + sizeof(crt::RefitMesh));
    for (uint32_t L = 0; L < levels; ++L) seg[L] = crt::RefitSeg{0u, s->tlas_level[L], 0u, 0u};
    IHIPCHK(hipMemcpyAsync(s->d_tlas_table, s->tlas_table.data(), s->tlas_table.size(), hipMemcpyHostToDevice, st));
    s->tlas_levels_ok = true;
    return CRT_OK;
}

// Same instances, new transforms: the prep into staging (the one wait for a verdict), then the live TLAS refitted in place
// deepest level first, each leaf slot's record renewed from the instance it holds, and the matrices and boxes published.  Reads nothing of
// the last attempted build (d_flat, d_tri_order, d_tri_slots, d_t8_stage): a set refused with CRT_ERR_LIMIT has rebuilt them, while the
// live TLAS is the one before it.
int refit_impl(crt_instances* s, const void* d_src, uint32_t n, const std::string& who) {
    const auto t0 = std::chrono::steady_clock::now();
    if (n != s->n_instances)
        return fail(CRT_ERR_INVALID, who + "n_instances (" + std::to_string(n) + ") differs from the live count (" + std::to_string(s->n_instances) + ")");
    hipStream_t st = s->stream;
    { const int wrc = wait_bound(s); if (wrc) return wrc; }
    IHIPCHK(hipEventRecord(s->ev0, st));
    if (n > 0) {
        int rc = prep_instances(s, d_src, n, live_tables(s), who);
        if (rc) return rc;
        if (!s->tlas_levels_ok && (rc = find_tlas_levels(s))) return rc;
        const auto* d_mesh = reinterpret_cast<const crt::RefitMesh*>(s->d_tlas_table);
        const auto* d_seg = reinterpret_cast<const crt::RefitSeg*>(s->d_tlas_table + sizeof(crt::RefitMesh));
        const std::vector<uint32_t>& lv = s->tlas_level;
        for (size_t L = lv.size() - 1; L-- > 0;)
            crt::launch_refit_node8_level(s->d_nodes, 5u, 0u, s->n_tlas8, s->d_tlas_order, d_seg + L, 1u, lv[L + 1] - lv[L], s->d_inst, 4u, n, d_mesh,
                                          s->d_tlas_box8, st);
        crt::launch_regather_instances(s->d_rec, n, s->d_inst, st);
        s->cmask_ok = false;                      // the records may carry new masks
        IHIPCHK(hipGetLastError());
        IHIPCHK(hipMemcpyAsync(s->d_w2o, s->d_w2o_stage, (size_t)n * 48, hipMemcpyDeviceToDevice, st));
        IHIPCHK(hipMemcpyAsync(s->d_wbox, s->d_box, (size_t)n * 24, hipMemcpyDeviceToDevice, st));
        IHIPCHK(hipMemcpyAsync(s->d_mesh_of, s->d_mesh_of_stage, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
        IHIPCHK(hipMemcpyAsync(s->d_o2w, s->d_o2w_stage, (size_t)n * 48, hipMemcpyDeviceToDevice, st));
        if (s->upd && d_src != s->upd->d_live)
            IHIPCHK(hipMemcpyAsync(s->upd->d_live, d_src, (size_t)n * sizeof(crt_instance), hipMemcpyDeviceToDevice, st));
    }
    IHIPCHK(hipEventRecord(s->ev1, st));
    IHIPCHK(hipEventSynchronize(s->ev1));             // the publication is done when the call returns
    IHIPCHK(hipGetLastError());
    ++s->mutations;
    IHIPCHK(hipEventElapsedTime(&s->set_device_ms, s->ev0, s->ev1));
    s->set_wall_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return CRT_OK;
}

// The TLAS child masks of the live TLAS and records, if stale: two launches on the handle's stream, ordered before whatever the caller
// enqueues next there (the masked walk, a debug read).  No host wait, no allocation.
int ensure_child_masks(crt_instances* s) {
    if (s->cmask_ok) return CRT_OK;
    if (s->n_instances)
        crt::launch_tlas_child_masks(s->d_nodes, s->n_tlas8, s->d_inst, s->n_instances, s->d_cm_parent, s->d_cm_leaf, s->d_cmask, s->stream);
    IHIPCHK(hipGetLastError());
    IHIPCHK(hipEventRecord(s->ev_cmask, s->stream));
    ++s->cmask_gen;
    s->cmask_ok = true;
    return CRT_OK;
}

// CRT_INSTANCES_UPDATABLE: the refit state, once at create.  Level discovery runs on each BLAS as built (bases not rebased yet); the order
// holds global node indices.
int init_update_state(crt_instances* s, const crt_blas_desc* meshes, const std::vector<crt_node8*>& blas_nodes, const std::vector<uint32_t>& blas_n8,
                      const std::vector<uint32_t>& roots, const std::vector<float>& mesh_box) {
    std::unique_ptr<InstUpdateState> u(new (std::nothrow) InstUpdateState);
    if (!u) return fail(CRT_ERR_NOMEM, "crt_instances_create: out of memory");
    hipStream_t st = s->stream;
    const uint32_t M = s->n_meshes;
    const uint64_t n8_all = s->blas_nodes8, tris_all = s->blas_tris;
    u->nv.resize(M); u->nt.resize(M); u->tri_off.resize(M); u->v_off.resize(M);
    u->mesh_box = mesh_box;
    uint64_t v_total = 0, t_off = 0;
    std::vector<int32_t> idx(3 * tris_all);
    for (uint32_t k = 0; k < M; ++k) {
        u->nv[k] = (uint32_t)meshes[k].n_vertices; u->nt[k] = (uint32_t)meshes[k].n_triangles; u->tri_off[k] = (uint32_t)t_off;
        u->v_off[k] = v_total;
        for (size_t i = 0; i < meshes[k].n_triangles; ++i)
            for (int j = 0; j < 3; ++j) idx[3 * (t_off + i) + j] = meshes[k].triangles[i].v[j];
        v_total += meshes[k].n_vertices; t_off += meshes[k].n_triangles;
    }
    if (v_total >= (1ull << 32) / 12) return fail(CRT_ERR_LIMIT, "crt_instances_create: more vertices than an updatable handle stages");
    int rc;
    if ((rc = dev_alloc(&u->d_src_idx, idx.size())) || (rc = dev_alloc(&u->d_box8, 6 * n8_all)) ||
        (rc = dev_alloc(&u->d_live, 16 * (size_t)s->capacity)) || (rc = dev_alloc(&u->d_mesh_box_stage, 6 * (size_t)M)) ||
        (rc = dev_alloc(&u->d_vstage, 3 * v_total)) || (rc = dev_alloc(&u->d_check, 8 * (size_t)M)))
        return rc;
    IHIPCHK(hipHostMalloc(reinterpret_cast<void**>(&u->h_check), 8 * (size_t)M * sizeof(uint32_t)));
    IHIPCHK(hipEventCreate(&u->ev0));
    IHIPCHK(hipEventCreate(&u->ev1));
    IHIPCHK(hipMemcpyAsync(u->d_src_idx, idx.data(), idx.size() * 4, hipMemcpyHostToDevice, st));
    IHIPCHK(hipMemsetAsync(u->d_box8, 0, 24 * n8_all, st));
    std::vector<crt::RefitTree> trees(M);
    for (uint32_t k = 0; k < M; ++k) trees[k] = crt::RefitTree{blas_nodes[k], false, 5u, blas_n8[k], roots[k]};
    if ((rc = crt::discover_levels(trees.data(), M, st, &u->d_order, u->level))) return rc;
    for (const auto& l : u->level) u->max_levels = std::max(u->max_levels, (uint32_t)l.size() - 1u);
    // the call's tables: RefitMesh, chunk starts and record segments per mesh, level segments per mesh and level
    auto A = [](size_t b) { return (b + 15) & ~size_t(15); };
    u->table_cap = A(M * sizeof(crt::RefitMesh)) + A(M * 4) + A(M * sizeof(crt::RefitSeg)) + (size_t)M * u->max_levels * sizeof(crt::RefitSeg);
    if ((rc = dev_alloc(&u->d_table, u->table_cap))) return rc;
    IHIPCHK(hipStreamSynchronize(st));            // before the host arrays go
    u->bytes = 4 * n8_all + 24 * n8_all + 12 * tris_all + 64 * (uint64_t)s->capacity + 24 * (uint64_t)M + 12 * v_total + 32 * (uint64_t)M +
               u->table_cap;
    s->upd = std::move(u);
    return CRT_OK;
}

// New positions for n distinct meshes (h_verts: host arrays, or d_verts: device arrays).  Order: check + mesh boxes on the
// device (one host wait), the prep of the live instances and the TLAS into staging against the staged mesh boxes, and only then the BLAS
// refit in place and the publication.  A refused call has written nothing the walk reads.
int update_impl(crt_instances* s, const uint32_t* ids, uint32_t n, const float* const* h_verts, const void* const* d_verts, const size_t* n_vertices,
                const std::string& who) {
    const auto t0 = std::chrono::steady_clock::now();
    if (!s) return fail(CRT_ERR_INVALID, who + "null handle");
    InstUpdateState* u = s->upd.get();
    if (!u) return fail(CRT_ERR_INVALID, who + "the handle was created without CRT_INSTANCES_UPDATABLE");
    if (n && (!ids || !n_vertices || (!h_verts && !d_verts))) return fail(CRT_ERR_INVALID, who + "null argument");
    if (n > s->n_meshes) return fail(CRT_ERR_INVALID, who + "more meshes than the handle holds");
    std::vector<char> seen(s->n_meshes, 0);
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t m = ids[k];
        if (m >= s->n_meshes) return fail(CRT_ERR_INVALID, who + "mesh index " + std::to_string(m) + " is out of range");
        if (seen[m]) return fail(CRT_ERR_INVALID, who + "mesh index " + std::to_string(m) + " is repeated");
        seen[m] = 1;
        if (h_verts ? !h_verts[k] : !d_verts[k]) return fail(CRT_ERR_INVALID, who + "null vertices");
        if (n_vertices[k] != u->nv[m]) return fail(CRT_ERR_INVALID, who + "n_vertices of mesh " + std::to_string(m) + " differs from the count given at create");
    }
    if (n == 0) return CRT_OK;
    IHIPCHK(hipSetDevice(s->device));
    hipStream_t st = s->stream;
    { const int wrc = wait_bound(s); if (wrc) return wrc; }
    // the call's tables
    auto A = [](size_t b) { return (b + 15) & ~size_t(15); };
    const size_t o_chunk = A(n * sizeof(crt::RefitMesh)), o_rseg = o_chunk + A(n * 4), o_lseg = o_rseg + A(n * sizeof(crt::RefitSeg));
    u->table.assign(o_lseg + (size_t)n * u->max_levels * sizeof(crt::RefitSeg), 0);
    auto* tm = reinterpret_cast<crt::RefitMesh*>(u->table.data());
    auto* tc = reinterpret_cast<uint32_t*>(u->table.data() + o_chunk);
    auto* tr = reinterpret_cast<crt::RefitSeg*>(u->table.data() + o_rseg);
    auto* tl = reinterpret_cast<crt::RefitSeg*>(u->table.data() + o_lseg);
    uint32_t chunks = 0, recs = 0, levels = 0;
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t m = ids[k];
        const float* v = nullptr;
        if (h_verts) {
            float* dst = u->d_vstage + 3 * u->v_off[m];
            IHIPCHK(hipMemcpyAsync(dst, h_verts[k], (size_t)u->nv[m] * 12, hipMemcpyHostToDevice, st));
            v = dst;
        } else {
            v = static_cast<const float*>(d_verts[k]);
        }
        // a BLAS as a refit mesh: its slice of the source-order index array, keyed by the source id in v0.w
        tm[k] = crt::RefitMesh{v, u->d_src_idx + 3 * (size_t)u->tri_off[m], 3u, u->nt[m], 3u, u->nv[m]};
        tc[k] = chunks;
        chunks += (std::max(u->nv[m], u->nt[m]) + crt::kCheckChunk - 1) / crt::kCheckChunk;
        tr[k] = crt::RefitSeg{recs, u->tri_off[m], k, 0u};
        recs += u->nt[m];
        levels = std::max(levels, (uint32_t)u->level[m].size() - 1u);
    }
    // level L: a segment per mesh that reaches it
    std::vector<uint32_t> lseg_at(levels + 1, 0), lcount(levels, 0);
    uint32_t n_lseg = 0;
    for (uint32_t L = 0; L < levels; ++L) {
        lseg_at[L] = n_lseg;
        for (uint32_t k = 0; k < n; ++k) {
            const uint32_t m = ids[k];
            const std::vector<uint32_t>& lm = u->level[m];
            if (lm.size() <= L + 1u) continue;
            tl[n_lseg++] = crt::RefitSeg{lcount[L], lm[L], k, 0u};
            lcount[L] += lm[L + 1] - lm[L];
        }
    }
    lseg_at[levels] = n_lseg;
    IHIPCHK(hipMemcpyAsync(u->d_table, u->table.data(), u->table.size(), hipMemcpyHostToDevice, st));
    const auto* d_tm = reinterpret_cast<const crt::RefitMesh*>(u->d_table);
    const auto* d_tc = reinterpret_cast<const uint32_t*>(u->d_table + o_chunk);
    const auto* d_tr = reinterpret_cast<const crt::RefitSeg*>(u->d_table + o_rseg);
    const auto* d_tl = reinterpret_cast<const crt::RefitSeg*>(u->d_table + o_lseg);

    // 1. the coordinates and the new mesh boxes: the one wait for a verdict before the TLAS build
    IHIPCHK(hipEventRecord(u->ev0, st));
    IHIPCHK(hipMemsetAsync(u->d_check, 0, (size_t)n * 32, st));
    crt::launch_check_meshes(d_tm, d_tc, n, chunks, u->d_check, st);
    IHIPCHK(hipMemcpyAsync(u->h_check, u->d_check, (size_t)n * 32, hipMemcpyDeviceToHost, st));
    IHIPCHK(hipStreamSynchronize(st));
    IHIPCHK(hipGetLastError());
    u->box_stage = u->mesh_box;
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t* c = u->h_check + 8 * (size_t)k;
        if (c[0]) return fail(CRT_ERR_INVALID, who + "a vertex coordinate of mesh " + std::to_string(ids[k]) + " is not finite or exceeds 1e18");
        for (int a = 0; a < 3; ++a) {
            u->box_stage[6 * (size_t)ids[k] + a] = crt::rf::key_to_float(~c[4 + a]);
            u->box_stage[6 * (size_t)ids[k] + 3 + a] = crt::rf::key_to_float(c[1 + a]);
        }
    }
    IHIPCHK(hipMemcpyAsync(u->d_mesh_box_stage, u->box_stage.data(), u->box_stage.size() * 4, hipMemcpyHostToDevice, st));
    // 2. + 3. the live instances against the staged boxes, and their TLAS, into staging
    const uint32_t ni = s->n_instances;
    TlasStage ts;
    if (ni > 0) {
        MeshTables mt = live_tables(s);
        mt.d_box = u->d_mesh_box_stage;
        const int rc = stage_tlas(s, u->d_live, ni, mt, who, ts);
        if (rc) return rc;
    }
    // 4. the BLAS refit in place (records first: the leaf slots read only their id words), then the publication
    crt::launch_refit_records(s->d_tris, 3u, (uint32_t)s->blas_tris, d_tr, n, recs, d_tm, st);
    const uint32_t n_nodes = s->tlas_cap_nodes + (uint32_t)s->blas_nodes8;
    for (uint32_t L = levels; L-- > 0;)
        crt::launch_refit_node8_level(s->d_nodes, 5u, s->tlas_cap_nodes, n_nodes, u->d_order, d_tl + lseg_at[L], lseg_at[L + 1] - lseg_at[L], lcount[L],
                                      s->d_tris, 3u, (uint32_t)s->blas_tris, d_tm, u->d_box8, st);
    if (hipGetLastError() != hipSuccess) return fail(CRT_ERR_HIP, who + "refit launch failed");
    if (ni > 0) {
        const int rc = publish_tlas(s, u->d_live, ni, ts);
        if (rc) return rc;
    }
    IHIPCHK(hipMemcpyAsync(s->d_mesh_box, u->d_mesh_box_stage, u->box_stage.size() * 4, hipMemcpyDeviceToDevice, st));
    IHIPCHK(hipEventRecord(u->ev1, st));
    IHIPCHK(hipStreamSynchronize(st));
    IHIPCHK(hipGetLastError());
    if (ni > 0) { s->n_tlas8 = ts.n8; s->tlas_depth8 = ts.depth8; s->stack_entries = ts.stack; }
    u->mesh_box.swap(u->box_stage);
    ++s->mutations;
    IHIPCHK(hipEventElapsedTime(&u->device_ms, u->ev0, u->ev1));
    u->wall_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    u->have_times = true;
    return CRT_OK;
}

// One mesh of a create, add or replace, checked on the host before any device work; box: the exact float box of its referenced vertices.
int validate_mesh(const crt_blas_desc& m, uint32_t k, const std::string& who, float* box) {
    if (!m.vertices || !m.triangles || m.n_vertices == 0 || m.n_triangles == 0) return fail(CRT_ERR_INVALID, who + "mesh " + std::to_string(k) + " is empty");
    if (2ull * m.n_triangles >= (1ull << 29)) return fail(CRT_ERR_LIMIT, who + "a mesh has 2^28 triangles or more");
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (size_t i = 0; i < m.n_triangles; ++i)
        for (int j = 0; j < 3; ++j) {
            const int32_t vi = m.triangles[i].v[j];
            if (vi < 0 || (size_t)vi >= m.n_vertices) return fail(CRT_ERR_INVALID, who + "vertex index out of range");
            for (int a = 0; a < 3; ++a) {
                const float x = m.vertices[3 * (size_t)vi + a];
                if (!(std::fabs(x) <= 1e18f)) return fail(CRT_ERR_INVALID, who + "a vertex coordinate is not finite or exceeds 1e18");
                lo[a] = std::min(lo[a], x); hi[a] = std::max(hi[a], x);
            }
        }
    for (int a = 0; a < 3; ++a) { box[a] = lo[a]; box[3 + a] = hi[a]; }
    return CRT_OK;
}

int create_impl(const crt_blas_desc* meshes, uint32_t n_meshes, const crt_instance* instances, uint32_t n_instances, uint32_t capacity,
                uint32_t build_flags, crt_instances** out) {
    const auto t0 = std::chrono::steady_clock::now();
    if (!out) return fail(CRT_ERR_INVALID, "crt_instances_create: null out");
    *out = nullptr;
    if (!meshes || n_meshes == 0) return fail(CRT_ERR_INVALID, "crt_instances_create: no mesh");
    if (n_instances && !instances) return fail(CRT_ERR_INVALID, "crt_instances_create: null instances");
    if (capacity == 0) capacity = n_instances;
    if (capacity < n_instances) return fail(CRT_ERR_INVALID, "crt_instances_create: capacity below n_instances");
    if (capacity > (1u << 24)) return fail(CRT_ERR_LIMIT, "crt_instances_create: capacity above 2^24 instances");
    std::vector<float> mesh_box(6 * (size_t)n_meshes);
    uint64_t tris_total = 0;
    for (uint32_t k = 0; k < n_meshes; ++k) {
        int rc = validate_mesh(meshes[k], k, "crt_instances_create: ", &mesh_box[6 * (size_t)k]);
        if (rc) return rc;
        tris_total += meshes[k].n_triangles;
    }
    int rc = require_device();
    if (rc) return rc;
    std::unique_ptr<crt_instances> owner(new (std::nothrow) crt_instances);
    crt_instances* s = owner.get();
    if (!s) return fail(CRT_ERR_NOMEM, "crt_instances_create: out of memory");
    IHIPCHK(hipGetDevice(&s->device));
    IHIPCHK(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
    IHIPCHK(hipEventCreate(&s->ev0));
    IHIPCHK(hipEventCreate(&s->ev1));
    IHIPCHK(hipEventCreateWithFlags(&s->ev_cmask, hipEventDisableTiming));
    s->n_meshes = n_meshes; s->capacity = capacity;
    s->tlas_cap_nodes = std::max<uint32_t>(capacity, 1u);          // a CWBVH over c >= 1 leaves has at most max(1, c - 1) node8s
    hipStream_t st = s->stream;

    // every mesh once, then ONE node array (TLAS region first) and ONE record array
    struct Blas { crt_node8* nodes = nullptr; float4* recs = nullptr; uint32_t n8 = 0, depth8 = 0; };
    std::vector<Blas> blas(n_meshes);
    struct FreeAll { std::vector<Blas>& b; ~FreeAll() { for (auto& x : b) { if (x.nodes) (void)hipFree(x.nodes); if (x.recs) (void)hipFree(x.recs); } } } free_all{blas};
    const uint32_t gflags = s->gpu_flags = gpu_flags_of(build_flags);
    s->mesh.resize(n_meshes);
    uint64_t nodes_total = s->tlas_cap_nodes;
    for (uint32_t k = 0; k < n_meshes; ++k) {
        if ((rc = build_blas(meshes[k], gflags, st, "crt_instances_create: ", &blas[k].nodes, &blas[k].recs, &blas[k].n8, &blas[k].depth8))) return rc;
        s->mesh[k] = MeshSlot{blas[k].n8, (uint32_t)meshes[k].n_triangles, blas[k].depth8};
        nodes_total += blas[k].n8;
        s->max_blas_depth8 = std::max(s->max_blas_depth8, blas[k].depth8);
    }
    // one 32-bit byte offset per node / record fetch (rt_traverse.hpp node_rows / tri_rows)
    if (nodes_total * CRT_NODE_ROWS * 16 >= (1ull << 32) || tris_total * CRT_TRI_ROWS * 16 >= (1ull << 32))
        return fail(CRT_ERR_LIMIT, "crt_instances_create: the packed node or record array exceeds 4 GiB");
    if (CRT_NODE_ROWS != 5 || CRT_TRI_ROWS != 3) return fail(CRT_ERR_LIMIT, "crt_instances_create: needs the packed row strides (5 / 3)");
    if ((rc = dev_alloc(&s->d_nodes, nodes_total * 5))) return rc;
    if ((rc = dev_alloc(&s->d_tris, tris_total * 3))) return rc;
    std::vector<uint32_t> roots(n_meshes);
    std::vector<crt_node8*> blas_nodes(n_meshes);
    std::vector<uint32_t> blas_n8(n_meshes);
    uint64_t node_off = s->tlas_cap_nodes, tri_off = 0;
    for (uint32_t k = 0; k < n_meshes; ++k) {
        IHIPCHK(hipMemcpyAsync(s->d_nodes + 5 * node_off, blas[k].nodes, (size_t)blas[k].n8 * sizeof(crt_node8), hipMemcpyDeviceToDevice, st));
        IHIPCHK(hipMemcpyAsync(s->d_tris + 3 * tri_off, blas[k].recs, meshes[k].n_triangles * 48, hipMemcpyDeviceToDevice, st));
        crt::launch_rebase_nodes(s->d_nodes + 5 * node_off, blas[k].n8, (uint32_t)node_off, (uint32_t)tri_off, st);
        roots[k] = (uint32_t)node_off;
        blas_nodes[k] = blas[k].nodes; blas_n8[k] = blas[k].n8;
        node_off += blas[k].n8; tri_off += meshes[k].n_triangles;
    }
    s->blas_nodes8 = nodes_total - s->tlas_cap_nodes; s->blas_tris = tris_total;
    if ((rc = dev_alloc(&s->d_mesh_box, mesh_box.size()))) return rc;
    if ((rc = dev_alloc(&s->d_mesh_root, n_meshes))) return rc;
    IHIPCHK(hipMemcpyAsync(s->d_mesh_box, mesh_box.data(), mesh_box.size() * 4, hipMemcpyHostToDevice, st));
    IHIPCHK(hipMemcpyAsync(s->d_mesh_root, roots.data(), n_meshes * 4, hipMemcpyHostToDevice, st));
    const size_t C = capacity;
    if ((rc = dev_alloc(&s->d_inst, C * 4)) || (rc = dev_alloc(&s->d_w2o, C * 12)) || (rc = dev_alloc(&s->d_wbox, C * 6)) || (rc = dev_alloc(&s->d_in, C * 16)) ||
        (rc = dev_alloc(&s->d_rec, C * 4)) || (rc = dev_alloc(&s->d_box, C * 6)) || (rc = dev_alloc(&s->d_w2o_stage, C * 12)) || (rc = dev_alloc(&s->d_flag, 2)) ||
        (rc = dev_alloc(&s->d_overflow, 1)) || (rc = dev_alloc(&s->d_t8_stage, s->tlas_cap_nodes)) || (rc = dev_alloc(&s->d_tlas_box8, 6 * (size_t)s->tlas_cap_nodes)) ||
        (rc = dev_alloc(&s->d_box_idx, C * 3)) || (rc = dev_alloc(&s->d_tlas_table, sizeof(crt::RefitMesh) + 255 * sizeof(crt::RefitSeg))) ||
        (rc = dev_alloc(&s->d_cmask, s->tlas_cap_nodes)) || (rc = dev_alloc(&s->d_cm_parent, s->tlas_cap_nodes)) || (rc = dev_alloc(&s->d_cm_leaf, C)) ||
        (rc = dev_alloc(&s->d_mesh_of, C)) || (rc = dev_alloc(&s->d_mesh_of_stage, C)) ||
        (rc = dev_alloc(&s->d_o2w, C * 12)) || (rc = dev_alloc(&s->d_o2w_stage, C * 12)))
        return rc;
    crt::launch_box_triples(s->d_box_idx, capacity, st);
    IHIPCHK(hipMemsetAsync(s->d_overflow, 0, 4, st));
    // the TLAS build's space for `capacity` instances, reserved once
    const size_t cn = std::max<size_t>(C, 2), cn2 = 2 * cn - 1;
    auto P = crt::DeviceArena::padded;
    const size_t tmp = std::max(crt::lbvh_tmp_bytes(cn, CRT_GPU_BUILD_SAH), crt::cwbvh_tmp_bytes(cn2, cn));
    hipError_t he = s->arena.reserve(P(cn2 * sizeof(crt_flatnode)) + 2 * P(cn * 4) + tmp);
    if (he != hipSuccess) return fail(CRT_ERR_NOMEM, std::string("crt_instances_create: hipMalloc: ") + hipGetErrorString(he));
    s->d_flat = s->arena.take<crt_flatnode>(cn2);
    s->d_tri_order = s->arena.take<uint32_t>(cn);
    s->d_tri_slots = s->arena.take<int32_t>(cn);
    s->arena_mark = s->arena.used;
    IHIPCHK(hipStreamSynchronize(st));
    IHIPCHK(hipGetLastError());
    if ((build_flags & CRT_INSTANCES_UPDATABLE) && (rc = init_update_state(s, meshes, blas_nodes, blas_n8, roots, mesh_box))) return rc;
    if (n_instances) {
        IHIPCHK(hipMemcpyAsync(s->d_in, instances, (size_t)n_instances * sizeof(crt_instance), hipMemcpyHostToDevice, st));
        if ((rc = set_impl(s, s->d_in, n_instances))) return fail(rc, std::string("crt_instances_create: ") + crt_last_error());
    }
    s->build_wall_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    *out = owner.release();
    return CRT_OK;
}

// The staging of an add / replace: everything built for the new mesh list.  The publication swaps the live arrays in, so that what is
// freed here is either an abandoned attempt or the arrays the handle had before.
struct Remesh {
    struct Blas { crt_node8* nodes = nullptr; float4* recs = nullptr; uint32_t n8 = 0, depth8 = 0; };
    hipStream_t st = nullptr;             // set once work is enqueued: an abandoned attempt waits for it before its arrays go
    std::vector<float> box_all;           // host sources of enqueued uploads: the mesh boxes, the BLAS roots, the call's index triples
    std::vector<uint32_t> node_at;
    std::vector<int32_t> idx;
    std::vector<Blas> blas;               // the call's meshes as built: zero-based
    uint4* d_nodes = nullptr;
    float4* d_tris = nullptr;
    float* d_mesh_box = nullptr;
    uint32_t* d_mesh_root = nullptr;
    uint32_t* d_order_new = nullptr;      // level order of the call's meshes (discover_levels)
    std::unique_ptr<InstUpdateState> upd;
    ~Remesh() {
        if (st) (void)hipStreamSynchronize(st);
        for (auto& b : blas) { if (b.nodes) (void)hipFree(b.nodes); if (b.recs) (void)hipFree(b.recs); }
        void* bufs[] = {d_nodes, d_tris, d_mesh_box, d_mesh_root, d_order_new};
        for (void* p : bufs) if (p) (void)hipFree(p);
    }
};

// crt_instances_add_meshes (add: the call's meshes go behind the existing ones) and crt_instances_replace_meshes (ids name the meshes
// they stand for); DESIGN.md §15.  The new mesh list is laid out in NEW arrays as create lays it out: kept BLASes are copied from the live
// arrays with their bases moved (k_move_nodes), the call's BLASes from their builds.  A replace then stages the live instances' records,
// boxes and TLAS against the new roots, boxes and deepest BLAS.  Only when every check has passed do the new arrays become the live ones.
int remesh_impl(crt_instances* s, const uint32_t* ids, uint32_t n, const crt_blas_desc* meshes, uint32_t* first_id, bool add, const std::string& who) {
    const auto t0 = std::chrono::steady_clock::now();
    if (!s) return fail(CRT_ERR_INVALID, who + "null handle");
    if (!s->bound.empty())
        return fail(CRT_ERR_INVALID, who + "a scene renders this handle (crt_scene_create_instanced): its per-mesh shading tables would go stale; destroy the scene first");
    InstUpdateState* u = s->upd.get();
    if (!add && !u) return fail(CRT_ERR_INVALID, who + "the handle was created without CRT_INSTANCES_UPDATABLE");
    if (n && (!meshes || (!add && !ids))) return fail(CRT_ERR_INVALID, who + "null argument");
    const uint32_t M0 = s->n_meshes;
    if (add ? n > 0xffffffffu - M0 : n > M0) return fail(CRT_ERR_INVALID, who + (add ? "too many meshes" : "more meshes than the handle holds"));
    const uint32_t M1 = add ? M0 + n : M0;
    std::vector<int32_t> from(M1, -1);                // per mesh of the new list: its position in the call, or -1 = kept
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t m = add ? M0 + k : ids[k];
        if (m >= M1) return fail(CRT_ERR_INVALID, who + "mesh index " + std::to_string(m) + " is out of range");
        if (from[m] >= 0) return fail(CRT_ERR_INVALID, who + "mesh index " + std::to_string(m) + " is repeated");
        from[m] = (int32_t)k;
    }
    Remesh r;
    std::vector<float>& box_all = r.box_all;
    box_all.resize(6 * (size_t)M1);
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t m = add ? M0 + k : ids[k];
        const int rc = validate_mesh(meshes[k], m, who, &box_all[6 * (size_t)m]);
        if (rc) return rc;
    }
    if (n == 0) { if (first_id) *first_id = M0; return CRT_OK; }
    IHIPCHK(hipSetDevice(s->device));
    hipStream_t st = s->stream;
    IHIPCHK(hipEventRecord(s->ev0, st));
    int rc;
    r.st = st;
    r.blas.resize(n);
    for (uint32_t k = 0; k < n; ++k)
        if ((rc = build_blas(meshes[k], s->gpu_flags, st, who, &r.blas[k].nodes, &r.blas[k].recs, &r.blas[k].n8, &r.blas[k].depth8))) return rc;

    // the new layout, and where every kept mesh lies today
    std::vector<MeshSlot> slot(M1);
    std::vector<uint32_t>& node_at = r.node_at;
    node_at.resize(M1);
    std::vector<uint32_t> tri_at(M1), old_node_at(M0), old_tri_at(M0);
    uint64_t nodes_total = s->tlas_cap_nodes, tris_total = 0;
    uint32_t max_depth8 = 0;
    for (uint32_t m = 0; m < M1; ++m) {
        slot[m] = from[m] < 0 ? s->mesh[m] : MeshSlot{r.blas[from[m]].n8, (uint32_t)meshes[from[m]].n_triangles, r.blas[from[m]].depth8};
        nodes_total += slot[m].n8; tris_total += slot[m].n_tris;
        max_depth8 = std::max(max_depth8, slot[m].depth8);
    }
    if (nodes_total * CRT_NODE_ROWS * 16 >= (1ull << 32) || tris_total * CRT_TRI_ROWS * 16 >= (1ull << 32))
        return fail(CRT_ERR_LIMIT, who + "the packed node or record array would exceed 4 GiB");
    {
        uint64_t a = s->tlas_cap_nodes, b = 0;
        for (uint32_t m = 0; m < M1; ++m) { node_at[m] = (uint32_t)a; tri_at[m] = (uint32_t)b; a += slot[m].n8; b += slot[m].n_tris; }
        a = s->tlas_cap_nodes; b = 0;
        for (uint32_t m = 0; m < M0; ++m) { old_node_at[m] = (uint32_t)a; old_tri_at[m] = (uint32_t)b; a += s->mesh[m].n8; b += s->mesh[m].n_tris; }
    }
    // an add keeps the TLAS: its stack bound is known now.  A replace rebuilds the TLAS: stage_tlas bounds it
    uint32_t stack = s->stack_entries;
    if (add && s->n_instances) {
        stack = std::max<uint32_t>(2u, s->tlas_depth8 + max_depth8);
        if (stack > CRT_INST_STACK_ENTRIES)
            return fail(CRT_ERR_LIMIT, who + "TLAS depth + deepest BLAS exceed the walk's stack (" + std::to_string(stack) + " > " +
                                           std::to_string(CRT_INST_STACK_ENTRIES) + " entries)");
    }
    IHIPCHK(hipStreamSynchronize(st));
    {
        std::vector<float> live_box(6 * (size_t)M0);
        IHIPCHK(hipMemcpy(live_box.data(), s->d_mesh_box, live_box.size() * 4, hipMemcpyDeviceToHost));
        for (uint32_t m = 0; m < M0; ++m)
            if (from[m] < 0) std::copy(live_box.begin() + 6 * (size_t)m, live_box.begin() + 6 * (size_t)m + 6, box_all.begin() + 6 * (size_t)m);
    }
    if ((rc = dev_alloc(&r.d_nodes, nodes_total * 5)) || (rc = dev_alloc(&r.d_tris, tris_total * 3)) || (rc = dev_alloc(&r.d_mesh_box, box_all.size())) ||
        (rc = dev_alloc(&r.d_mesh_root, M1)))
        return rc;

    // the refit state of an updatable handle for the new list: kept meshes re-offset, the call's meshes discovered
    std::vector<int32_t>& idx = r.idx;
    if (u) {
        r.upd.reset(new (std::nothrow) InstUpdateState);
        InstUpdateState* nu = r.upd.get();
        if (!nu) return fail(CRT_ERR_NOMEM, who + "out of memory");
        const uint64_t n8_all = nodes_total - s->tlas_cap_nodes;
        nu->nv.resize(M1); nu->nt.resize(M1); nu->tri_off.resize(M1); nu->v_off.resize(M1); nu->level.resize(M1);
        nu->mesh_box = box_all;
        uint64_t v_total = 0, call_tris = 0;
        for (uint32_t m = 0; m < M1; ++m) {
            nu->nv[m] = from[m] < 0 ? u->nv[m] : (uint32_t)meshes[from[m]].n_vertices;
            nu->nt[m] = slot[m].n_tris; nu->tri_off[m] = tri_at[m]; nu->v_off[m] = v_total;
            v_total += nu->nv[m];
            if (from[m] >= 0) call_tris += slot[m].n_tris;
        }
        if (v_total >= (1ull << 32) / 12) return fail(CRT_ERR_LIMIT, who + "more vertices than an updatable handle stages");
        if ((rc = dev_alloc(&nu->d_src_idx, 3 * tris_total)) || (rc = dev_alloc(&nu->d_box8, 6 * n8_all)) || (rc = dev_alloc(&nu->d_order, n8_all)) ||
            (rc = dev_alloc(&nu->d_mesh_box_stage, 6 * (size_t)M1)) || (rc = dev_alloc(&nu->d_vstage, 3 * v_total)) || (rc = dev_alloc(&nu->d_check, 8 * (size_t)M1)))
            return rc;
        IHIPCHK(hipHostMalloc(reinterpret_cast<void**>(&nu->h_check), 8 * (size_t)M1 * sizeof(uint32_t)));
        IHIPCHK(hipEventCreate(&nu->ev0));
        IHIPCHK(hipEventCreate(&nu->ev1));
        std::vector<crt::RefitTree> trees(n);
        for (uint32_t k = 0; k < n; ++k) {
            const uint32_t m = add ? M0 + k : ids[k];
            trees[k] = crt::RefitTree{r.blas[k].nodes, false, 5u, r.blas[k].n8, node_at[m]};
        }
        std::vector<std::vector<uint32_t>> lv;
        if ((rc = crt::discover_levels(trees.data(), n, st, &r.d_order_new, lv))) return rc;
        idx.resize(3 * call_tris);
        uint64_t io = 0;
        for (uint32_t m = 0; m < M1; ++m) {
            // a tree's nodes fill positions [its node offset in the BLAS region, + n8) of the order, as init_update_state lays them out
            const uint32_t pos = node_at[m] - s->tlas_cap_nodes;
            if (from[m] < 0) {
                const std::vector<uint32_t>& ol = u->level[m];
                nu->level[m].resize(ol.size());
                for (size_t l = 0; l < ol.size(); ++l) nu->level[m][l] = ol[l] - ol[0] + pos;
                crt::launch_move_order(u->d_order + ol[0], nu->d_order + pos, slot[m].n8, node_at[m] - old_node_at[m], st);
                IHIPCHK(hipMemcpyAsync(nu->d_src_idx + 3 * (size_t)tri_at[m], u->d_src_idx + 3 * (size_t)old_tri_at[m], 12 * (size_t)slot[m].n_tris,
                                       hipMemcpyDeviceToDevice, st));
            } else {
                const uint32_t k = (uint32_t)from[m];
                const std::vector<uint32_t>& ol = lv[k];
                nu->level[m].resize(ol.size());
                for (size_t l = 0; l < ol.size(); ++l) nu->level[m][l] = ol[l] - ol[0] + pos;
                IHIPCHK(hipMemcpyAsync(nu->d_order + pos, r.d_order_new + ol[0], 4 * (size_t)slot[m].n8, hipMemcpyDeviceToDevice, st));
                for (size_t i = 0; i < meshes[k].n_triangles; ++i)
                    for (int j = 0; j < 3; ++j) idx[io + 3 * i + j] = meshes[k].triangles[i].v[j];
                IHIPCHK(hipMemcpyAsync(nu->d_src_idx + 3 * (size_t)tri_at[m], idx.data() + io, 12 * (size_t)slot[m].n_tris, hipMemcpyHostToDevice, st));
                io += 3 * (uint64_t)slot[m].n_tris;
            }
            nu->max_levels = std::max(nu->max_levels, (uint32_t)nu->level[m].size() - 1u);
        }
        IHIPCHK(hipMemsetAsync(nu->d_box8, 0, 24 * n8_all, st));
        auto A = [](size_t b) { return (b + 15) & ~size_t(15); };
        nu->table_cap = A(M1 * sizeof(crt::RefitMesh)) + A(M1 * 4) + A(M1 * sizeof(crt::RefitSeg)) + (size_t)M1 * nu->max_levels * sizeof(crt::RefitSeg);
        if ((rc = dev_alloc(&nu->d_table, nu->table_cap))) return rc;
        nu->bytes = 4 * n8_all + 24 * n8_all + 12 * tris_total + 64 * (uint64_t)s->capacity + 24 * (uint64_t)M1 + 12 * v_total + 32 * (uint64_t)M1 +
                    nu->table_cap;
    }

    // the repack: the TLAS region as it is, then every BLAS at its new offset
    IHIPCHK(hipMemcpyAsync(r.d_nodes, s->d_nodes, (size_t)s->tlas_cap_nodes * sizeof(crt_node8), hipMemcpyDeviceToDevice, st));
    for (uint32_t m = 0; m < M1; ++m) {
        const bool kept = from[m] < 0;
        const void* src_nodes = kept ? static_cast<const void*>(s->d_nodes + 5 * (size_t)old_node_at[m]) : r.blas[from[m]].nodes;
        const float4* src_recs = kept ? s->d_tris + 3 * (size_t)old_tri_at[m] : r.blas[from[m]].recs;
        // the wrapped difference new - old offset; a fresh build's offsets are 0
        crt::launch_move_nodes(src_nodes, r.d_nodes + 5 * (size_t)node_at[m], slot[m].n8, node_at[m] - (kept ? old_node_at[m] : 0u),
                               tri_at[m] - (kept ? old_tri_at[m] : 0u), st);
        IHIPCHK(hipMemcpyAsync(r.d_tris + 3 * (size_t)tri_at[m], src_recs, 48 * (size_t)slot[m].n_tris, hipMemcpyDeviceToDevice, st));
    }
    IHIPCHK(hipMemcpyAsync(r.d_mesh_box, box_all.data(), box_all.size() * 4, hipMemcpyHostToDevice, st));
    IHIPCHK(hipMemcpyAsync(r.d_mesh_root, node_at.data(), (size_t)M1 * 4, hipMemcpyHostToDevice, st));
    IHIPCHK(hipGetLastError());

    // a replace: the live instances against the NEW boxes, roots and deepest BLAS, into staging (the last refusals)
    const uint32_t ni = s->n_instances;
    TlasStage ts;
    if (!add && ni > 0 && (rc = stage_tlas(s, u->d_live, ni, MeshTables{r.d_mesh_box, r.d_mesh_root, M1, max_depth8}, who, ts))) return rc;
    IHIPCHK(hipStreamSynchronize(st));                // the new arrays are complete, and nothing in flight reads the old ones
    IHIPCHK(hipGetLastError());

    // publication: r takes the previous arrays and frees them
    std::swap(s->d_nodes, r.d_nodes); std::swap(s->d_tris, r.d_tris); std::swap(s->d_mesh_box, r.d_mesh_box); std::swap(s->d_mesh_root, r.d_mesh_root);
    s->mesh.swap(slot);
    s->n_meshes = M1; s->blas_nodes8 = nodes_total - s->tlas_cap_nodes; s->blas_tris = tris_total; s->max_blas_depth8 = max_depth8;
    if (u) {
        InstUpdateState* nu = r.upd.get();
        std::swap(nu->d_live, u->d_live);
        nu->have_times = u->have_times; nu->device_ms = u->device_ms; nu->wall_ms = u->wall_ms;
        s->upd.swap(r.upd);
    }
    if (!add && ni > 0) {
        if ((rc = publish_tlas(s, s->upd->d_live, ni, ts))) return rc;
        IHIPCHK(hipStreamSynchronize(st));
        s->n_tlas8 = ts.n8; s->tlas_depth8 = ts.depth8; s->stack_entries = ts.stack;
    } else {
        s->stack_entries = stack;
    }
    IHIPCHK(hipEventRecord(s->ev1, st));
    IHIPCHK(hipEventSynchronize(s->ev1));
    IHIPCHK(hipGetLastError());
    IHIPCHK(hipEventElapsedTime(&s->set_device_ms, s->ev0, s->ev1));
    if (first_id) *first_id = M0;
    ++s->mutations;
    s->set_wall_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return CRT_OK;
}

}  // namespace

namespace crt {

void instances_view(const crt_instances* h, InstancesView* out) {
    *out = InstancesView{h->device, h->d_nodes, h->d_tris, h->d_inst, h->d_w2o, h->d_mesh_of, h->d_cmask, h->n_instances, h->stack_entries, h->n_meshes,
                         h->n_tlas8, h->tlas_depth8, h->max_blas_depth8, h->blas_nodes8, h->blas_tris, h->d_o2w, h->capacity, h->mutations};
}
uint32_t instances_mesh_triangles(const crt_instances* h, uint32_t mesh) { return h->mesh[mesh].n_tris; }
int instances_bind(crt_instances* h, hipStream_t stream, const InstOffsetRule& rule) {
    // the rule against the LIVE instances, on the handle's stream behind whatever it has queued
    if (h->n_instances) {
        hipStream_t st = h->stream;
        IHIPCHK(hipMemsetAsync(h->d_flag, 0, 4, st));
        IHIPCHK(hipMemsetAsync(h->d_flag + 1, 0xff, 4, st));
        check_offsets(h, rule, h->d_mesh_of, h->n_instances, h->n_meshes);
        uint32_t flag[2] = {0u, 0u};
        IHIPCHK(hipMemcpyAsync(flag, h->d_flag, 8, hipMemcpyDeviceToHost, st));
        IHIPCHK(hipStreamSynchronize(st));
        IHIPCHK(hipGetLastError());
        if (flag[0]) return fail(CRT_ERR_INVALID, "crt_scene_create_instanced: " + offset_refusal(flag));
    }
    try { h->bound.push_back(crt_instances::Bound{stream, rule}); } catch (const std::exception&) { return fail(CRT_ERR_NOMEM, "crt_scene_create_instanced: out of memory"); }
    return CRT_OK;
}
void instances_unbind(crt_instances* h, hipStream_t stream) {
    auto it = std::find_if(h->bound.begin(), h->bound.end(), [&](const crt_instances::Bound& b) { return b.stream == stream; });
    if (it != h->bound.end()) h->bound.erase(it);
}
// The pass itself runs on the handle's stream only, and only when a publish or refit has left the masks stale — calls that have waited
// for every bound stream first, so no frame in flight reads what the pass rewrites.  `stream` then waits for the event behind the LAST
// pass, whoever asked for it (a masked trace may have enqueued it and not be done): on the device, and once per pass (*seen).
int instances_child_masks_for(crt_instances* h, hipStream_t stream, uint64_t* seen) {
    const int rc = ensure_child_masks(h);
    if (rc) return rc;
    if (*seen != h->cmask_gen) {
        IHIPCHK(hipStreamWaitEvent(stream, h->ev_cmask, 0));
        *seen = h->cmask_gen;
    }
    return CRT_OK;
}

}  // namespace crt

extern "C" {

int crt_instance_inverse(const float object_to_world[12], float world_to_object[12]) {
    if (!object_to_world || !world_to_object) return fail(CRT_ERR_INVALID, "crt_instance_inverse: null argument");
    if (!crt::instance_inverse(object_to_world, world_to_object))
        return fail(CRT_ERR_INVALID, "crt_instance_inverse: the matrix is not finite, or singular, or its inverse is not finite");
    return CRT_OK;
}

int crt_instance_world_box(const float object_to_world[12], const float box[6], float out[6]) {
    if (!object_to_world || !box || !out) return fail(CRT_ERR_INVALID, "crt_instance_world_box: null argument");
    crt::instance_world_box(object_to_world, box, out);
    return CRT_OK;
}

int crt_instance_lights(const float object_to_world[12], const crt_light* in, size_t n, crt_light* out) {
    if (!object_to_world || (n && (!in || !out))) return fail(CRT_ERR_INVALID, "crt_instance_lights: null argument");
    float w[12];
    if (!crt::instance_inverse(object_to_world, w))
        return fail(CRT_ERR_INVALID, "crt_instance_lights: the matrix is not finite, or singular, or its inverse is not finite");
    const bool identity = crt::instance_is_identity(object_to_world);
    for (size_t k = 0; k < n; ++k) {
        float src[18], dst[18];
        std::memcpy(src, &in[k], sizeof src);
        crt::light_to_world(object_to_world, w, identity, src, dst);
        std::memcpy(&out[k], dst, sizeof dst);
    }
    return CRT_OK;
}

int crt_lights_finish(crt_light* lights, size_t n) {
    if (n && !lights) return fail(CRT_ERR_INVALID, "crt_lights_finish: null argument");
    if (n == 0) return CRT_OK;
    try {
        size_t p2 = 1;
        while (p2 < n) p2 <<= 1;
        std::vector<float> a(p2, 0.0f);
        for (size_t k = 0; k < n; ++k) a[k] = crt::light_area_term(lights[k].area_pdf[0]);
        for (size_t m = p2; m > 1; m >>= 1)
            for (size_t j = 0; j < m / 2; ++j) a[j] = a[2 * j] + a[2 * j + 1];
        const float S = a[0];
        for (size_t k = 0; k < n; ++k) lights[k].area_pdf[1] = crt::light_pdf(crt::light_area_term(lights[k].area_pdf[0]), S);
    } catch (const std::exception& e) {
        return fail(CRT_ERR_NOMEM, std::string("crt_lights_finish: ") + e.what());
    }
    return CRT_OK;
}

int crt_instances_create(const crt_blas_desc* meshes, uint32_t n_meshes, const crt_instance* instances, uint32_t n_instances, uint32_t capacity,
                         uint32_t build_flags, crt_instances** out) {
    try {
        return create_impl(meshes, n_meshes, instances, n_instances, capacity, build_flags, out);
    } catch (const std::exception& e) {
        return fail(CRT_ERR_NOMEM, std::string("crt_instances_create: ") + e.what());
    }
}

int crt_instances_set(crt_instances* s, const crt_instance* instances, uint32_t n_instances) {
    if (!s || (n_instances && !instances)) return fail(CRT_ERR_INVALID, "crt_instances_set: null argument");
    if (n_instances > s->capacity) return fail(CRT_ERR_INVALID, "crt_instances_set: more instances than the capacity given at create");
    IHIPCHK(hipSetDevice(s->device));
    if (n_instances) IHIPCHK(hipMemcpyAsync(s->d_in, instances, (size_t)n_instances * sizeof(crt_instance), hipMemcpyHostToDevice, s->stream));
    return set_impl(s, s->d_in, n_instances);
}

int crt_instances_set_device(crt_instances* s, const void* d_instances, uint32_t n_instances, int sync) {
    if (!s || (n_instances && !d_instances)) return fail(CRT_ERR_INVALID, "crt_instances_set_device: null argument");
    IHIPCHK(hipSetDevice(s->device));
    (void)sync;                                   // a set checks its instances on the host before it publishes anything: it always returns done
    return set_impl(s, d_instances, n_instances);
}

int crt_instances_refit(crt_instances* s, const crt_instance* instances, uint32_t n_instances) {
    if (!s || (n_instances && !instances)) return fail(CRT_ERR_INVALID, "crt_instances_refit: null argument");
    if (n_instances != s->n_instances)
        return fail(CRT_ERR_INVALID, "crt_instances_refit: n_instances (" + std::to_string(n_instances) + ") differs from the live count (" +
                                         std::to_string(s->n_instances) + ")");
    IHIPCHK(hipSetDevice(s->device));
    if (n_instances) IHIPCHK(hipMemcpyAsync(s->d_in, instances, (size_t)n_instances * sizeof(crt_instance), hipMemcpyHostToDevice, s->stream));
    try {
        return refit_impl(s, s->d_in, n_instances, "crt_instances_refit: ");
    } catch (const std::exception& e) {
        return fail(CRT_ERR_NOMEM, std::string("crt_instances_refit: ") + e.what());
    }
}

int crt_instances_refit_device(crt_instances* s, const void* d_instances, uint32_t n_instances, int sync) {
    if (!s || (n_instances && !d_instances)) return fail(CRT_ERR_INVALID, "crt_instances_refit_device: null argument");
    IHIPCHK(hipSetDevice(s->device));
    (void)sync;                                   // the check's verdict waits on the host: a refit always returns done, as a set does
    try {
        return refit_impl(s, d_instances, n_instances, "crt_instances_refit_device: ");
    } catch (const std::exception& e) {
        return fail(CRT_ERR_NOMEM, std::string("crt_instances_refit_device: ") + e.what());
    }
}

int crt_instances_trace_device(crt_instances* s, const void* d_rays, size_t n, void* d_hits, void* d_instance_of_hit, int mode, void* d_stats, int sync) {
    if (!s || (n && (!d_rays || !d_hits))) return fail(CRT_ERR_INVALID, "crt_instances_trace_device: null argument");
    const int base = mode & ~CRT_TRACE_INSTANCE_MASK;
    if (base != CRT_TRACE_CLOSEST && base != CRT_TRACE_ANY)
        return fail(CRT_ERR_INVALID, "crt_instances_trace_device: mode must be CRT_TRACE_CLOSEST or CRT_TRACE_ANY, optionally | CRT_TRACE_INSTANCE_MASK");
    const bool masked = (mode & CRT_TRACE_INSTANCE_MASK) != 0;
    if (n >= (1ull << 31)) return fail(CRT_ERR_LIMIT, "crt_instances_trace_device: too many rays for one launch");
    IHIPCHK(hipSetDevice(s->device));
    if (n == 0) return CRT_OK;
    crt::InstMaskTraceArgs a{};
    a.nodes = s->d_nodes; a.tris = s->d_tris; a.inst = s->d_inst;
    a.rays = static_cast<const float4*>(d_rays); a.hits = static_cast<float4*>(d_hits);
    a.inst_out = static_cast<int32_t*>(d_instance_of_hit); a.stats = static_cast<uint32_t*>(d_stats);
    a.n = (uint32_t)n; a.n_instances = s->n_instances; a.stack_entries = s->stack_entries;
    a.refill_min = 8; a.tri_min = 2;              // crt_trace's defaults (options refill_min, tri_min)
    a.overflow = s->d_overflow;
    a.child_masks = s->d_cmask; a.n_tlas8 = s->n_tlas8;
    if (masked) { const int rc = ensure_child_masks(s); if (rc) return rc; }
    // k_trace's grid: every XCD group's share of 4096-ray units, in 1024-ray chunks
    const uint64_t share = ((n + 4095) / 4096 + 7) / 8 * 4096;
    const uint32_t chunks = (uint32_t)std::max<uint64_t>(8, 8 * ((share + 1023) / 1024));
    crt::launch_trace_instances(a, base, d_stats != nullptr, masked, chunks, s->stream);
    IHIPCHK(hipGetLastError());
    if (sync) IHIPCHK(hipStreamSynchronize(s->stream));
    return CRT_OK;
}

int crt_instances_trace(crt_instances* s, const crt_ray* rays, size_t n, crt_hit* hits, int32_t* instance_of_hit, int mode, crt_ray_stats* stats) {
    if (!s || (n && (!rays || !hits))) return fail(CRT_ERR_INVALID, "crt_instances_trace: null argument");
    const int base = mode & ~CRT_TRACE_INSTANCE_MASK;
    if (base != CRT_TRACE_CLOSEST && base != CRT_TRACE_ANY)
        return fail(CRT_ERR_INVALID, "crt_instances_trace: mode must be CRT_TRACE_CLOSEST or CRT_TRACE_ANY, optionally | CRT_TRACE_INSTANCE_MASK");
    IHIPCHK(hipSetDevice(s->device));
    if (n == 0) return CRT_OK;
    if (n > s->t_cap) {
        void* bufs[] = {s->d_t_rays, s->d_t_hits, s->d_t_inst, s->d_t_stats};
        for (void* p : bufs) if (p) (void)hipFree(p);
        s->d_t_rays = s->d_t_hits = s->d_t_inst = s->d_t_stats = nullptr;
        s->t_cap = 0;
        IHIPCHK(hipMalloc(&s->d_t_rays, n * sizeof(crt_ray)));
        IHIPCHK(hipMalloc(&s->d_t_hits, n * sizeof(crt_hit)));
        IHIPCHK(hipMalloc(&s->d_t_inst, n * 4));
        IHIPCHK(hipMalloc(&s->d_t_stats, n * sizeof(crt_ray_stats)));
        s->t_cap = n;
    }
    IHIPCHK(hipMemcpyAsync(s->d_t_rays, rays, n * sizeof(crt_ray), hipMemcpyHostToDevice, s->stream));
    int rc = crt_instances_trace_device(s, s->d_t_rays, n, s->d_t_hits, s->d_t_inst, mode, stats ? s->d_t_stats : nullptr, 0);
    if (rc) return rc;
    IHIPCHK(hipMemcpyAsync(hits, s->d_t_hits, n * sizeof(crt_hit), hipMemcpyDeviceToHost, s->stream));
    if (instance_of_hit) IHIPCHK(hipMemcpyAsync(instance_of_hit, s->d_t_inst, n * 4, hipMemcpyDeviceToHost, s->stream));
    if (stats) IHIPCHK(hipMemcpyAsync(stats, s->d_t_stats, n * sizeof(crt_ray_stats), hipMemcpyDeviceToHost, s->stream));
    IHIPCHK(hipStreamSynchronize(s->stream));
    return CRT_OK;
}

int crt_instances_get_info(crt_instances* s, crt_instances_info* out) {
    if (!s || !out) return fail(CRT_ERR_INVALID, "crt_instances_get_info: null argument");
    IHIPCHK(hipSetDevice(s->device));
    IHIPCHK(hipStreamSynchronize(s->stream));
    crt_instances_info i{};
    i.n_meshes = s->n_meshes; i.n_instances = s->n_instances; i.capacity = s->capacity; i.stack_entries = s->stack_entries;
    i.tlas_nodes8 = s->n_tlas8; i.tlas_depth8 = s->tlas_depth8; i.max_blas_depth8 = s->max_blas_depth8;
    IHIPCHK(hipMemcpy(&i.stack_overflows, s->d_overflow, 4, hipMemcpyDeviceToHost));
    i.blas_nodes8 = s->blas_nodes8; i.blas_tris = s->blas_tris;
    i.blas_bytes = s->blas_nodes8 * sizeof(crt_node8) + s->blas_tris * 48;
    i.tlas_bytes = (uint64_t)s->tlas_cap_nodes * sizeof(crt_node8);
    i.instance_bytes = (uint64_t)s->capacity * (64 + 48 + 24 + 64 + 64 + 24 + 48 + 48 + 48)    // live records, matrices (both ways), boxes + the set's staging
                       + (uint64_t)s->tlas_cap_nodes * (8 + 4) + (uint64_t)s->capacity * 4;   // TLAS child masks + their parent / leaf links
    i.tlas_build_bytes = (uint64_t)s->arena.cap + (uint64_t)s->tlas_cap_nodes * sizeof(crt_node8);   // the TLAS builder's arena + node staging
    i.set_device_ms = s->set_device_ms; i.set_wall_ms = s->set_wall_ms; i.create_wall_ms = s->build_wall_ms;
    *out = i;
    return CRT_OK;
}

int crt_instances_debug_read(crt_instances* s, int which, void* dst, size_t cap_bytes, size_t* n_out) {
    if (!s) return fail(CRT_ERR_INVALID, "crt_instances_debug_read: null handle");
    const void* src = nullptr;
    size_t n = 0, item = 0;
    switch (which) {
        case 0: src = s->d_w2o; n = s->n_instances; item = 48; break;
        case 1: src = s->d_wbox; n = s->n_instances; item = 24; break;
        case 2: src = s->d_nodes; n = s->n_tlas8; item = sizeof(crt_node8); break;
        case 3: src = s->d_inst; n = s->n_instances; item = 64; break;
        case 4: src = s->d_nodes + 5 * (size_t)s->tlas_cap_nodes; n = s->blas_nodes8; item = sizeof(crt_node8); break;
        case 5: src = s->d_tris; n = s->blas_tris; item = 48; break;
        case 6: src = s->d_cmask; n = s->n_instances ? s->n_tlas8 : 0; item = 8; break;
        case 7: src = s->d_o2w; n = s->n_instances; item = 48; break;
        default: return fail(CRT_ERR_INVALID, "crt_instances_debug_read: which must be 0..7");
    }
    if (n_out) *n_out = n;
    if (!dst || n == 0) return CRT_OK;
    if (cap_bytes < n * item) return fail(CRT_ERR_INVALID, "crt_instances_debug_read: destination too small");
    IHIPCHK(hipSetDevice(s->device));
    if (which == 6) { const int rc = ensure_child_masks(s); if (rc) return rc; }
    IHIPCHK(hipStreamSynchronize(s->stream));
    IHIPCHK(hipMemcpy(dst, src, n * item, hipMemcpyDeviceToHost));
    return CRT_OK;
}

int crt_instances_tree_cost(crt_instances* s, int32_t mesh, crt_tree_cost* out) {
    if (!s || !out) return fail(CRT_ERR_INVALID, "crt_instances_tree_cost: null argument");
    *out = crt_tree_cost{};
    if (mesh < -1 || (mesh >= 0 && (uint32_t)mesh >= s->n_meshes)) return fail(CRT_ERR_INVALID, "crt_instances_tree_cost: mesh must be -1 (the TLAS) or a mesh index");
    IHIPCHK(hipSetDevice(s->device));
    { const int wrc = wait_bound(s); if (wrc) return wrc; }
    IHIPCHK(hipStreamSynchronize(s->stream));
    if (mesh < 0) {
        if (s->n_instances == 0) return CRT_OK;
        return crt::tree_cost_on_device(s->d_nodes, 5u, 0u, s->n_tlas8, 0u, s->stream, out);
    }
    uint64_t first = s->tlas_cap_nodes;           // the packed array: the TLAS region, then the BLASes in mesh order, each root first
    for (int32_t k = 0; k < mesh; ++k) first += s->mesh[(size_t)k].n8;
    return crt::tree_cost_on_device(s->d_nodes, 5u, first, s->mesh[(size_t)mesh].n8, first, s->stream, out);
}

int crt_instances_update_meshes(crt_instances* s, const uint32_t* mesh_ids, uint32_t n, const float* const* vertices, const size_t* n_vertices) {
    if (n && !vertices) return fail(CRT_ERR_INVALID, "crt_instances_update_meshes: null vertices");
    try {
        return update_impl(s, mesh_ids, n, vertices, nullptr, n_vertices, "crt_instances_update_meshes: ");
    } catch (const std::exception& e) {
        return fail(CRT_ERR_NOMEM, std::string("crt_instances_update_meshes: ") + e.what());
    }
}

int crt_instances_update_meshes_device(crt_instances* s, const uint32_t* mesh_ids, uint32_t n, const void* const* d_vertices, const size_t* n_vertices,
                                       int sync) {
    if (n && !d_vertices) return fail(CRT_ERR_INVALID, "crt_instances_update_meshes_device: null vertices");
    (void)sync;                                   // the TLAS rebuild waits on the host: an update always returns done, as a set does
    try {
        return update_impl(s, mesh_ids, n, nullptr, d_vertices, n_vertices, "crt_instances_update_meshes_device: ");
    } catch (const std::exception& e) {
        return fail(CRT_ERR_NOMEM, std::string("crt_instances_update_meshes_device: ") + e.what());
    }
}

int crt_instances_add_meshes(crt_instances* s, const crt_blas_desc* meshes, uint32_t n, uint32_t* first_id) {
    try {
        return remesh_impl(s, nullptr, n, meshes, first_id, true, "crt_instances_add_meshes: ");
    } catch (const std::exception& e) {
        return fail(CRT_ERR_NOMEM, std::string("crt_instances_add_meshes: ") + e.what());
    }
}

int crt_instances_replace_meshes(crt_instances* s, const uint32_t* mesh_ids, uint32_t n, const crt_blas_desc* meshes) {
    try {
        return remesh_impl(s, mesh_ids, n, meshes, nullptr, false, "crt_instances_replace_meshes: ");
    } catch (const std::exception& e) {
        return fail(CRT_ERR_NOMEM, std::string("crt_instances_replace_meshes: ") + e.what());
    }
}

int crt_instances_last_update(crt_instances* s, float* device_ms, float* wall_ms, uint64_t* state_bytes) {
    if (state_bytes) *state_bytes = (s && s->upd) ? s->upd->bytes : 0;
    if (!s) return fail(CRT_ERR_INVALID, "crt_instances_last_update: null handle");
    if (!s->upd) return fail(CRT_ERR_INVALID, "crt_instances_last_update: the handle was created without CRT_INSTANCES_UPDATABLE");
    if (!s->upd->have_times) return fail(CRT_ERR_INVALID, "crt_instances_last_update: no update yet");
    if (device_ms) *device_ms = s->upd->device_ms;
    if (wall_ms) *wall_ms = s->upd->wall_ms;
    return CRT_OK;
}

int crt_instances_destroy(crt_instances* s) {
    if (!s) return CRT_OK;
    if (!s->bound.empty())
        return fail(CRT_ERR_INVALID, "crt_instances_destroy: a scene renders this handle (crt_scene_create_instanced): destroy the scene first");
    (void)hipSetDevice(s->device);
    delete s;
    return CRT_OK;
}

}  // extern "C"
