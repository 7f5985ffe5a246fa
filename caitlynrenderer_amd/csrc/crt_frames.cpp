// Frame dispatch of the device half of include/crt.h: the shard's frame buffers, what a frame's options make of it (FramePlan), the
// chain of launches of one batch of samples on a flat and on an instanced scene, crt_render_frame[s], crt_sync, the frame's statistics
// and the debug hooks that read what the last chain left.  (The rest of the device half is crt_device.cpp and crt_outputs.cpp.)
// Replaces Scene::Render (Caitlyn/Scene.h:1158-1231).  Every kernel of a frame is enqueued on the scene's stream, queue lengths stay
// on the device, and the host synchronises once per call (never inside the frame).
#include "crt_scene.hpp"

using crt::dev_alloc;
using crt::fail;

namespace {

int build_shard(crt_scene* s) {
    crt::deal_tiles(s->width, s->height, s->tile, s->rank, s->world, s->tiles, &s->n_local_in_frame);
    s->n_local_tiles = (uint32_t)s->tiles.size();
    const uint64_t px = (uint64_t)s->n_local_tiles * s->tile * s->tile;
    if (px >= (1ull << 31)) return fail(CRT_ERR_LIMIT, "framebuffer shard too large for 32-bit pixel indices");
    s->n_local_pixels = (uint32_t)px;
    return CRT_OK;
}

void free_frame_buffers(crt_scene* s) {
    void** ptrs[] = {(void**)&s->d_tile_xy, (void**)&s->d_tile_order, (void**)&s->d_tile_cost, (void**)&s->d_sum, (void**)&s->d_linear, (void**)&s->d_rgba, (void**)&s->d_rays[0],
                     (void**)&s->d_rays[1], (void**)&s->d_nee, (void**)&s->d_contrib, (void**)&s->d_nee_perm, (void**)&s->d_qhits, (void**)&s->pb.L, (void**)&s->pb.T, (void**)&s->pb.seed,
                     (void**)&s->d_lfinal, (void**)&s->d_qinst, (void**)&s->d_rays_lens};
    for (void** p : ptrs) { if (*p) hipFree(*p); *p = nullptr; }
    s->batch_cap = 1;
    s->lens_sub_capacity = 0;
    s->defer_cap = s->defer_regions = s->defer_sub_capacity = s->lfinal_cap = 0;
    // the bins' capacities and offsets describe the queues that were just freed: back to "everything overflows"
    if (s->d_bins) (void)hipMemset(s->d_bins, 0, crt_scene::bins_words() * sizeof(uint32_t));
    if (s->h_tile_cost) { (void)hipHostFree(s->h_tile_cost); s->h_tile_cost = nullptr; }
    if (s->h_tile_order) { (void)hipHostFree(s->h_tile_order); s->h_tile_order = nullptr; }
    s->frame_buffers_ready = false;
}

// one sample's path-ray queues and path state, for the sub_capacity in force
int alloc_queues_and_paths(crt_scene* s) {
    const size_t P = s->n_local_pixels, Q = 8 * (size_t)s->sub_capacity;
    int rc;
    if ((rc = dev_alloc(&s->d_rays[0], 2 * Q)) || (rc = dev_alloc(&s->d_rays[1], 2 * Q))) return rc;
    s->rays_doubled = false;
    if ((!s->pb.L && (rc = dev_alloc(&s->pb.L, P))) || (!s->pb.T && (rc = dev_alloc(&s->pb.T, P))) || (!s->pb.seed && (rc = dev_alloc(&s->pb.seed, P)))) return rc;
    return CRT_OK;
}

}  // namespace

int crt::alloc_frame_buffers(crt_scene* s) {
    free_frame_buffers(s);
    int rc = build_shard(s);
    if (rc) return rc;
    const size_t P = s->n_local_pixels;
    if ((rc = dev_alloc(&s->d_tile_xy, s->n_local_tiles))) return rc;
    HIPCHK(hipMemcpy(s->d_tile_xy, s->tiles.data(), s->tiles.size() * sizeof(uint2), hipMemcpyHostToDevice));
    {   // processing order: centre-out until a frame has been measured
        const uint32_t nt = s->n_local_tiles, T = s->tile;
        const float cx = 0.5f * (float)((s->width + T - 1) / T) - 0.5f, cy = 0.5f * (float)((s->height + T - 1) / T) - 0.5f;
        std::vector<uint32_t> order(nt);
        for (uint32_t i = 0; i < nt; ++i) order[i] = i;
        auto d2 = [&](uint32_t i) { const float dx = (float)s->tiles[i].x - cx, dy = (float)s->tiles[i].y - cy; return dx * dx + dy * dy; };
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return d2(a) < d2(b); });
        if ((rc = dev_alloc(&s->d_tile_order, std::max<uint32_t>(nt, 1)))) return rc;
        if ((rc = dev_alloc(&s->d_tile_cost, std::max<uint32_t>(nt, 1)))) return rc;
        HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&s->h_tile_cost), std::max<uint32_t>(nt, 1) * sizeof(uint32_t)));
        HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&s->h_tile_order), std::max<uint32_t>(nt, 1) * sizeof(uint32_t)));
        if (nt) HIPCHK(hipMemcpy(s->d_tile_order, order.data(), nt * sizeof(uint32_t), hipMemcpyHostToDevice));
        if (!s->ev_tile_cost) HIPCHK(hipEventCreateWithFlags(&s->ev_tile_cost, hipEventDisableTiming));
        if (!s->ev_tile_order) HIPCHK(hipEventCreateWithFlags(&s->ev_tile_order, hipEventDisableTiming));
        s->tile_state = crt_scene::TILES_WANT;
        s->tile_order_uploading = s->tiles_measured_once = false;
        s->tile_cost_spread = 0.f;
    }
    if ((rc = dev_alloc(&s->d_sum, 3 * std::max<size_t>(P, 1)))) return rc;     // a shard may hold no tile at all (more devices or streams than tiles)
    HIPCHK(hipMemset(s->d_sum, 0, 3 * std::max<size_t>(P, 1) * sizeof(float)));
    // a workgroup group handles every 8th unit of 4096 pixels/rays, so it can emit at most this many rays per segment
    s->sub_capacity = (uint32_t)(((P + 4095) / 4096 + 7) / 8 * 4096);
    // the deferred shadow rays' buffers (inplace_shadow 0 / 2) and the hit buffer of the bounce pools (bounce_refill = 1) are allocated
    // by the first frame that needs them; path state and ray queues exist only for multi-segment paths, and for the queue-fed frames of
    // an instanced scene
    if ((s->max_depth > 1 || s->inst) && (rc = alloc_queues_and_paths(s))) return rc;
    s->frame_buffers_ready = true;
    return CRT_OK;
}

int crt::ensure_frame(crt_scene* s) { return s->frame_buffers_ready ? CRT_OK : alloc_frame_buffers(s); }

// the closest hits of the path-ray queue, and of an instanced scene the hit instances beside them: allocated by the first call that needs them
int crt::ensure_queue_hits(crt_scene* s, bool hits, bool instances) {
    const size_t Q = 8 * (size_t)s->sub_capacity;
    int rc;
    if (hits && !s->d_qhits && (rc = dev_alloc(&s->d_qhits, Q))) return rc;
    if (instances && !s->d_qinst && (rc = dev_alloc(&s->d_qinst, Q))) return rc;
    return CRT_OK;
}

// k_raygen's arguments for primary rays into `rays` / `count`, in storage order: the adaptive tile order belongs to the fused
// first-segment kernels.  zero_bank: the launch clears the other frame's counter bank, as k_segment<FIRST> does
crt::RaygenArgs crt::raygen_args(const crt_scene* s, const crt::FrameArgs& f, float4* rays, uint32_t* count, bool zero_bank) {
    crt::RaygenArgs ra{};
    ra.f = f;
    ra.f.tile_order = nullptr;
    ra.rays = rays; ra.count = count; ra.sub_capacity = s->sub_capacity; ra.pb = s->pb;
    if (zero_bank) { ra.zero_counts = s->d_counts + (size_t)(s->bank ^ 1u) * kCounters; ra.n_zero = kCounters; }
    return ra;
}

// k_closest_instances_queue's arguments for the queue in `rays` / `count`; a scene with "instance_masks" walks by the handle's TLAS child masks
crt::InstMaskQueueArgs crt::inst_queue_args(const crt_scene* s, const crt::InstancesView& v, const float4* rays, const uint32_t* count, uint32_t ray_mask,
                                            unsigned long long* visit_totals) {
    crt::InstMaskQueueArgs qa{};
    qa.nodes = v.nodes; qa.tris = v.tris; qa.inst = v.inst;
    if (s->instance_masks != 0u) { qa.child_masks = v.child_masks; qa.n_tlas8 = v.tlas_nodes8; qa.ray_mask = ray_mask; }
    qa.rays = rays; qa.count = count; qa.hits = s->d_qhits; qa.hit_inst = s->d_qinst;
    qa.sub_capacity = s->sub_capacity; qa.n_instances = v.n_instances; qa.stack_entries = v.stack_entries;
    qa.refill_min = 8; qa.tri_min = 2;          // crt_instances_trace's
    qa.visit_totals = visit_totals; qa.overflow = s->d_overflow;
    return qa;
}

namespace {

// A frame's FORM (DESIGN.md "Where a frame is decided"): everything the scene's options make of a chain of n_samples, decided once
// per chain by plan_frame, where each field is explained.  prepare_batch allocates what `need_*`, `defer_regions` and `bins` name, the
// two renderers launch what the rest says, and crt_render_frames' chunking and crt_debug_read_queue ask the same record.
struct FramePlan {
    bool instanced, lens, rays, env, queue_fed, bvh2, small_tree, bins, refill, batched_paths, any_deferred, folds, lanes4;
    uint32_t first_deferred, defer_regions, limit;
    bool need_queues, need_lens_queue, need_lfinal, need_qhits, need_qinst, need_visit_totals;
    bool first(uint32_t b) const { return b == 0 && !queue_fed && !instanced; }     // the fused first-segment kernels; false = a queue-fed segment
    bool inplace(uint32_t b) const { return b < first_deferred; }                   // shadow rays walked inside k_segment
    bool pretraced(uint32_t b) const { return env || (!first(b) && refill); }       // closest hits from k_closest_queue in d_qhits
};

// Pure host arithmetic on the scene's fields: allocates nothing, enqueues nothing, calls no HIP.
FramePlan plan_frame(const crt_scene* s, uint32_t n_samples) {
    FramePlan p{};
    p.instanced = s->inst != nullptr;   // the two-level walk of a crt_instances handle: every segment queue-fed, every shadow ray deferred
    p.rays = s->camera_rays();          // segment 0's rays are the caller's, through k_raygen_rays (crt_set_camera_rays): the camera is not read
    p.lens = s->lens() && !p.rays;      // segment 0's rays come from k_raygen_lens (camera aperture > 0)
    const bool fed = p.lens || p.rays;  // a ray generator of up to 8 samples per launch feeds segment 0, from a queue of its own on a flat scene
    p.env = s->env();                   // k_env_miss behind every closest-hit launch
    p.queue_fed = !p.instanced && (fed || p.env);    // a flat frame whose segment 0 is queue-fed too: no fused first-segment kernel, tile order untouched
    p.bvh2 = s->accel != 0u;            // the BVH2 frame mode (a comparison aid): shadow rays in place, one sample per chain
    p.small_tree = s->info.n_nodes8 < 64;               // plain per-lane closest-hit loop (tri_min = 0) and no bounce pools
    // bounce rays binned between the segments (option "ray_bins"): big trees, CWBVH walks, the lock-step segment kernels
    p.bins = s->ray_bins != 0u && s->max_depth > 1u && !p.small_tree && !p.bvh2 && !s->bounce_refill && !p.env;
    // option "bounce_refill": the closest hits of a bounce segment through lane-refill pools (k_closest_queue), then a shade-only pass
    p.refill = s->bounce_refill && !p.small_tree && !p.bvh2 && s->tri_min != 0u && !p.bins;
    p.batched_paths = n_samples > 1u && (s->max_depth > 1u || p.queue_fed);     // every sample its own path state and queue entries
    // Segments [first_deferred, max_depth) leave their NEE shadow rays to ONE any-hit launch behind the last segment.  Option
    // "inplace_shadow": 1 = in place, 0 = every segment deferred, 2 = bounce segments deferred, 3 = 2 for trees of 64+ nodes.  An
    // instanced frame and one with an environment give every segment a slot region, whatever the option says; BVH2 frames walk in place.
    const uint32_t mode = s->inplace_shadow == 3u ? (p.small_tree ? 1u : 2u) : s->inplace_shadow;
    p.first_deferred = (p.instanced || p.env) ? 0u : (p.bvh2 || mode == 1u) ? s->max_depth : mode == 0u ? 0u : std::min(1u, s->max_depth);
    p.any_deferred = p.first_deferred < s->max_depth;
    p.defer_regions = s->max_depth - p.first_deferred;  // regions of the NEE queue and of the slot array
    p.folds = p.batched_paths || p.any_deferred || p.queue_fed;     // finished paths leave their radiance in d_lfinal, k_fold_paths adds it to the sum
    p.lanes4 = s->wave_samples >= 2u && !p.small_tree && !p.bvh2 && !fed;    // a launch of 4 k samples can put four in the lanes of a wave
    // More than one sample per chain only when nothing travels between launches (one path segment, shadow rays walked in place) or every
    // sample keeps its own path state and queue entries (ensure_batch_buffers); path ids are sample * n_local_pixels + pixel and must
    // stay below 2^31 (bit 31 tags queue entries).  1 M triangles, 4 segments: 1.78 / 1.61 / 1.50 / 1.45 ms per frame at 1 / 2 / 4 / 8.
    const uint64_t fit = s->n_local_pixels ? 0x7fffffffull / s->n_local_pixels : 8ull;
    const uint32_t by_paths = (uint32_t)std::min<uint64_t>(8ull, std::max<uint64_t>(1ull, fit));
    if (fed && !p.instanced) p.limit = (s->count_visits || p.bvh2) ? 1u : by_paths;     // queue-fed whatever the depth; counting and BVH2 frames one by one
    else if (p.first_deferred == 0u || (s->count_visits && !s->count_batched) || p.bvh2) p.limit = 1u;      // the batched first-segment builds walk their shadow rays in place
    else if (s->count_visits)       // counting in the timed form: exactly the launch of four samples in the lanes of a wave has a counting build
        p.limit = (s->wave_samples >= 2u && !p.small_tree && s->tri_min != 0u && s->lanes_per_ray >= 8u && fit >= 4ull) ? 4u : 1u;
    else p.limit = s->max_depth == 1u ? 8u : by_paths;
    // what must exist before the first launch, beside what reads it
    p.need_queues = p.queue_fed;                       // a one-segment flat scene holds none until its camera gets an aperture or the scene an environment
    p.need_lens_queue = fed && !p.instanced;           // segment 0 of such a frame reads d_rays_lens, which no later segment writes over
    p.need_lfinal = p.queue_fed || p.any_deferred;     // (with batched_paths, ensure_batch_buffers brings it): read where `folds`
    // d_qhits is read where pretraced(b), and by every instanced segment; allocated for this superset of those frames
    p.need_qhits = (s->bounce_refill && (s->max_depth > 1u || (fed && !p.instanced))) || p.instanced || p.env;
    p.need_qinst = p.instanced; p.need_visit_totals = s->count_visits;
    return p;
}

// d_lfinal for the samples the path buffers are sized for (frames that fold: several samples of multi-segment paths, deferred shadow rays)
int ensure_lfinal(crt_scene* s) {
    if (s->d_lfinal && s->lfinal_cap >= s->batch_cap) return CRT_OK;
    HIPCHK(hipStreamSynchronize(s->stream));
    if (s->d_lfinal) { (void)hipFree(s->d_lfinal); s->d_lfinal = nullptr; }
    const size_t n = (size_t)s->n_local_pixels * s->batch_cap;
    int rc = dev_alloc(&s->d_lfinal, n);
    if (rc) return rc;
    HIPCHK(hipMemset(s->d_lfinal, 0, n * sizeof(float4)));      // pixels outside the frame are never written: they stay zero
    s->lfinal_cap = s->batch_cap;
    return CRT_OK;
}

// The NEE queue and the contribution slots of `regions` deferring segments, for the samples per launch the path buffers are sized for
int ensure_defer_buffers(crt_scene* s, uint32_t regions) {
    if (regions == 0u) return CRT_OK;
    if (s->d_nee && s->defer_cap == s->batch_cap && s->defer_regions >= regions && s->defer_sub_capacity == s->sub_capacity) return CRT_OK;
    HIPCHK(hipStreamSynchronize(s->stream));
    for (void** p : {(void**)&s->d_nee, (void**)&s->d_contrib, (void**)&s->d_nee_perm}) { if (*p) (void)hipFree(*p); *p = nullptr; }
    s->defer_cap = s->defer_regions = 0;
    const uint64_t slots = (uint64_t)regions * s->n_local_pixels * s->batch_cap;
    if (slots >= (1ull << 32)) return fail(CRT_ERR_LIMIT, "deferred shadow rays: more than 2^32 contribution slots (segments x pixels x samples per launch); use inplace_shadow 1");
    int rc;
    if ((rc = dev_alloc(&s->d_nee, 2 * 8 * (size_t)s->sub_capacity * regions)) || (rc = dev_alloc(&s->d_contrib, (size_t)slots))) return rc;
    if ((uint64_t)8 * s->sub_capacity * regions >= (1ull << 32)) return fail(CRT_ERR_LIMIT, "deferred shadow rays: more than 2^32 queue entries; use inplace_shadow 1");
    if ((rc = dev_alloc(&s->d_nee_perm, 8 * (size_t)s->sub_capacity * regions))) return rc;
    if (!s->d_nee_bins) {
        if ((rc = dev_alloc(&s->d_nee_bins, 2 * 4096 + 9 * kCounterStride))) return rc;
        HIPCHK(hipMemset(s->d_nee_bins, 0, (2 * 4096 + 9 * kCounterStride) * sizeof(uint32_t)));
    }
    s->defer_cap = s->batch_cap; s->defer_regions = regions; s->defer_sub_capacity = s->sub_capacity;
    return CRT_OK;
}

// Path state, ray queues and the final-radiance buffer for `cap` samples per launch (multi-segment paths).  The per-group queue
// capacity grows with it, so the lazily allocated shadow queue / hit buffer are dropped and come back at the new size.
int ensure_batch_buffers(crt_scene* s, uint32_t cap) {
    if (s->batch_cap >= cap) return CRT_OK;
    HIPCHK(hipStreamSynchronize(s->stream));
    // The lazily allocated hit buffer and the deferred shadow rays' buffers follow the per-group capacity: dropped now (null pointers the
    // next frame re-allocates at the size then in force), whatever happens below.
    for (void** p : {(void**)&s->d_nee, (void**)&s->d_contrib, (void**)&s->d_nee_perm, (void**)&s->d_qhits}) { if (*p) (void)hipFree(*p); *p = nullptr; }
    s->defer_cap = s->defer_regions = 0;
    // Everything else is allocated at the new size FIRST and swapped in only when all of it exists: a failed growth (~250 B per
    // pixel and sample: 16 GB for a 4K frame at 8 samples) leaves the scene exactly as it was, able to render frame by frame.
    const size_t P = s->n_local_pixels;
    const uint32_t sub_capacity = (uint32_t)(((P + 4095) / 4096 + 7) / 8 * 4096) * cap;
    const size_t Q = 8 * (size_t)sub_capacity;
    float4 *rays0 = nullptr, *rays1 = nullptr, *L = nullptr, *T = nullptr, *lfinal = nullptr;
    float2* seed = nullptr;
    auto undo = [&](int code) {
        for (void* p : {(void*)rays0, (void*)rays1, (void*)L, (void*)T, (void*)seed, (void*)lfinal}) if (p) (void)hipFree(p);
        return code;
    };
    int rc;
    if (s->debug_fail_batch_alloc) { s->debug_fail_batch_alloc = 0; return fail(CRT_ERR_NOMEM, "hipMalloc: injected failure (debug_fail_batch_alloc)"); }
    if ((rc = dev_alloc(&rays0, 2 * Q)) || (rc = dev_alloc(&rays1, 2 * Q)) || (rc = dev_alloc(&L, P * cap)) || (rc = dev_alloc(&T, P * cap)) ||
        (rc = dev_alloc(&seed, P * cap)) || (rc = dev_alloc(&lfinal, P * cap)))
        return undo(rc);
    if (hipMemset(lfinal, 0, P * cap * sizeof(float4)) != hipSuccess)      // pixels outside the frame are never written: they stay zero
        return undo(fail(CRT_ERR_HIP, "hipMemset failed"));
    for (void* p : {(void*)s->d_rays[0], (void*)s->d_rays[1], (void*)s->pb.L, (void*)s->pb.T, (void*)s->pb.seed, (void*)s->d_lfinal}) if (p) (void)hipFree(p);
    s->d_rays[0] = rays0; s->d_rays[1] = rays1; s->pb.L = L; s->pb.T = T; s->pb.seed = seed; s->d_lfinal = lfinal;
    s->sub_capacity = sub_capacity;
    s->batch_cap = cap;
    s->lfinal_cap = cap;
    s->rays_doubled = false;
    if (s->d_bins) HIPCHK(hipMemset(s->d_bins, 0, crt_scene::bins_words() * sizeof(uint32_t)));     // new queues: the bins start empty-handed again
    return CRT_OK;
}

// Everything a chain of plan `p` needs ALLOCATED on this device, and nothing enqueued: a scene on several devices or streams prepares
// all of them before the first launch of any, so that an allocation failing on one leaves no device with half a batch in its sums.
int prepare_batch(crt_scene* s, const FramePlan& p, uint32_t n_samples) {
    HIPCHK(hipSetDevice(s->device));
    int rc = crt::ensure_frame(s);
    if (rc) return rc;
    if (s->n_local_pixels == 0) return CRT_OK;
    if (p.need_queues && !s->d_rays[0] && (rc = alloc_queues_and_paths(s))) return rc;
    if (p.batched_paths && (rc = ensure_batch_buffers(s, n_samples))) return rc;   // grows to the largest batch ever asked for
    if (p.need_lens_queue && (!s->d_rays_lens || s->lens_sub_capacity != s->sub_capacity)) {
        HIPCHK(hipStreamSynchronize(s->stream));
        if (s->d_rays_lens) { (void)hipFree(s->d_rays_lens); s->d_rays_lens = nullptr; }
        if ((rc = dev_alloc(&s->d_rays_lens, 2 * 8 * (size_t)s->sub_capacity))) return rc;
        s->lens_sub_capacity = s->sub_capacity;
    }
    if (p.need_lfinal && (rc = ensure_lfinal(s))) return rc;
    if ((rc = ensure_defer_buffers(s, p.defer_regions))) return rc;
    if (p.need_visit_totals && !s->d_visit_totals) {
        if ((rc = dev_alloc(&s->d_visit_totals, 16))) return rc;
        HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&s->h_visit_totals), 16 * sizeof(unsigned long long)));
    }
    if ((p.need_qhits || p.need_qinst) && (rc = crt::ensure_queue_hits(s, p.need_qhits, p.need_qinst))) return rc;
    if (p.bins && !s->d_bins) {
        if ((rc = dev_alloc(&s->d_bins, crt_scene::bins_words()))) return rc;
        HIPCHK(hipMemsetAsync(s->d_bins, 0, crt_scene::bins_words() * sizeof(uint32_t), s->stream));     // capacities 0: a first launch overflows entirely
    }
    if (p.bins && !s->rays_doubled) {
        // twice the entries any launch can emit: the bins' places in the first half, the overflow region — in the worst case every
        // ray of a launch, e.g. the first one after the view changed — in the second.  Between two frames the queues hold nothing.
        const uint32_t Qe = 8u * s->sub_capacity;
        HIPCHK(hipStreamSynchronize(s->stream));
        float4 *r0 = nullptr, *r1 = nullptr;
        if ((rc = dev_alloc(&r0, 4 * (size_t)Qe)) || (rc = dev_alloc(&r1, 4 * (size_t)Qe))) { if (r0) (void)hipFree(r0); return rc; }
        (void)hipFree(s->d_rays[0]); (void)hipFree(s->d_rays[1]);
        s->d_rays[0] = r0; s->d_rays[1] = r1;
        s->rays_doubled = true;
    }
    return CRT_OK;
}

// A launch whose kernel carries no events of its own (the instanced kernels, the ray generators, k_env_miss): a span of `kind` sits
// between two events recorded around it
template <typename F>
void timed(crt_scene* s, int kind, F&& enqueue) {
    EventSpan* sp = s->new_span(kind);
    if (sp) (void)hipEventRecord(sp->a, s->stream);
    enqueue();
    if (sp) (void)hipEventRecord(sp->b, s->stream);
}

// One chain of launches: what both renderers and their pieces share
struct Chain {
    FramePlan p;
    uint32_t n_samples; const float *rxs, *rys;      // and the randomVector of each sample
    crt::FrameArgs f;
    uint32_t* cnt;               // this chain's counter bank
    size_t n_paths;              // samples x local pixels
    bool measure_tiles;          // the fused first segment adds its waves' clock ticks to their tiles' counters
};

// Spans restart, the visit totals are zeroed, the counter banks alternate: the chain's first kernel clears the other bank for the next
// frame, so a memset is only needed for the very first frame (or after a failed launch left the banks in an unknown state)
int begin_chain(crt_scene* s, uint32_t** cnt) {
    if (!s->timing_accumulate) s->n_spans = 0;
    if (s->count_visits) HIPCHK(hipMemsetAsync(s->d_visit_totals, 0, 16 * sizeof(unsigned long long), s->stream));
    s->bank ^= 1u;
    if (!s->counts_clean) HIPCHK(hipMemsetAsync(s->d_counts, 0, 2 * kCounters * sizeof(uint32_t), s->stream));
    s->counts_clean = false;
    *cnt = s->counts();
    return CRT_OK;
}

int end_chain(crt_scene* s, uint32_t n_samples) {
    if (s->count_visits) HIPCHK(hipMemcpyAsync(s->h_visit_totals, s->d_visit_totals, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s->stream));
    s->stats_counted = s->count_visits;
    HIPCHK(hipGetLastError());
    s->counts_clean = s->stats_pending = true;
    s->stats_from_frame = true;   // ray counts come from h_counts at the next sync
    s->samples_in_stats = n_samples;
    return CRT_OK;
}

// segment 0's rays and path state from a ray generator: k_raygen_rays along the caller's rays, k_raygen_lens through a
// lens, else the pinhole's k_raygen
void launch_primary_rays(crt_scene* s, const Chain& c, float4* rays) {
    const crt::RaygenArgs ra = crt::raygen_args(s, c.f, rays, c.cnt + counter_index(0, 0, 0), true);
    if (c.p.rays) {
        crt::RaysRaygenArgs ca{};
        static_cast<crt::RaygenArgs&>(ca) = ra;
        ca.cam_rays = s->camera_rays_buffer(); ca.l_final = s->d_lfinal; ca.n_samples = c.n_samples;
        timed(s, 0, [&] { crt::launch_raygen_rays(ca, s->stream); });
        return;
    }
    if (!c.p.lens) { timed(s, 0, [&] { crt::launch_raygen(ra, s->stream); }); return; }
    crt::LensRaygenArgs la{};
    static_cast<crt::RaygenArgs&>(la) = ra;
    la.aperture = s->cam.aperture; la.focal_dist = s->cam.focal_dist; la.n_samples = c.n_samples;
    for (uint32_t k = 0; k < 8u; ++k) la.rv_s[k] = k < c.n_samples ? c.rxs[k] * c.rys[k] : 0.f;
    timed(s, 0, [&] { crt::launch_raygen_lens(la, s->stream); });
}

// The paths a segment's closest-hit walk found to miss take the environment's radiance through their slot of that segment (DESIGN.md
// §28): k_env_miss over segment b's queue, whose hits sit in d_qhits.  Option "timing" 2: a span of its own (inside the segment's span
// on a flat scene; crt_frame_stats counts it under ms_shade)
void launch_env_miss_of(crt_scene* s, const Chain& c, uint32_t b, const crt::SegmentArgs& sa) {
    if (b == 0 && (s->env_flags & CRT_ENV_HIDE_FROM_CAMERA)) return;
    crt::EnvMissArgs ea{};
    ea.rays = sa.rays_in; ea.count = sa.count_in; ea.hits = s->d_qhits; ea.sub_capacity = s->sub_capacity; ea.n_paths = (uint32_t)c.n_paths;
    ea.T = s->pb.T; ea.contrib = s->d_contrib; ea.slot_first = sa.slot_first; ea.slot_bit = sa.slot_bit;
    ea.texels = s->d_env; ea.size = s->env_size;
    for (int k = 0; k < 9; ++k) ea.rotation[k] = s->env_rotation[k];
    for (int k = 0; k < 3; ++k) ea.scale[k] = s->env_scale[k];
    timed(s, 3, [&] { crt::launch_env_miss(ea, s->stream); });
}

// cell coordinate of a point = clamp((p - origin) * scale, 0, cells - 1): the scene's bounds cut into `cells` per axis
void cell_grid(const crt_scene* s, float cells, float origin[3], float scale[3]) {
    for (int k = 0; k < 3; ++k) {
        const float ext = s->bounds_hi[k] - s->bounds_lo[k];
        origin[k] = s->bounds_lo[k];
        scale[k] = ext > 0.f ? cells / ext : 0.f;
    }
}

// What segment b's shading reads and writes on either kind of scene: the scene's tables, the segment's queues and counters, the path
// state, its region of the NEE queue and of the slot array where it defers, the samples' random vectors
void shading_args(const crt_scene* s, const Chain& c, uint32_t b, crt::SegmentArgs& sa) {
    const FramePlan& p = c.p;
    sa.triangles = s->d_triangles; sa.normals = s->d_normals; sa.materials = s->d_materials; sa.lights = s->d_lights; sa.n_lights = (int32_t)s->n_lights;
    sa.texcoords = s->d_texcoords; sa.textures = s->d_textures; sa.tex_width = s->tex_width; sa.tex_height = s->tex_height; sa.n_textures = s->n_textures;
    sa.f = c.f; sa.sub_capacity = s->sub_capacity;
    sa.rays_in = (p.need_lens_queue && b == 0) ? s->d_rays_lens : s->d_rays[b & 1]; sa.count_in = c.cnt + counter_index(b, 0, 0);
    sa.rays_next = s->d_rays[(b + 1) & 1]; sa.count_next = c.cnt + counter_index(b + 1, 0, 0);
    sa.count_shadow = c.cnt + counter_index(b, 1, 0);
    if (!p.inplace(b)) {
        const uint32_t r = b - p.first_deferred;         // this segment's region of the NEE queue and of the slot array
        sa.shadow = s->d_nee + 2 * (size_t)r * 8u * s->sub_capacity;
        sa.contrib = s->d_contrib + (size_t)r * c.n_paths;
        sa.slot_first = (uint32_t)((size_t)r * c.n_paths);
        sa.slot_bit = 1u << (8u + b);
    }
    sa.pb = s->pb; sa.sum = s->d_sum;
    sa.last_segment = (b + 1 == s->max_depth) ? 1u : 0u;
    sa.visit_totals = s->d_visit_totals; sa.overflow = s->d_overflow;
    sa.l_final = p.folds ? s->d_lfinal : nullptr;
    sa.n_samples = p.first(b) ? c.n_samples : 1u;
    for (uint32_t k = 0; k < 8u; ++k) sa.rv_s[k] = k < c.n_samples ? c.rxs[k] * c.rys[k] : 0.f;
}

// One frame of an instanced scene, buffers prepared: a ray generator, then per segment the two-level closest-hit walk
// over the segment's queue and the shade-only pass, then ONE two-level any-hit launch for every segment's shadow rays and the fold: the
// flat chain's bounce_refill 1 + inplace_shadow 0 sequence, segment 0 included.  The handle's live arrays are read HERE, at enqueue time.
int render_instanced_async(crt_scene* s, Chain& c) {
    if (s->lit) { const int rc = crt::ensure_light_table(s); if (rc) return rc; }      // lights that follow the instances
    crt::InstancesView v{};
    crt::instances_view(s->inst, &v);
    const uint32_t P = s->n_local_pixels;
    const bool masked = s->instance_masks != 0u;
    // a masked frame walks by the handle's TLAS child masks: renewed on the handle's stream if stale, this stream ordered behind that
    if (masked) { const int rc = crt::instances_child_masks_for(s->inst, s->stream, &s->cmask_seen); if (rc) return rc; }
    const int rc = begin_chain(s, &c.cnt);
    if (rc) return rc;
    launch_primary_rays(s, c, s->d_rays[0]);
    for (uint32_t b = 0; b < s->max_depth; ++b) {
        crt::InstSegmentArgs sa{};
        shading_args(s, c, b, sa);                  // region = segment: every segment defers
        const crt::InstMaskQueueArgs qa = crt::inst_queue_args(s, v, sa.rays_in, sa.count_in, b == 0 ? s->mask_primary : s->mask_bounce, s->d_visit_totals);
        timed(s, 1, [&] { crt::launch_closest_instances_queue(qa, s->count_visits, masked, s->stream); });
        if (c.p.env) launch_env_miss_of(s, c, b, sa);
        sa.stack_entries = 2;                       // the shade-only pass walks nothing
        sa.f.tile_order = nullptr;                  // storage order, as the ray generator's
        sa.hits_in = s->d_qhits;
        sa.hit_inst = s->d_qinst; sa.inst_w2o = v.w2o; sa.inst_mesh = v.mesh_of; sa.mesh_base = s->d_mesh_base;
        sa.light_first = s->lit ? s->lit->d_first : nullptr;
        timed(s, 3, [&] { crt::launch_segment_instanced(sa, s->count_visits, s->trace_grid(P, 5), s->waves_per_workgroup, s->stream); });
    }
    crt::InstMaskShadowArgs sh{};
    sh.nodes = v.nodes; sh.tris = v.tris; sh.inst = v.inst;
    if (masked) { sh.child_masks = v.child_masks; sh.n_tlas8 = v.tlas_nodes8; sh.ray_mask = s->mask_shadow; }
    sh.shadow = s->d_nee; sh.count = c.cnt + counter_index(0, 1, 0); sh.count_stride = counter_index(1, 1, 0) - counter_index(0, 1, 0);
    sh.contrib = s->d_contrib; sh.n_slots = (uint32_t)(c.n_paths * s->max_depth);
    sh.pools_per_region = (s->sub_capacity + 63u) / 64u; sh.n_regions = c.p.defer_regions;
    sh.sub_capacity = s->sub_capacity; sh.n_instances = v.n_instances; sh.stack_entries = v.stack_entries;
    sh.refill_min = 8; sh.tri_min = 2;
    sh.visit_totals = s->d_visit_totals ? s->d_visit_totals + 2 : nullptr; sh.overflow = s->d_overflow;
    timed(s, 2, [&] { crt::launch_shadow_instances_deferred(sh, s->count_visits, masked, s->stream); });
    crt::launch_fold_paths(s->d_sum, s->d_lfinal, s->d_contrib, P, 1u, 0u, s->stream);
    s->last_launch = LaunchInfo{0, (c.p.lens ? 16 : 0) | (c.p.env ? 32 : 0) | (c.p.rays ? 64 : 0), 1};
    return end_chain(s, 1u);
}

// Tile order of the fused first-segment kernels: adopts a finished measurement (most expensive first, dealt to the eight workgroup
// groups in snake order) and starts one if the view is new: *measure is set when this chain's first segment measures.
int adopt_tile_order(crt_scene* s, bool* measure) {
    if (!s->adaptive_tiles || s->n_local_tiles <= 1 || s->capturing) return CRT_OK;
    const bool arrived = s->tile_state == crt_scene::TILES_PENDING && hipEventQuery(s->ev_tile_cost) == hipSuccess;
    (void)hipGetLastError();                                    // "not ready" is an answer, not an error to report later
    if (arrived) {
        if (s->tile_order_uploading) HIPCHK(hipEventSynchronize(s->ev_tile_order));     // the pinned order buffer is free again
        const uint32_t nt = s->n_local_tiles;
        // Most expensive first.  A unit of work is 4096 pixels = spu tiles (1 for the default 64x64 tile); unit U belongs to
        // workgroup group U & 7 (one group per XCD, no rebalancing between them) and a group renders its units in order.
        // So group g's k-th tile sits in slot ((k / spu) * 8 + g) * spu + k % spu, and the sorted list is dealt to the
        // groups' k-th places in snake order — 0..7, 7..0, ... — which keeps the groups' sums level and every group's
        // own sequence descending.
        std::vector<uint32_t> sorted, row;
        try { sorted.resize(nt); row.reserve(8); } catch (const std::exception&) { return fail(CRT_ERR_NOMEM, "crt_render_frame: out of host memory (tile order)"); }
        for (uint32_t i = 0; i < nt; ++i) sorted[i] = i;
        const uint32_t* cost = s->h_tile_cost;
        std::sort(sorted.begin(), sorted.end(), [cost](uint32_t a, uint32_t b) { return cost[a] > cost[b] || (cost[a] == cost[b] && a < b); });
        const uint32_t tile_px = s->tile * s->tile, spu = tile_px < 4096u && 4096u % tile_px == 0u ? 4096u / tile_px : 1u;
        // how far the expensive tiles stand above the rest (99th percentile over mean): what wave_samples = 2 decides on
        uint64_t cost_sum = 0;
        for (uint32_t i = 0; i < nt; ++i) cost_sum += cost[i];
        s->tile_cost_spread = cost_sum ? (float)((double)cost[sorted[nt / 100u]] * nt / (double)cost_sum) : 0.f;
        uint32_t next = 0;
        for (uint32_t k = 0; next < nt; ++k) {
            row.clear();
            for (uint32_t g = 0; g < 8u; ++g) {
                const uint64_t slot = ((uint64_t)(k / spu) * 8u + g) * spu + k % spu;
                if (slot < nt) row.push_back((uint32_t)slot);
            }
            if (k & 1u) std::reverse(row.begin(), row.end());
            for (uint32_t slot : row) s->h_tile_order[slot] = sorted[next++];
        }
        HIPCHK(hipMemcpyAsync(s->d_tile_order, s->h_tile_order, nt * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream));
        HIPCHK(hipEventRecord(s->ev_tile_order, s->stream));
        s->tile_order_uploading = true;
        s->tile_state = crt_scene::TILES_DONE;
    }
    ++s->frames_since_tile_measure;
    // a camera that moves every frame would otherwise sort the tiles on the host every frame: at most one measurement per 16
    // frames (the first one at once); the counting kernels have another cost profile (measured: a worse order) and do not measure
    if (s->tile_state == crt_scene::TILES_WANT && !s->count_visits && (!s->tiles_measured_once || s->frames_since_tile_measure >= 16u)) {
        s->tiles_measured_once = true;
        s->frames_since_tile_measure = 0;
        HIPCHK(hipMemsetAsync(s->d_tile_cost, 0, s->n_local_tiles * sizeof(uint32_t), s->stream));
        *measure = true;
    }
    return CRT_OK;
}

// k_segment's arguments for segment b of a flat scene's chain: what it walks, the bins it reads and fills, its sample form and build
crt::SegmentArgs segment_args(crt_scene* s, const Chain& c, uint32_t b) {
    const FramePlan& p = c.p;
    const bool first = p.first(b);
    crt::SegmentArgs sa{};
    shading_args(s, c, b, sa);
    sa.nodes = s->d_nodes; sa.planes = s->d_planes; sa.tris = s->d_tris; sa.stack_entries = s->stack_entries;
    sa.tri_min = p.small_tree ? 0u : s->tri_min;
    sa.lanes_log2 = s->lanes_per_ray >= 8u ? 3u : s->lanes_per_ray >= 4u ? 2u : s->lanes_per_ray >= 2u ? 1u : 0u;
    sa.nodes2 = s->d_bvh2; sa.tris2 = s->d_tris2; sa.stack_entries2 = s->bvh2_stack; sa.tie = s->accel == 2u ? 1u : 0u;
    const uint32_t Qe = 8u * s->sub_capacity;        // entries of the bins' half of a queue = what the sub-queue form holds
    if (p.bins && b + 1 < s->max_depth) {            // tables and the queues' overflow halves exist (prepare_batch)
        crt::RayBins& o = sa.bins_out;
        o.count = s->bin_count(b + 1); o.cap = s->bin_cap(s->bank, b + 1); o.off = s->bin_off(s->bank, b + 1);
        o.ovf_count = s->bin_ovf(b + 1); o.ovf_base = Qe;
        // option "ray_bins": 1 ballots, 2 per-ray atomics, 3 ballots for the first segment's emission and per-ray atomics after, 4 ranking
        // through LDS, 5 ballots for the first segment's emission (a handful of keys per wave) and LDS ranking after
        o.per_lane = s->ray_bins == 2u ? 1u : s->ray_bins == 3u ? (b > 0 ? 1u : 0u) : s->ray_bins == 4u ? 2u : s->ray_bins == 5u ? (b > 0 ? 2u : 0u) : 0u;
        cell_grid(s, 8.0f, o.origin, o.scale);
    }
    if (p.bins && b > 0) { sa.bin_start = s->bin_start(b); sa.bin_off_in = s->bin_off(s->bank, b); sa.ovf_base_in = Qe; }
    if (first) { sa.zero_counts = s->d_counts + (size_t)(s->bank ^ 1u) * kCounters; sa.n_zero = kCounters; }
    sa.tile_cost = (first && c.measure_tiles) ? s->d_tile_cost : nullptr;
    // how the samples of a batched launch sit on the hardware (option "wave_samples"): 2 = four samples of a 4 x 4 pixel quadrant in
    // the lanes of one wave — the 64 rays of a wave leave a quarter of the area and agree on their nodes like the rays of a frame of
    // twice the resolution (1 M triangles, 1080p: +8.5 % at 4 samples per launch, +12 % at 8; shards gain as well; trees of a few
    // nodes lose 9 %: more, shorter waves) —, 1 = the samples on the waves of a workgroup, 0 = one after the other in each wave
    sa.wave_samples = 0u;
    if (first && c.n_samples > 1u) {
        if (p.lanes4 && (c.n_samples & 3u) == 0u) sa.wave_samples = 2u;
        else if (s->wave_samples != 3u && s->use_wave_samples()) sa.wave_samples = 1u;
    }
    // the first segment's 6-wave build where the launch is bound by throughput, the 5-wave build where its longest waves set its length
    // (with four samples in the lanes of a wave a launch has four times the waves, each a quarter as long, and the measure above —
    // made for samples that follow each other in a wave — flips too early: the 6-wave build wins down to about a million pixels,
    // i.e. while the launch fills the chip's 6,144 wave slots eight times over; an eighth of the 4K frame 0.405 -> 0.396 ms, half a
    // 1080p frame 0.435 -> 0.421, a quarter 0.225 against 0.231 the other way)
    bool wide_auto = !s->bound_by_longest_waves();
    if (sa.wave_samples == 2u)
        wide_auto = (double)(s->n_local_pixels / 16u) * (double)(c.n_samples / 4u) >= 8.0 * (double)s->n_cu * 4.0 * 6.0;
    sa.wide_first = (first && (s->wide_first == 2u ? wide_auto : s->wide_first != 0u)) ? 1u : 0u;
    sa.last_build = s->last_build;
    return sa;
}

// Segment b of a flat scene's chain: where the plan says so its closest hits through k_closest_queue (and k_env_miss for the paths that
// missed), then k_segment in the build launch_segment picks, then the scan of the bins it filled
void launch_flat_segment(crt_scene* s, const Chain& c, uint32_t b) {
    const FramePlan& p = c.p;
    const bool first = p.first(b), pretraced = p.pretraced(b);
    crt::SegmentArgs sa = segment_args(s, c, b);
    EventSpan* sp = s->new_span(1);
    if (pretraced) {
        crt::QueueTraceArgs qa{};
        qa.nodes = s->d_nodes; qa.tris = s->d_tris; qa.rays = sa.rays_in; qa.count = sa.count_in; qa.hits = s->d_qhits;
        qa.stack_entries = s->stack_entries; qa.sub_capacity = s->sub_capacity; qa.refill_min = s->refill_min; qa.tri_min = s->tri_min ? s->tri_min : 1u;      // (0 only on an environment frame: the pools vote, as k_shadow_deferred's do)
        qa.pool = s->refill_pool; qa.lanes_log2 = sa.lanes_log2;
        qa.persistent = s->persistent; qa.cursors = c.cnt + cursor_index_closest(b);
        qa.visit_totals = s->d_visit_totals; qa.overflow = s->d_overflow;
        if (sp) crt::set_launch_events(sp->a, nullptr);                 // span = both launches of the segment
        crt::launch_closest_queue(qa, s->count_visits, s->persistent ? s->resident_waves(s->pool_lds(), 8) : 8u * ((s->sub_capacity + qa.pool - 1u) / qa.pool), s->stream);
        sa.hits_in = s->d_qhits;
        if (p.env) launch_env_miss_of(s, c, b, sa);
        if (sp) crt::set_launch_events(nullptr, sp->b);
    } else if (sp) crt::set_launch_events(sp->a, sp->b);
    // A workgroup renders ONE chunk (CRT_CHUNK_LOOP), so the grid has to cover every chunk a sub-queue can hold: a group's
    // sub-queue gets the rays of that group's units of 4096 pixels — ceil(units / 8) of them — times the samples of the launch.
    // (P * n_samples spread evenly over the 8 groups is fewer chunks than that when the units do not divide by 8.)
    uint32_t grid = s->trace_grid(s->n_local_pixels, sa.wide_first ? 6 : 5);
    if (!first && p.batched_paths) grid *= c.n_samples;
    const int build = crt::launch_segment(sa, first, pretraced, p.inplace(b), p.bvh2, s->special_materials, s->count_visits, s->lean_build != 0u && s->tree_validated, grid, s->waves_per_workgroup, s->stream);
    if (b == 0) s->last_launch = LaunchInfo{(int)sa.wave_samples, (build & 15) | (p.lens ? 16 : 0) | (p.env ? 32 : 0) | (p.rays ? 64 : 0), (int)c.n_samples};
    if (sa.bins_out.count) {
        // fill counts -> the next launch's index space and ray count, and the next frame's capacities (the other parity)
        crt::BinScanArgs ba{};
        ba.count = s->bin_count(b + 1); ba.cap = s->bin_cap(s->bank, b + 1); ba.start = s->bin_start(b + 1); ba.ovf_count = s->bin_ovf(b + 1);
        ba.n_in = c.cnt + counter_index(b + 1, 0, 0);
        ba.cap_next = s->bin_cap(s->bank ^ 1u, b + 1); ba.off_next = s->bin_off(s->bank ^ 1u, b + 1);
        ba.queue_entries = 8u * s->sub_capacity;
        crt::launch_bin_scan(ba, s->stream);
    }
}

// ONE any-hit launch for the shadow rays of every deferring segment: full waves from the first step
void launch_deferred_shadows(crt_scene* s, const Chain& c) {
    crt::ShadowArgs sh{};
    sh.nodes = s->d_nodes; sh.tris = s->d_tris; sh.shadow = s->d_nee; sh.contrib = s->d_contrib;
    sh.count = c.cnt + counter_index(c.p.first_deferred, 1, 0); sh.count_stride = counter_index(1, 1, 0) - counter_index(0, 1, 0);
    sh.stack_entries = s->stack_entries; sh.sub_capacity = s->sub_capacity;
    sh.pool = s->shadow_pool; sh.refill_min = s->shadow_refill_min; sh.tri_min = s->tri_min ? s->tri_min : 1u;
    sh.lanes_log2 = s->lanes_per_ray >= 8u ? 3u : 0u;
    sh.pools_per_region = (s->sub_capacity + sh.pool - 1u) / sh.pool;
    sh.persistent = s->persistent; sh.n_regions = c.p.defer_regions; sh.cursors = c.cnt + kCursorShadow;
    if (s->sort_shadow && !c.p.small_tree) {
        // sorted by the cell the rays start in: three small launches (histogram, scan, scatter), then a persistent grid over the sorted order
        crt::NeeSortArgs na{};
        na.shadow = s->d_nee; na.count = sh.count; na.count_stride = sh.count_stride; na.sub_capacity = s->sub_capacity; na.n_queues = sh.n_regions * 8u;
        cell_grid(s, 16.0f, na.origin, na.scale);
        na.hist = s->d_nee_bins; na.cursor = s->d_nee_bins + 4096; na.perm = s->d_nee_perm; na.meta = s->d_nee_bins + 2 * 4096;
        crt::launch_nee_sort(na, (uint32_t)s->n_cu * 2u, s->stream);
        sh.perm = s->d_nee_perm; sh.sort_meta = na.meta; sh.persistent = 1u;
    }
    sh.visit_totals = s->d_visit_totals ? s->d_visit_totals + 2 : nullptr;
    sh.overflow = s->d_overflow;
    EventSpan* sp = s->new_span(2);
    if (sp) crt::set_launch_events(sp->a, sp->b);
    crt::launch_shadow_deferred(sh, s->count_visits, sh.persistent ? s->resident_waves(s->pool_lds(), s->shadow_waves) : 8u * sh.n_regions * sh.pools_per_region, s->stream);
}

// One chain of a flat scene, buffers prepared: [ray generator ->] per segment [closest, env miss,] k_segment [, bin scan] -> deferred
// shadow rays -> fold.  n_samples > 1: the same chain renders that many samples of every pixel — what n_samples calls would do, bit
// for bit, without their launch gaps and kernel tails.
int render_flat_async(crt_scene* s, Chain& c) {
    const FramePlan& p = c.p;
    int rc;
    // a frame through a lens, along the caller's rays or with an environment leaves the tile order and its measurement as they are
    if (!p.queue_fed && (rc = adopt_tile_order(s, &c.measure_tiles))) return rc;
    if (!p.bvh2 && (rc = crt::ensure_planes(s))) return rc;
    if ((rc = begin_chain(s, &c.cnt))) return rc;
    if (p.queue_fed) launch_primary_rays(s, c, p.need_lens_queue ? s->d_rays_lens : s->d_rays[0]);
    for (uint32_t b = 0; b < s->max_depth; ++b) launch_flat_segment(s, c, b);
    if (p.any_deferred) launch_deferred_shadows(s, c);
    if (p.folds) crt::launch_fold_paths(s->d_sum, s->d_lfinal, p.any_deferred ? s->d_contrib : nullptr, s->n_local_pixels, c.n_samples, p.first_deferred, s->stream);
    if (c.measure_tiles) {
        HIPCHK(hipMemcpyAsync(s->h_tile_cost, s->d_tile_cost, s->n_local_tiles * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
        HIPCHK(hipEventRecord(s->ev_tile_cost, s->stream));
        s->tile_state = crt_scene::TILES_PENDING;
    }
    return end_chain(s, c.n_samples);
}

int render_batch_async(crt_scene* s, uint32_t n_samples, const float* rxs, const float* rys) {
    if (!s->have_camera && !s->camera_rays()) return fail(CRT_ERR_INVALID, "crt_render_frame: crt_set_camera was never called");      // (the caller's rays need no camera)
    Chain c{plan_frame(s, n_samples), n_samples, rxs, rys, {}, nullptr, 0, false};
    const int rc = prepare_batch(s, c.p, n_samples);          // sets the device; a no-op when render_batch_all has prepared every device already
    if (rc) return rc;
    if (s->n_local_pixels == 0) return CRT_OK;
    c.f = crt::frame_args(s, rxs[0], rys[0]);
    c.n_paths = (size_t)s->n_local_pixels * n_samples;
    s->stats_seg0_counted = c.p.rays;       // entries without a path emit no ray: segment 0's count comes from its queue counters
    return c.p.instanced ? render_instanced_async(s, c) : render_flat_async(s, c);      // an instanced chain is one sample (FramePlan::limit)
}

// one batch on every device of the scene: each enqueues on its own stream and returns, so the devices render concurrently
int render_batch_all(crt_scene* s, uint32_t n_samples, const float* rxs, const float* rys) {
    int rc = CRT_OK;
    if (!s->peers.empty()) {
        // phase 1: every device's buffers for this batch exist before any device renders (a failed growth leaves every sum as it was)
        if (!s->have_camera && !s->camera_rays()) return fail(CRT_ERR_INVALID, "crt_render_frame: crt_set_camera was never called");      // (the caller's rays need no camera)
        if ((rc = prepare_batch(s, plan_frame(s, n_samples), n_samples))) { (void)hipSetDevice(s->device); return rc; }
        for (crt_scene* p : s->peers) if ((rc = prepare_batch(p, plan_frame(p, n_samples), n_samples))) { (void)hipSetDevice(s->device); return rc; }
    }
    // phase 2: enqueue everywhere
    rc = render_batch_async(s, n_samples, rxs, rys);
    for (size_t k = 0; !rc && k < s->peers.size(); ++k) rc = render_batch_async(s->peers[k], n_samples, rxs, rys);
    if (!s->peers.empty()) (void)hipSetDevice(s->device);      // the caller's thread keeps the device the scene lives on
    return rc;
}

int collect_stats(crt_scene* s) {
    if (!s->stats_pending) return CRT_OK;
    HIPCHK(hipStreamSynchronize(s->stream));
    crt_frame_stats st{};
    for (int i = 0; i < s->n_spans; ++i) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, s->spans[i].a, s->spans[i].b) != hipSuccess) continue;
        switch (s->spans[i].kind) {
            case 0: st.ms_raygen += ms; break;
            case 1: st.ms_trace_closest += ms; st.n_trace_launches++; break;
            case 2: st.ms_trace_any += ms; st.n_trace_launches++; break;
            default: st.ms_shade += ms; break;
        }
    }
    if (s->n_spans > 0) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, s->spans[0].a, s->spans[s->n_spans - 1].b) == hipSuccess) st.ms_total = ms;
    }
    st.closest_rays = s->stats.closest_rays;
    st.any_rays = s->stats.any_rays;
    if (s->stats_from_frame && s->stats_counted && s->h_visit_totals) {
        st.nodes_closest = s->h_visit_totals[0]; st.tris_closest = s->h_visit_totals[1];
        st.nodes_any = s->h_visit_totals[2]; st.tris_any = s->h_visit_totals[3];
        st.wave_steps_closest_nodes = s->h_visit_totals[4]; st.wave_steps_closest_tris = s->h_visit_totals[5];
        st.wave_steps_any_nodes = s->h_visit_totals[6]; st.wave_steps_any_tris = s->h_visit_totals[7];
        st.closest_hits = s->h_visit_totals[8];
        st.nodes_closest_uniform = s->h_visit_totals[10]; st.nodes_any_uniform = s->h_visit_totals[11];
    }
    s->stats = st;
    s->stats_pending = false;
    return CRT_OK;
}

}  // namespace

extern "C" {

int crt_render_frame_async(crt_scene* s, float rx, float ry) {
    if (!s) return fail(CRT_ERR_INVALID, "crt_render_frame: null scene");
    return render_batch_all(s, 1u, &rx, &ry);
}

int crt_render_frames_async(crt_scene* s, uint32_t n, const float* rx, const float* ry) {
    if (!s) return fail(CRT_ERR_INVALID, "crt_render_frames: null scene");
    if (n && (!rx || !ry)) return fail(CRT_ERR_INVALID, "crt_render_frames: null argument");
    const FramePlan p = plan_frame(s, 1u);
    for (uint32_t i = 0; i < n;) {
        uint32_t k = std::min(p.limit, n - i);
        if (p.lanes4 && k > 4u && (k & 3u)) k &= ~3u;                    // 7 frames = 4 + 3, not 7 one after the other
        if (s->count_visits && k != 4u) k = 1u;                          // counting launches: four samples in the lanes form, or one
        const int rc = render_batch_all(s, k, rx + i, ry + i);
        if (rc) return rc;
        i += k;
    }
    return CRT_OK;
}

int crt_render_frames(crt_scene* s, uint32_t n, const float* rx, const float* ry) {
    const int rc = crt_render_frames_async(s, n, rx, ry);
    return rc ? rc : crt_sync(s);
}

int crt_sync(crt_scene* s) {
    if (!s) return fail(CRT_ERR_INVALID, "crt_sync: null scene");
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipStreamSynchronize(s->stream));
    HIPCHK(hipGetLastError());
    for (crt_scene* p : s->peers) { const int rc = crt_sync(p); if (rc) return rc; }
    if (!s->peers.empty()) HIPCHK(hipSetDevice(s->device));
    return CRT_OK;
}

int crt_render_frame(crt_scene* s, float rx, float ry) {
    const int rc = crt_render_frame_async(s, rx, ry);
    return rc ? rc : crt_sync(s);
}

int crt_get_frame_stats(crt_scene* s, crt_frame_stats* out) {
    if (!s || !out) return fail(CRT_ERR_INVALID, "crt_get_frame_stats: null argument");
    HIPCHK(hipSetDevice(s->device));
    if (s->stats_pending) {
        HIPCHK(hipStreamSynchronize(s->stream));
        if (s->stats_from_frame) {
            // the queue counters stay valid until the next frame's memset: fetch them only when asked
            if (!s->h_counts && hipHostMalloc(reinterpret_cast<void**>(&s->h_counts), kCounters * sizeof(uint32_t)) != hipSuccess)
                return fail(CRT_ERR_NOMEM, "hipHostMalloc failed");
            HIPCHK(hipMemcpy(s->h_counts, s->counts(), kCounters * sizeof(uint32_t), hipMemcpyDeviceToHost));
            uint64_t any = 0, closest = s->stats_seg0_counted ? 0u : (uint64_t)s->n_local_in_frame * s->samples_in_stats;   // segment 0: one primary ray per in-frame pixel and sample (the caller's rays: those that have a path)
            for (uint32_t b = 0; b < s->max_depth; ++b)
                for (uint32_t g = 0; g < 8; ++g) {
                    if (b || s->stats_seg0_counted) closest += s->h_counts[counter_index(b, 0, g)];
                    any += s->h_counts[counter_index(b, 1, g)];
                }
            s->stats.closest_rays = closest; s->stats.any_rays = any;
        }
        int rc = collect_stats(s);
        if (rc) return rc;
        HIPCHK(hipMemcpy(&s->stats.stack_overflows, s->d_overflow, sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    *out = s->stats;
    // several devices: ray and visit counts are sums over the devices, times the slowest device's (they run side by side)
    for (crt_scene* p : s->peers) {
        crt_frame_stats ps{};
        const int rc = crt_get_frame_stats(p, &ps);
        if (rc) return rc;
        out->closest_rays += ps.closest_rays; out->any_rays += ps.any_rays;
        out->nodes_closest += ps.nodes_closest; out->tris_closest += ps.tris_closest; out->nodes_any += ps.nodes_any; out->tris_any += ps.tris_any;
        out->wave_steps_closest_nodes += ps.wave_steps_closest_nodes; out->wave_steps_closest_tris += ps.wave_steps_closest_tris;
        out->wave_steps_any_nodes += ps.wave_steps_any_nodes; out->wave_steps_any_tris += ps.wave_steps_any_tris;
        out->closest_hits += ps.closest_hits; out->stack_overflows += ps.stack_overflows;
        out->nodes_closest_uniform += ps.nodes_closest_uniform; out->nodes_any_uniform += ps.nodes_any_uniform;
        out->ms_total = std::max(out->ms_total, ps.ms_total); out->ms_trace_closest = std::max(out->ms_trace_closest, ps.ms_trace_closest);
        out->ms_trace_any = std::max(out->ms_trace_any, ps.ms_trace_any); out->ms_shade = std::max(out->ms_shade, ps.ms_shade);
    }
    if (!s->peers.empty()) HIPCHK(hipSetDevice(s->device));
    return CRT_OK;
}

int crt_get_launch_times(crt_scene* s, float* ms, size_t cap, size_t* n_out) {
    if (!s || !n_out) return fail(CRT_ERR_INVALID, "crt_get_launch_times: null argument");
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipStreamSynchronize(s->stream));
    size_t n = 0;
    for (int i = 0; i < s->n_spans; ++i) {
        float t = 0.f;
        if (hipEventElapsedTime(&t, s->spans[i].a, s->spans[i].b) != hipSuccess) continue;
        if (ms && n < cap) ms[n] = t;
        ++n;
    }
    *n_out = n;
    return CRT_OK;
}

int crt_debug_launch_form(crt_scene* s, int32_t* form) {
    if (!s || !form) return fail(CRT_ERR_INVALID, "crt_debug_launch_form: null argument");
    *form = s->last_launch.form;
    return CRT_OK;
}

int crt_debug_launch_info(crt_scene* s, int32_t info[4]) {
    if (!s || !info) return fail(CRT_ERR_INVALID, "crt_debug_launch_info: null argument");
    info[0] = s->last_launch.form; info[1] = s->last_launch.build; info[2] = s->last_launch.samples; info[3] = (int32_t)s->peers.size() + 1;
    return CRT_OK;
}

int crt_debug_time_graph(crt_scene* s, uint32_t n_frames, const float* rxy, uint32_t reps, float* ms_stream, float* ms_graph) {
    if (!s || !rxy || !ms_stream || !ms_graph || n_frames == 0 || (n_frames & 1u) || reps == 0)
        return fail(CRT_ERR_INVALID, "crt_debug_time_graph: bad argument (n_frames must be even: the counter banks alternate)");
    if (s->inst) return fail(CRT_ERR_INVALID, "crt_debug_time_graph: not offered for an instanced scene");
    if (!s->peers.empty() || s->primary)
        return fail(CRT_ERR_INVALID, "crt_debug_time_graph: one stream only (option streams 1, no crt_set_devices): the capture records this scene's stream, not its peers'");
    HIPCHK(hipSetDevice(s->device));
    const uint32_t timing0 = s->timing;
    s->timing = 0;                                         // event-carrying launches are not capturable
    int rc = crt_render_frame(s, rxy[0], rxy[1]);          // allocates, clears the counter banks once
    if (!rc) rc = crt_render_frame(s, rxy[0], rxy[1]);
    if (rc) { s->timing = timing0; return rc; }
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr;
    auto done = [&](int code) {
        if (exec) (void)hipGraphExecDestroy(exec);
        if (graph) (void)hipGraphDestroy(graph);
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        s->timing = timing0;
        return code;
    };
#define G_CHK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return done(fail(CRT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_))); } while (0)
    G_CHK(hipEventCreate(&e0));
    G_CHK(hipEventCreate(&e1));
    G_CHK(hipEventRecord(e0, s->stream));
    for (uint32_t r = 0; r < reps; ++r)
        for (uint32_t f = 0; f < n_frames; ++f)
            if ((rc = crt_render_frame_async(s, rxy[2 * f], rxy[2 * f + 1]))) return done(rc);
    G_CHK(hipEventRecord(e1, s->stream));
    G_CHK(hipStreamSynchronize(s->stream));
    float ms = 0.f;
    G_CHK(hipEventElapsedTime(&ms, e0, e1));
    *ms_stream = ms / (float)(reps * n_frames);
    G_CHK(hipStreamBeginCapture(s->stream, hipStreamCaptureModeThreadLocal));
    s->capturing = true;
    for (uint32_t f = 0; f < n_frames; ++f)
        if ((rc = crt_render_frame_async(s, rxy[2 * f], rxy[2 * f + 1]))) { s->capturing = false; (void)hipStreamEndCapture(s->stream, &graph); return done(rc); }
    s->capturing = false;
    G_CHK(hipStreamEndCapture(s->stream, &graph));
    G_CHK(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
    G_CHK(hipGraphLaunch(exec, s->stream));                // warm
    G_CHK(hipStreamSynchronize(s->stream));
    G_CHK(hipEventRecord(e0, s->stream));
    for (uint32_t r = 0; r < reps; ++r) G_CHK(hipGraphLaunch(exec, s->stream));
    G_CHK(hipEventRecord(e1, s->stream));
    G_CHK(hipStreamSynchronize(s->stream));
    G_CHK(hipEventElapsedTime(&ms, e0, e1));
    *ms_graph = ms / (float)(reps * n_frames);
#undef G_CHK
    return done(CRT_OK);
}

// Debug/test hook: copy out one of the frame's ray queues as left by the last crt_render_frame.
// which: 0/1 = path-ray queue written for an even/odd segment, 2 = shadow-ray queue of the last segment.
int crt_debug_read_queue(crt_scene* s, int which, uint32_t segment, crt_ray* dst, size_t cap, size_t* n_out) {
    if (!s || !n_out) return fail(CRT_ERR_INVALID, "crt_debug_read_queue: null argument");
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipStreamSynchronize(s->stream));
    if (!s->frame_buffers_ready || segment > 16) return fail(CRT_ERR_INVALID, "crt_debug_read_queue: no frame rendered");
    std::vector<uint32_t> counts(kCounters);
    HIPCHK(hipMemcpy(counts.data(), s->counts(), kCounters * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (which != 2 && s->d_bins && s->ray_bins) return fail(CRT_ERR_INVALID, "crt_debug_read_queue: the path-ray queue is binned (option ray_bins 0 gives the sub-queue form this reads)");
    const FramePlan p = plan_frame(s, 1u);
    const float4* src = which == 2 ? ((s->d_nee && segment >= p.first_deferred && segment - p.first_deferred < s->defer_regions) ? s->d_nee + 2 * (size_t)(segment - p.first_deferred) * 8u * s->sub_capacity : nullptr)
                                   : (segment == 0 && p.need_lens_queue) ? s->d_rays_lens : s->d_rays[segment & 1];      // a lens frame's primary rays keep a queue of their own
    if (!src) return fail(CRT_ERR_INVALID, "crt_debug_read_queue: that queue does not exist (shadow rays: only of segments that defer them, inplace_shadow 0 / 2; path queues: max_depth > 1)");
    const size_t entry = sizeof(crt_ray);        // a deferred shadow ray is (o, tmax) (d, contribution slot)
    size_t total = 0;
    for (uint32_t g = 0; g < 8; ++g) total += counts[counter_index(segment, which == 2 ? 1 : 0, g)];
    *n_out = total;
    if (dst) {
        size_t done = 0;
        for (uint32_t g = 0; g < 8 && done < cap; ++g) {
            size_t n = counts[counter_index(segment, which == 2 ? 1 : 0, g)];
            n = std::min(n, cap - done);
            if (!n) continue;
            const char* from = reinterpret_cast<const char*>(src) + (size_t)g * s->sub_capacity * entry;
            HIPCHK(hipMemcpy2D(dst + done, sizeof(crt_ray), from, entry, sizeof(crt_ray), n, hipMemcpyDeviceToHost));
            done += n;
        }
    }
    return CRT_OK;
}

}  // extern "C"
