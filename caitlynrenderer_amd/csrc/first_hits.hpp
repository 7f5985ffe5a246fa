// The first hits of the scene's current view into buffers that belong to a stage (ambient occlusion; fog, §33):
// crt_render_aov's launches with another destination, so crt_render_aov's own channels keep their bytes.  `out` names the destination of
// every channel in `channels`; `st` is what the launches need beside it (crt_scene.hpp), kept by the stage from call to call.
#pragma once
#include <exception>
#include <string>
#include <vector>

#include "crt_scene.hpp"
#include "instances.hpp"

namespace crt {

inline int enqueue_first_hits(crt_scene* s, const AovOut& out, uint32_t channels, FirstHitWork* st, const char* who, float rx, float ry, uint32_t n_pixels) {
    int rc;
    if (s->inst) {
        if ((rc = ensure_frame(s))) return rc;
        if ((rc = ensure_queue_hits(s, true, true))) return rc;
        if (!st->d_count && (rc = dev_alloc(&st->d_count, 8 * kCounterStride))) return rc;
    } else if (!st->d_tile_xy || st->tile != s->tile) {
        std::vector<uint2> tiles;
        try { deal_tiles(s->width, s->height, s->tile, 0u, 1u, tiles, nullptr); }
        catch (const std::exception&) { return fail(CRT_ERR_NOMEM, std::string(who) + ": out of host memory (tile list)"); }
        const uint64_t px = (uint64_t)tiles.size() * s->tile * s->tile;
        if (px >= (1ull << 31)) return fail(CRT_ERR_LIMIT, std::string(who) + ": frame too large for 32-bit pixel indices");
        HIPCHK(hipStreamSynchronize(s->stream));                          // an earlier call may still read the old list
        if (st->d_tile_xy) { (void)hipFree(st->d_tile_xy); st->d_tile_xy = nullptr; }
        if ((rc = dev_alloc(&st->d_tile_xy, tiles.size()))) return rc;
        if (!tiles.empty()) HIPCHK(hipMemcpy(st->d_tile_xy, tiles.data(), tiles.size() * sizeof(uint2), hipMemcpyHostToDevice));
        st->n_local_pixels = (uint32_t)px; st->tile = s->tile;
    }
    launch_aov_fill(out, channels, n_pixels, s->stream);
    if (s->inst) {
        if (s->n_local_pixels) {
            InstancesView v{};
            instances_view(s->inst, &v);
            const bool masked = s->instance_masks != 0u;
            if (masked && (rc = instances_child_masks_for(s->inst, s->stream, &s->cmask_seen))) return rc;
            HIPCHK(hipMemsetAsync(st->d_count, 0, 8 * kCounterStride * sizeof(uint32_t), s->stream));
            const RaygenArgs ra = raygen_args(s, frame_args(s, rx, ry), s->d_rays[0], st->d_count, false);
            launch_raygen(ra, s->stream);
            launch_closest_instances_queue(inst_queue_args(s, v, s->d_rays[0], st->d_count, s->mask_primary, nullptr), false, masked, s->stream);
            InstAovArgs a{};
            a.triangles = s->d_triangles; a.normals = s->d_normals; a.materials = s->d_materials;
            a.texcoords = s->d_texcoords; a.textures = s->d_textures;
            a.tex_width = s->tex_width; a.tex_height = s->tex_height; a.n_textures = s->n_textures;
            a.f = ra.f;
            a.sub_capacity = s->sub_capacity;
            a.rays_in = s->d_rays[0]; a.count_in = st->d_count; a.hits_in = s->d_qhits;
            a.hit_inst = s->d_qinst; a.inst_w2o = v.w2o; a.inst_mesh = v.mesh_of; a.mesh_base = s->d_mesh_base;
            a.channels = channels; a.out = out;
            launch_aov_instanced(a, s->stream);
        }
    } else if (st->n_local_pixels) {
        AovArgs a{};
        a.nodes = s->d_nodes; a.tris = s->d_tris; a.triangles = s->d_triangles; a.normals = s->d_normals; a.materials = s->d_materials;
        a.stack_entries = s->stack_entries;
        a.texcoords = s->d_texcoords; a.textures = s->d_textures;
        a.tex_width = s->tex_width; a.tex_height = s->tex_height; a.n_textures = s->n_textures;
        a.f = frame_args(s, rx, ry);
        a.f.tile_xy = st->d_tile_xy; a.f.tile_order = nullptr; a.f.n_local_pixels = st->n_local_pixels;
        a.overflow = s->d_overflow;
        a.channels = channels; a.out = out;
        launch_aov(a, s->stream);
    }
    HIPCHK(hipGetLastError());
    return CRT_OK;
}

}  // namespace crt
