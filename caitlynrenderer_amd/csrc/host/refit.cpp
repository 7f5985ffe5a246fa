// [host] refits of include/crt.h (crt_bvh2_refit, crt_cwbvh_refit): new boxes for new vertex positions, topology unchanged.
// The reference the device refit of crt_update_vertices (refit.hip) is compared with, byte for byte: both take every box
// and every quantised plane from host/refit_core.hpp.
#include <string>
#include <vector>

#include "../../../include/crt.h"
#include "../crt_error.hpp"
#include "flatnode_link.hpp"
#include "refit_core.hpp"

using crt::fail;
using crt::rf::Box;

namespace {

// what crt_scene_create accepts: every coordinate finite and within 1e18
bool coordinates_ok(const float* v, size_t n_vertices) {
    for (size_t i = 0; i < 3 * n_vertices; ++i)
        if (!(v[i] <= 1.0e18f && v[i] >= -1.0e18f)) return false;
    return true;
}

bool vertices_ok(const crt_triangle& t, size_t n_vertices) {
    for (int j = 0; j < 3; ++j)
        if (t.v[j] < 0 || (size_t)t.v[j] >= n_vertices) return false;
    return true;
}

}  // namespace

extern "C" {

int crt_bvh2_refit(crt_flatnode* nodes, size_t n_nodes, const crt_triangle* leaf_tris, size_t n_slots, const float* vertices, size_t n_vertices) {
    if (!nodes || !n_nodes || !leaf_tris || !vertices) return fail(CRT_ERR_INVALID, "crt_bvh2_refit: null argument");
    if (!coordinates_ok(vertices, n_vertices)) return fail(CRT_ERR_INVALID, "crt_bvh2_refit: a vertex coordinate is not finite or exceeds 1e18");
    for (size_t i = 0; i < n_slots; ++i)
        if (!vertices_ok(leaf_tris[i], n_vertices)) return fail(CRT_ERR_INVALID, "crt_bvh2_refit: vertex index out of range");
    // children after their parent (crt_scene_create's rule for a BVH2): one reverse pass sees every child before its parent
    for (size_t i = 0; i < n_nodes; ++i) {
        const crt_flatnode& f = nodes[i];
        const size_t a = (size_t)crt::link_of(f.bmin[3]);
        if (f.bmax[3] != 0.0f) {
            if (!(f.bmax[3] >= 1.0f) || a + (size_t)f.bmax[3] > n_slots) return fail(CRT_ERR_INVALID, "crt_bvh2_refit: leaf range outside the triangle array");
        } else if (a <= i || a + 1 >= n_nodes) {
            return fail(CRT_ERR_INVALID, "crt_bvh2_refit: child link out of order");
        }
    }
    for (size_t i = n_nodes; i-- > 0;) {
        crt_flatnode& f = nodes[i];
        const size_t a = (size_t)crt::link_of(f.bmin[3]);
        Box b = crt::rf::empty_box();
        if (f.bmax[3] != 0.0f) {
            for (size_t s = a; s < a + (size_t)f.bmax[3]; ++s) crt::rf::grow_triangle(b, leaf_tris[s].v, vertices);
        } else {
            for (size_t c = a; c <= a + 1; ++c)
                for (int k = 0; k < 3; ++k) {
                    b.lo[k] = crt::rf::tmin(b.lo[k], nodes[c].bmin[k]);
                    b.hi[k] = crt::rf::tmax(b.hi[k], nodes[c].bmax[k]);
                }
        }
        for (int k = 0; k < 3; ++k) { f.bmin[k] = b.lo[k]; f.bmax[k] = b.hi[k]; }
    }
    return CRT_OK;
}

int crt_cwbvh_refit(crt_node8* nodes, size_t n_nodes8, const int32_t* tri_slots, size_t n_tris8, const crt_triangle* leaf_tris, size_t n_slots,
                    const float* vertices, size_t n_vertices) {
    if (!nodes || !n_nodes8 || !tri_slots || !leaf_tris || !vertices) return fail(CRT_ERR_INVALID, "crt_cwbvh_refit: null argument");
    for (size_t i = 0; i < n_tris8; ++i)
        if (tri_slots[i] < 0 || (size_t)tri_slots[i] >= n_slots) return fail(CRT_ERR_INVALID, "crt_cwbvh_refit: triangle slot out of range");
    if (!coordinates_ok(vertices, n_vertices)) return fail(CRT_ERR_INVALID, "crt_cwbvh_refit: a vertex coordinate is not finite or exceeds 1e18");
    for (size_t i = 0; i < n_slots; ++i)
        if (!vertices_ok(leaf_tris[i], n_vertices)) return fail(CRT_ERR_INVALID, "crt_cwbvh_refit: vertex index out of range");
    // parents before children, from the root: each node once (a node reached twice would be a DAG, not a tree)
    std::vector<uint32_t> order;
    std::vector<uint8_t> seen(n_nodes8, 0);
    order.reserve(n_nodes8);
    order.push_back(0);
    seen[0] = 1;
    for (size_t k = 0; k < order.size(); ++k) {
        const crt_node8& n = nodes[order[k]];
        for (int s = 0; s < 8; ++s) {
            if (!n.meta[s]) continue;
            if ((n.imask >> s) & 1u) {
                const uint32_t c = crt::rf::inner_child(n, s);
                if (c >= n_nodes8 || seen[c]) return fail(CRT_ERR_INVALID, "crt_cwbvh_refit: child index out of range or referenced twice");
                seen[c] = 1;
                order.push_back(c);
            } else {
                const size_t t = (size_t)n.triangle_base_index + (size_t)crt::rf::leaf_offset(n.meta[s]);
                if (t + (size_t)crt::rf::leaf_count(n.meta[s]) > n_tris8) return fail(CRT_ERR_INVALID, "crt_cwbvh_refit: triangle index out of range");
            }
        }
    }
    std::vector<Box> box(n_nodes8);
    for (size_t k = order.size(); k-- > 0;) {
        crt_node8& n = nodes[order[k]];
        Box slot[8];
        Box u = crt::rf::empty_box();
        for (int s = 0; s < 8; ++s) {
            slot[s] = crt::rf::empty_box();
            if (!n.meta[s]) continue;
            if ((n.imask >> s) & 1u) {
                slot[s] = box[crt::rf::inner_child(n, s)];
            } else {
                const size_t t = (size_t)n.triangle_base_index + (size_t)crt::rf::leaf_offset(n.meta[s]);
                for (int j = 0; j < crt::rf::leaf_count(n.meta[s]); ++j) crt::rf::grow_triangle(slot[s], leaf_tris[tri_slots[t + j]].v, vertices);
            }
            crt::rf::grow(u, slot[s]);
        }
        float scale[3];
        crt::rf::node_frame(u, n.p, n.e, scale);
        uint8_t* planes[6] = {n.qlo_x, n.qhi_x, n.qlo_y, n.qhi_y, n.qlo_z, n.qhi_z};
        for (int s = 0; s < 8; ++s) {
            if (!n.meta[s]) continue;
            uint8_t q[6];
            crt::rf::quantise_slot(slot[s], n.p, scale, q);
            for (int r = 0; r < 6; ++r) planes[r][s] = q[r];
        }
        box[order[k]] = u;
    }
    return CRT_OK;
}

}  // extern "C"
