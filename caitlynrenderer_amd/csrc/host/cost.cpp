// [host] crt_cwbvh_cost of include/crt.h: the SAH cost of a range of node8s, node by node and slot by slot.  The reference the device
// kernel behind crt_get_tree_cost / crt_instances_tree_cost (refit.hip k_tree_cost) is compared with: both take every slot's area from
// host/cost_core.hpp, so they agree up to the order in which the areas are added.
#include "../../../include/crt.h"
#include "../crt_error.hpp"
#include "cost_core.hpp"

using crt::fail;

extern "C" {

int crt_cwbvh_cost(const crt_node8* nodes, size_t first, size_t count, size_t root, crt_tree_cost* out) {
    if (!out) return fail(CRT_ERR_INVALID, "crt_cwbvh_cost: null out");
    *out = crt_tree_cost{};
    if (count == 0) return CRT_OK;
    if (!nodes) return fail(CRT_ERR_INVALID, "crt_cwbvh_cost: null nodes");
    if (root < first || root - first >= count) return fail(CRT_ERR_INVALID, "crt_cwbvh_cost: the root lies outside [first, first + count)");
    crt_tree_cost c{};
    c.n_nodes8 = count;
    for (size_t i = first; i < first + count; ++i) {
        const uint8_t* node = reinterpret_cast<const uint8_t*>(nodes + i);
        crt::rf::Box u = crt::rf::empty_box();
        bool used = false;
        for (int s = 0; s < 8; ++s) {
            const uint8_t meta = nodes[i].meta[s];
            if (!meta) continue;
            const crt::rf::Box b = crt::tc::slot_box(node, s);
            const double a = crt::tc::half_area(b);
            if ((nodes[i].imask >> s) & 1u) {
                c.inner_area += a;
                ++c.n_inner_slots;
            } else {
                const int items = crt::rf::leaf_count(meta);
                c.leaf_area += a * (double)items;
                ++c.n_leaf_slots;
                c.n_leaf_items += (uint64_t)items;
            }
            crt::rf::grow(u, b);
            used = true;
        }
        if (i == root && used) c.root_area = crt::tc::half_area(u);
    }
    c.cost = crt::tc::finish(c.root_area, c.inner_area, c.leaf_area);
    *out = c;
    return CRT_OK;
}

}  // extern "C"
