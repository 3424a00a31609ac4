// scene_tables.h — what pbrt_gpu_create derives from a scene descriptor on the
// host before anything is uploaded: its validation, its content hash, the BVH's
// preorder visit tables and the leaf culling groups. No HIP:
// tests/host_tables_check.cpp compiles this header on its own.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <functional>
#include <limits>
#include <vector>

#include "../../include/pbrt_gpu.h"
#include "bvh_tables.h"

namespace pbrt {

inline uint64_t fnv_bytes(uint64_t h, const void* p, size_t n) {
    const unsigned char* b = (const unsigned char*)p;
    for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}
// Content hash of a scene descriptor: every analytic record, the camera and
// film, and per mesh its sizes plus up to 4096 evenly spread vertices and
// triangles (a mesh of 10M triangles is not hashed whole on every create).
inline uint64_t scene_content_hash(const pbrt_scene_desc* s) {
    uint64_t h = 1469598103934665603ull;
    const int32_t counts[] = {s->n_shapes, s->n_materials, s->n_prims, s->n_nodes, s->n_lights, s->n_meshes};
    h = fnv_bytes(h, counts, sizeof(counts));
    if (s->n_shapes > 0) h = fnv_bytes(h, s->shapes, sizeof(pbrt_shape_desc) * (size_t)s->n_shapes);
    if (s->n_materials > 0) h = fnv_bytes(h, s->materials, sizeof(pbrt_material_desc) * (size_t)s->n_materials);
    if (s->n_prims > 0) h = fnv_bytes(h, s->prims, sizeof(pbrt_primitive_desc) * (size_t)s->n_prims);
    if (s->n_nodes > 0) h = fnv_bytes(h, s->nodes, sizeof(pbrt_bvh_node) * (size_t)s->n_nodes);
    if (s->n_lights > 0) h = fnv_bytes(h, s->lights, sizeof(pbrt_light_desc) * (size_t)s->n_lights);
    h = fnv_bytes(h, &s->camera, sizeof(s->camera));
    h = fnv_bytes(h, &s->film, sizeof(s->film));
    for (int m = 0; m < s->n_meshes && s->meshes; m++) {
        const pbrt_mesh_desc& md = s->meshes[m];
        const int32_t mc[] = {md.n_vertices, md.n_triangles, md.material, md.reverse_orientation};
        h = fnv_bytes(h, mc, sizeof(mc));
        const int64_t nv = md.n_vertices, nt = md.n_triangles;
        for (int64_t i = 0, st = std::max<int64_t>(1, nv / 4096); md.p && i < nv; i += st)
            h = fnv_bytes(h, md.p + 3 * i, 3 * sizeof(float));
        for (int64_t i = 0, st = std::max<int64_t>(1, nt / 4096); md.indices && i < nt; i += st)
            h = fnv_bytes(h, md.indices + 3 * i, 3 * sizeof(int32_t));
    }
    return h;
}

// Preorder visit tables of the BVH, one per ray-direction octant (bvh_walk,
// pbrt_path.h). Node i's children: i + 1 and nodes[i].offset; the reference
// visits offset first when the direction along nodes[i].axis is negative
// (bvh.go:693-703). depth = far children pending on the reference's stack.
// Returns false if the node array is not a tree in that depth-first layout.
inline bool dev_order(const pbrt_scene_desc* s, std::vector<uint32_t>& out) {
    const int n = s->n_nodes;
    out.assign((size_t)16 * (n > 0 ? n : 1), 0u);   // [8][n] preorder, then [8][n] leaves in preorder
    if (n == 0) return true;
    struct Item { uint32_t node, depth; int64_t slot; };   // slot: table index whose skip this item sets (-1: none)
    for (int oct = 0; oct < 8; oct++) {
        uint32_t* t = out.data() + (size_t)oct * n;
        std::vector<Item> st;
        std::vector<int64_t> open;   // table indices of interior nodes whose skip is still unknown
        int k = 0;
        st.push_back({0u, 0u, -1});
        while (!st.empty()) {
            Item it = st.back();
            st.pop_back();
            if (it.slot >= 0) {   // marker: the subtree of table entry `slot` ends here
                t[it.slot] |= (uint32_t)k << 16;
                continue;
            }
            if (k >= n || it.node >= (uint32_t)n) return false;
            const pbrt_bvh_node& nd = s->nodes[it.node];
            const int idx = k++;
            const bool interior = nd.n_prims == 0;
            t[idx] = it.node | ((interior && it.depth >= 64) ? kOrdOverflow : 0u);
            if (!interior) {
                t[idx] |= (uint32_t)(idx + 1) << 16;
                continue;
            }
            const bool neg = (oct >> nd.axis) & 1;
            const uint32_t near_node = neg ? nd.offset : it.node + 1, far_node = neg ? it.node + 1 : nd.offset;
            st.push_back({0u, 0u, (int64_t)idx});            // after both subtrees: set skip
            st.push_back({far_node, it.depth, -1});           // visited after the near subtree
            st.push_back({near_node, it.depth + 1, -1});      // far child pending on the stack
        }
        if (k != n) return false;
        int nl = 0;
        for (int i = 0; i < n; i++) {
            const uint32_t node = t[i] & kOrdNode;
            if (s->nodes[node].n_prims > 0) out[(size_t)8 * n + (size_t)oct * n + nl++] = node;
        }
    }
    return true;
}

// Leaf culling groups of an LDS-staged tree of <= 32 leaves (bvh_walk_analytic): leaves whose
// box diagonal exceeds half the root's (the README floor and wall disks) and
// singletons are tested unconditionally; the others are split recursively at
// the median of their box centres along the widest axis into groups of <= 8
// (the README's three rows of seven spheres become row segments). A group's
// box is the exact union of its members' boxes. Output: boxes [G][6], then per
// octant [G + 1] masks over the octant's leaf preorder positions (last: the
// unconditional leaves). G = 0 (no culling) when the tree is not LDS-staged
// or the grouping needs more than kMaxCullGroups groups.
// cull_group, cull_min: the knobs PBRT_CULL_GROUP and PBRT_CULL_MIN (knobs.h).
inline int cull_groups(int cull_group, int cull_min, const pbrt_scene_desc* s, const std::vector<uint32_t>& order,
                       std::vector<double>& boxes, std::vector<uint32_t>& masks) {
    const double kInf = std::numeric_limits<double>::infinity();
    boxes.clear();
    masks.clear();
    const int n = s->n_nodes;
    if (n == 0 || n > kLdsNodes) return 0;
    std::vector<int> leaves;
    for (int i = 0; i < n; i++)
        if (s->nodes[i].n_prims > 0) leaves.push_back(i);
    if (leaves.size() > 32) return 0;
    auto diag2 = [&](int i) {
        double d = 0;
        for (int k = 0; k < 3; k++) d += (s->nodes[i].bmax[k] - s->nodes[i].bmin[k]) * (s->nodes[i].bmax[k] - s->nodes[i].bmin[k]);
        return d;
    };
    const double root = diag2(0);
    std::vector<int> rest;
    std::vector<int> group_of((size_t)n, -1);   // -1: unconditional
    for (int v : leaves)
        if (!(diag2(v) > 0.25 * root)) rest.push_back(v);
    std::vector<std::vector<int>> groups;
    // leaves per group at most: 4 measured best on config B (chain 420 -> 404 ms against 8;
    // 2: 450, 3: 403, 5: 418, 16: 492; profiles/r02/cull_group_ab.json). PBRT_CULL_GROUP overrides.
    const size_t gmax = (size_t)cull_group;
    std::function<void(std::vector<int>)> split = [&](std::vector<int> g) {
        if (g.size() <= gmax) {
            if (g.size() > 1) groups.push_back(g);
            return;
        }
        double lo[3] = {kInf, kInf, kInf}, hi[3] = {-kInf, -kInf, -kInf};
        auto cen = [&](int v, int k) { return 0.5 * (s->nodes[v].bmin[k] + s->nodes[v].bmax[k]); };
        for (int v : g)
            for (int k = 0; k < 3; k++) { lo[k] = std::min(lo[k], cen(v, k)); hi[k] = std::max(hi[k], cen(v, k)); }
        int a = 0;
        for (int k = 1; k < 3; k++)
            if (hi[k] - lo[k] > hi[a] - lo[a]) a = k;
        std::stable_sort(g.begin(), g.end(), [&](int x, int y) { return cen(x, a) < cen(y, a); });
        const size_t h = g.size() / 2;
        split(std::vector<int>(g.begin(), g.begin() + (long)h));
        split(std::vector<int>(g.begin() + (long)h, g.end()));
    };
    if (!rest.empty()) split(rest);
    const int G = (int)groups.size();
    // worth it only when the groups can skip a fair share of the leaf tests
    // (README: 21 of 23 leaves grouped; Cornell: 2 of 8, not grouped)
    const int min_frac2 = cull_min;   // grouped leaves must be at least half of all (PBRT_CULL_MIN=0: any)
    if (G == 0 || G > kMaxCullGroups || min_frac2 * (int)rest.size() < (int)leaves.size()) return 0;
    boxes.assign((size_t)G * 6, 0.0);
    for (int gi = 0; gi < G; gi++) {
        for (int k = 0; k < 3; k++) {
            boxes[(size_t)gi * 6 + k] = kInf;
            boxes[(size_t)gi * 6 + 3 + k] = -kInf;
        }
        for (int v : groups[(size_t)gi]) {
            group_of[(size_t)v] = gi;
            for (int k = 0; k < 3; k++) {
                boxes[(size_t)gi * 6 + k] = std::min(boxes[(size_t)gi * 6 + k], s->nodes[v].bmin[k]);
                boxes[(size_t)gi * 6 + 3 + k] = std::max(boxes[(size_t)gi * 6 + 3 + k], s->nodes[v].bmax[k]);
            }
        }
    }
    masks.assign((size_t)8 * (G + 1), 0u);
    const int nl = (int)leaves.size();
    for (int oct = 0; oct < 8; oct++)
        for (int j = 0; j < nl; j++) {
            const uint32_t node = order[(size_t)8 * n + (size_t)oct * n + (size_t)j];
            const int gi = group_of[node];
            masks[(size_t)oct * (G + 1) + (size_t)(gi < 0 ? G : gi)] |= 1u << j;
        }
    return G;
}

// PBRT_OK, or why pbrt_gpu_create refuses the scene: PBRT_E_INVALID for a descriptor
// that contradicts itself, PBRT_E_UNSUPPORTED for what the kernels do not take.
inline int validate_scene(const pbrt_scene_desc* s) {
    if (!s) return PBRT_E_INVALID;
    if (s->n_prims < 0 || s->n_nodes < 0 || s->n_lights < 0 || s->n_shapes < 0 || s->n_materials < 0)
        return PBRT_E_INVALID;
    if (s->n_nodes > 32767) return PBRT_E_UNSUPPORTED;   // 15-bit node index in the preorder tables
    for (int i = 0; i < s->n_prims; i++) {
        const pbrt_primitive_desc& p = s->prims[i];
        if (p.shape < 0 || p.shape >= s->n_shapes || p.material < 0 || p.material >= s->n_materials)
            return PBRT_E_INVALID;
        if (p.kind != PBRT_PRIM_GEOMETRIC && p.kind != PBRT_PRIM_TRANSFORMED) return PBRT_E_INVALID;
    }
    for (int i = 0; i < s->n_shapes; i++)
        if (s->shapes[i].type != PBRT_SHAPE_SPHERE && s->shapes[i].type != PBRT_SHAPE_DISK) return PBRT_E_UNSUPPORTED;
    for (int i = 0; i < s->n_nodes; i++) {
        const pbrt_bvh_node& n = s->nodes[i];
        if (n.n_prims > 0 && (int64_t)n.offset + n.n_prims > s->n_prims) return PBRT_E_INVALID;
        if (n.n_prims == 0 && (n.offset >= (uint32_t)s->n_nodes || n.axis > 2)) return PBRT_E_INVALID;
    }
    for (int i = 0; i < s->n_materials; i++)
        if (s->materials[i].type < PBRT_MAT_MATTE || s->materials[i].type > PBRT_MAT_GLASS) return PBRT_E_UNSUPPORTED;
    if (s->n_meshes < 0 || (s->n_meshes > 0 && !s->meshes)) return PBRT_E_INVALID;
    for (int i = 0; i < s->n_meshes; i++) {
        const pbrt_mesh_desc& m = s->meshes[i];
        if (m.n_vertices < 0 || m.n_triangles < 0 || m.material < 0 || m.material >= s->n_materials ||
            (m.n_triangles > 0 && (!m.p || !m.indices)))
            return PBRT_E_INVALID;
        for (int64_t k = 0; k < 3 * (int64_t)m.n_triangles; k++)
            if (m.indices[k] < 0 || m.indices[k] >= m.n_vertices) return PBRT_E_INVALID;
    }
    for (int i = 0; i < s->n_lights; i++) {
        const pbrt_light_desc& l = s->lights[i];
        if (l.type < PBRT_LIGHT_POINT || l.type > PBRT_LIGHT_DIFFUSE_AREA) return PBRT_E_UNSUPPORTED;
        if (l.type == PBRT_LIGHT_DIFFUSE_AREA &&
            (l.shape < 0 || l.shape >= s->n_shapes || s->shapes[l.shape].type != PBRT_SHAPE_SPHERE))
            return PBRT_E_UNSUPPORTED;
    }
    const pbrt_film_desc& f = s->film;
    if (f.crop_max_x <= f.crop_min_x || f.crop_max_y <= f.crop_min_y) return PBRT_E_INVALID;
    return PBRT_OK;
}

}  // namespace pbrt
