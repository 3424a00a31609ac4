// tests/host_tables_check.cpp — host check of what decides what the kernels read:
// the BVH visit tables, the leaf culling groups, scene validation
// (go-pbrt_amd/csrc/scene_tables.h), the schedule's learning step (schedule.h) and
// the environment knobs (knobs.h). Built alone, no HIP, under ASan + UBSan
// (tests/test_host_tables.py); every property is held against brute force
// written here. Node arrays are exact-size heap blocks, so a read past a tree's
// end is an ASan report.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "../go-pbrt_amd/csrc/knobs.h"
#include "../go-pbrt_amd/csrc/scene_tables.h"
#include "../go-pbrt_amd/csrc/schedule.h"

using namespace pbrt;

static long g_checks = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        g_checks++;                                                              \
        if (!(cond)) {                                                           \
            std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                        \
        }                                                                        \
    } while (0)
static long section(const char* name) {
    std::printf("ok %s %ld\n", name, g_checks);
    const long n = g_checks;
    g_checks = 0;
    return n;
}

// ---------------------------------------------------------------- trees
struct Box {
    double lo[3], hi[3];
};
static Box unite(const Box& a, const Box& b) {
    Box r;
    for (int k = 0; k < 3; k++) {
        r.lo[k] = std::min(a.lo[k], b.lo[k]);
        r.hi[k] = std::max(a.hi[k], b.hi[k]);
    }
    return r;
}
static Box box_of(const pbrt_bvh_node& n) {
    Box b;
    for (int k = 0; k < 3; k++) b.lo[k] = n.bmin[k], b.hi[k] = n.bmax[k];
    return b;
}
static void set_box(pbrt_bvh_node& n, const Box& b) {
    for (int k = 0; k < 3; k++) n.bmin[k] = b.lo[k], n.bmax[k] = b.hi[k];
}
static pbrt_bvh_node leaf_node(const Box& b, uint32_t first_prim) {
    pbrt_bvh_node n{};
    set_box(n, b);
    n.offset = first_prim;
    n.n_prims = 1;
    return n;
}
// The depth-first layout of bvh.go:632-651: an interior node's first child follows it, `offset` is
// its second child. Leaves [a, b) of `leaves`; split(a, b) picks where the two children part.
template <class Split, class Axis>
static int build(std::vector<pbrt_bvh_node>& out, const std::vector<Box>& leaves, int a, int b, Split split, Axis axis) {
    const int idx = (int)out.size();
    if (b - a == 1) {
        out.push_back(leaf_node(leaves[(size_t)a], (uint32_t)a));
        return idx;
    }
    out.push_back(pbrt_bvh_node{});
    const int m = split(a, b);
    const int l = build(out, leaves, a, m, split, axis);
    const int r = build(out, leaves, m, b, split, axis);
    set_box(out[(size_t)idx], unite(box_of(out[(size_t)l]), box_of(out[(size_t)r])));
    out[(size_t)idx].offset = (uint32_t)r;
    out[(size_t)idx].n_prims = 0;
    out[(size_t)idx].axis = (uint8_t)axis();
    return idx;
}
static Box small_box(double x, double y, double z, double h = 0.5) { return Box{{x - h, y - h, z - h}, {x + h, y + h, z + h}}; }
static pbrt_scene_desc scene_of(const std::vector<pbrt_bvh_node>& nodes) {
    pbrt_scene_desc s{};
    s.n_nodes = (int32_t)nodes.size();
    s.nodes = nodes.data();
    return s;
}

// ---------------------------------------------------------------- dev_order
// The reference's walk (bvh.go:659-765) for one octant, recursively: near child first; `depth` is
// the number of far children waiting on its stack when the node is visited.
struct Walk {
    std::vector<uint32_t> node, end;
    std::vector<bool> overflow;
};
static void walk(const std::vector<pbrt_bvh_node>& nodes, int oct, uint32_t i, int depth, Walk& w) {
    const size_t idx = w.node.size();
    const pbrt_bvh_node& n = nodes[i];
    w.node.push_back(i);
    w.end.push_back(0);
    w.overflow.push_back(n.n_prims == 0 && depth >= 64);
    if (n.n_prims == 0) {
        const bool neg = (oct >> n.axis) & 1;
        walk(nodes, oct, neg ? n.offset : i + 1, depth + 1, w);
        walk(nodes, oct, neg ? i + 1 : n.offset, depth, w);
    }
    w.end[idx] = (uint32_t)w.node.size();
}
static int check_order(const std::vector<pbrt_bvh_node>& nodes) {
    const pbrt_scene_desc s = scene_of(nodes);
    const size_t n = nodes.size();
    std::vector<uint32_t> out;
    CHECK(dev_order(&s, out));
    CHECK(out.size() == 16 * n);
    int overflows = 0;
    for (int oct = 0; oct < 8; oct++) {
        Walk w;
        walk(nodes, oct, 0, 0, w);
        CHECK(w.node.size() == n);
        size_t nl = 0;
        for (size_t i = 0; i < n; i++) {
            const uint32_t e = out[(size_t)oct * n + i];
            CHECK((e & kOrdNode) == w.node[i]);
            CHECK((e >> 16) == w.end[i]);   // the table index just past the subtree
            CHECK(((e & kOrdOverflow) != 0) == w.overflow[i]);
            overflows += w.overflow[i];
            if (nodes[w.node[i]].n_prims > 0) {
                CHECK((e >> 16) == i + 1);
                CHECK(out[8 * n + (size_t)oct * n + nl] == w.node[i]);   // the leaf lists: the leaves in that order
                nl++;
            }
        }
        for (size_t j = nl; j < n; j++) CHECK(out[8 * n + (size_t)oct * n + j] == 0);
    }
    return overflows;
}
static void check_refused(std::vector<pbrt_bvh_node> nodes) {
    nodes.shrink_to_fit();
    const pbrt_scene_desc s = scene_of(nodes);
    std::vector<uint32_t> out;
    CHECK(!dev_order(&s, out));
}
static void test_dev_order() {
    std::mt19937 rng(20260001);
    auto half = [](int a, int b) { return (a + b) / 2; };
    auto rnd_split = [&](int a, int b) { return a + 1 + (int)(rng() % (unsigned)(b - a - 1)); };
    auto rnd_axis = [&] { return (int)(rng() % 3); };
    auto boxes = [&](int n) {
        std::vector<Box> v;
        for (int i = 0; i < n; i++) v.push_back(small_box((double)(rng() % 100), (double)(rng() % 100), (double)(rng() % 100)));
        return v;
    };
    for (int leaves : {1, 2, 4}) {   // trees of 1, 3 and 7 nodes
        std::vector<pbrt_bvh_node> t;
        build(t, boxes(leaves), 0, leaves, half, rnd_axis);
        CHECK((int)t.size() == 2 * leaves - 1);
        CHECK(check_order(t) == 0);
    }
    {   // a left-deep chain of 70 interior nodes: chain node j is visited with j far children pending
        // in the octants that take its first child first, with none in the others
        std::vector<pbrt_bvh_node> t;
        std::vector<Box> lv = boxes(71);
        build(t, lv, 0, 71, [](int, int b) { return b - 1; }, rnd_axis);
        CHECK(t.size() == 141);
        for (int j = 0; j < 70; j++) CHECK(t[(size_t)j].n_prims == 0 && t[(size_t)j].offset == (uint32_t)(140 - j));
        const int ov = check_order(t);
        CHECK(ov > 0);
        for (auto& nd : t) nd.axis = 0;   // then octants 0, 2, 4, 6 go down the chain: nodes 64..69 overflow in each
        CHECK(check_order(t) == 4 * 6);
    }
    // a random tree of 200 nodes cannot be: n leaves make 2 n - 1 nodes. 199 and 201, several of each
    for (int rep = 0; rep < 6; rep++)
        for (int leaves : {100, 101}) {
            std::vector<pbrt_bvh_node> t;
            build(t, boxes(leaves), 0, leaves, rnd_split, rnd_axis);
            CHECK((int)t.size() == 2 * leaves - 1);
            check_order(t);
        }
    {   // not trees in that layout
        const Box b = small_box(0, 0, 0);
        pbrt_bvh_node in{};
        set_box(in, b);
        auto interior = [&](uint32_t off) {
            pbrt_bvh_node n = in;
            n.offset = off;
            return n;
        };
        check_refused({interior(2), interior(0), leaf_node(b, 0)});                    // offset back into a cycle
        check_refused({interior(1), interior(0)});                                     // nothing but the cycle
        check_refused({interior(5), leaf_node(b, 0), leaf_node(b, 1)});                // offset >= n
        check_refused({interior(3), leaf_node(b, 0), leaf_node(b, 1)});                // offset == n
        check_refused({interior(1), leaf_node(b, 0)});                                 // both children are node 1
        check_refused({leaf_node(b, 0), interior(3), leaf_node(b, 1), leaf_node(b, 2)});   // a forest
        check_refused({interior(2), leaf_node(b, 0), leaf_node(b, 1), leaf_node(b, 2)});   // one node unreachable
        check_refused({interior(2), interior(2), leaf_node(b, 0)});                    // a shared child, one index short
    }
    {   // no nodes: accepted, and the tables are one zeroed row per octant
        pbrt_scene_desc s{};
        std::vector<uint32_t> out(3, 7u);
        CHECK(dev_order(&s, out));
        CHECK(out == std::vector<uint32_t>(16, 0u));
    }
    section("dev_order");
}

// ---------------------------------------------------------------- cull_groups
static double diag2(const Box& b) {
    double d = 0;
    for (int k = 0; k < 3; k++) d += (b.hi[k] - b.lo[k]) * (b.hi[k] - b.lo[k]);
    return d;
}
struct Groups {
    int G = 0;
    std::vector<std::set<uint32_t>> members;   // [G + 1]; last: the leaves tested unconditionally
};
// Runs cull_groups on a tree and holds its output against the tree, whatever it decided.
static Groups check_groups(const std::vector<pbrt_bvh_node>& nodes, int cull_group, int cull_min) {
    const pbrt_scene_desc s = scene_of(nodes);
    const size_t n = nodes.size();
    std::vector<uint32_t> order, masks(5, 9u);
    std::vector<double> bx(5, 9.0);
    CHECK(dev_order(&s, order));
    Groups g;
    g.G = cull_groups(cull_group, cull_min, &s, order, bx, masks);
    CHECK(g.G >= 0 && g.G <= kMaxCullGroups);
    if (g.G == 0) {
        CHECK(bx.empty() && masks.empty());
        return g;
    }
    const size_t G = (size_t)g.G;
    CHECK(bx.size() == 6 * G && masks.size() == 8 * (G + 1));
    size_t nl = 0;
    for (const auto& nd : nodes) nl += nd.n_prims > 0;
    CHECK(nl <= 32);
    const uint32_t all = nl == 32 ? 0xFFFFFFFFu : (1u << nl) - 1u;
    for (int oct = 0; oct < 8; oct++) {
        uint32_t seen = 0;
        std::vector<std::set<uint32_t>> mem(G + 1);
        for (size_t gi = 0; gi <= G; gi++) {
            const uint32_t m = masks[(size_t)oct * (G + 1) + gi];
            CHECK((m & seen) == 0);   // every leaf position once
            seen |= m;
            for (size_t j = 0; j < nl; j++)
                if (m >> j & 1) mem[gi].insert(order[8 * n + (size_t)oct * n + j]);
        }
        CHECK(seen == all);
        if (oct == 0) g.members = mem;
        CHECK(mem == g.members);   // the same leaves in every octant, whatever their positions
    }
    for (size_t gi = 0; gi < G; gi++) {
        CHECK(g.members[gi].size() >= 2 && g.members[gi].size() <= (size_t)cull_group);
        Box u{{1e300, 1e300, 1e300}, {-1e300, -1e300, -1e300}};
        for (uint32_t v : g.members[gi]) u = unite(u, box_of(nodes[v]));
        for (int k = 0; k < 3; k++) CHECK(bx[gi * 6 + (size_t)k] == u.lo[k] && bx[gi * 6 + 3 + (size_t)k] == u.hi[k]);
    }
    const double root = diag2(box_of(nodes[0]));
    for (size_t i = 0; i < n; i++)   // a leaf larger than half the root's diagonal is never grouped
        if (nodes[i].n_prims > 0 && diag2(box_of(nodes[i])) > 0.25 * root) CHECK(g.members[G].count((uint32_t)i) == 1);
    return g;
}
static std::vector<pbrt_bvh_node> tree_of(const std::vector<Box>& leaves) {
    std::vector<pbrt_bvh_node> t;
    int ax = 0;
    build(t, leaves, 0, (int)leaves.size(), [](int a, int b) { return (a + b) / 2; }, [&] { return ax++ % 3; });
    t.shrink_to_fit();
    return t;
}
static void test_cull_groups() {
    // two rows of small leaves (7 and 6) and a floor under them that spans the scene
    std::vector<Box> lv;
    for (int i = 0; i < 7; i++) lv.push_back(small_box(2.0 * i, 0, 0));
    for (int i = 0; i < 6; i++) lv.push_back(small_box(2.0 * i, 10, 0));
    lv.push_back(Box{{-1, -1, -2}, {13, 11, -1}});
    const std::vector<pbrt_bvh_node> t = tree_of(lv);
    CHECK(t.size() == 27);
    size_t floor_node = 0;
    for (size_t i = 0; i < t.size(); i++)
        if (t[i].n_prims > 0 && t[i].offset == 13) floor_node = i;
    for (int cg : {2, 3, 4, 5, 8, 16}) {
        const Groups g = check_groups(t, cg, 2);
        CHECK(g.G > 0);
        size_t grouped = 0;
        for (int gi = 0; gi < g.G; gi++) grouped += g.members[(size_t)gi].size();
        CHECK(g.members[(size_t)g.G].count((uint32_t)floor_node) == 1);
        CHECK(g.members[(size_t)g.G].size() == 14 - grouped);
        // 13 small leaves halve down to 3 + 3 and 3 + 4: at 2 per group each 3 leaves a singleton,
        // which is tested unconditionally beside the floor
        if (cg == 2) CHECK(g.G == 5 && grouped == 10);
        if (cg >= 7) CHECK(grouped == 13);
    }
    {   // more than kLdsNodes nodes: 33 leaves make 65
        std::vector<Box> many;
        for (int i = 0; i < 33; i++) many.push_back(small_box(2.0 * i, 0, 0));
        const std::vector<pbrt_bvh_node> big = tree_of(many);
        CHECK(big.size() == 65 && (int)big.size() > kLdsNodes);
        CHECK(check_groups(big, 4, 2).G == 0);
        // 32 leaves in 63 nodes: accepted, and at 2 per group exactly kMaxCullGroups groups. (More
        // would take 34 leaves: with at most 32 leaves and 2 or more per group that refusal cannot fire.)
        many.pop_back();
        const std::vector<pbrt_bvh_node> full = tree_of(many);
        CHECK(full.size() == 63);
        CHECK(check_groups(full, 2, 2).G == kMaxCullGroups);
        CHECK(check_groups(full, 4, 2).G == 8);
    }
    {   // more than 32 leaves within kLdsNodes nodes (no tree has that: the test comes before any table is read)
        std::vector<pbrt_bvh_node> flat;
        for (int i = 0; i < 40; i++) flat.push_back(leaf_node(small_box(2.0 * i, 0, 0), (uint32_t)i));
        flat.shrink_to_fit();
        const pbrt_scene_desc s = scene_of(flat);
        std::vector<uint32_t> order(16 * flat.size(), 0u), masks;
        std::vector<double> bx;
        CHECK(cull_groups(4, 2, &s, order, bx, masks) == 0 && bx.empty() && masks.empty());
    }
    {   // the grouped share below cull_min: 2 small leaves beside 3 large ones (2 * 2 < 5), enough at cull_min 3
        std::vector<Box> few = {small_box(0, 0, 0), small_box(2, 0, 0), Box{{-1, -1, -2}, {13, 11, -1}},
                                Box{{-1, -1, 2}, {13, 11, 3}}, Box{{-1, -2, -2}, {13, -1, 3}}};
        const std::vector<pbrt_bvh_node> c = tree_of(few);
        CHECK(check_groups(c, 4, 2).G == 0);
        CHECK(check_groups(c, 4, 3).G == 1);
    }
    {   // one leaf, and no nodes
        CHECK(check_groups(tree_of({small_box(0, 0, 0)}), 4, 2).G == 0);
        pbrt_scene_desc s{};
        std::vector<uint32_t> order(16, 0u), masks;
        std::vector<double> bx;
        CHECK(cull_groups(4, 2, &s, order, bx, masks) == 0);
    }
    section("cull_groups");
}

// ---------------------------------------------------------------- validate_scene
struct Scene {   // one sphere under one leaf, one disk, a point light and an area light on the sphere
    std::vector<pbrt_shape_desc> shapes;
    std::vector<pbrt_material_desc> materials;
    std::vector<pbrt_primitive_desc> prims;
    std::vector<pbrt_bvh_node> nodes;
    std::vector<pbrt_light_desc> lights;
    std::vector<float> p;
    std::vector<int32_t> indices;
    std::vector<pbrt_mesh_desc> meshes;
    pbrt_scene_desc d{};
    Scene() : shapes(2), materials(2), prims(2), lights(2), p(9, 0.f), indices{0, 1, 2}, meshes(1) {
        shapes[0].type = PBRT_SHAPE_SPHERE;
        shapes[1].type = PBRT_SHAPE_DISK;
        materials[0].type = PBRT_MAT_MATTE;
        materials[1].type = PBRT_MAT_GLASS;
        prims[0].kind = PBRT_PRIM_GEOMETRIC;
        prims[1].kind = PBRT_PRIM_TRANSFORMED;
        prims[1].shape = 1;
        prims[1].material = 1;
        const Box b = small_box(0, 0, 0);
        nodes = {pbrt_bvh_node{}, leaf_node(b, 0), leaf_node(b, 1)};
        set_box(nodes[0], b);
        nodes[0].offset = 2;
        nodes[0].axis = 2;
        lights[0].type = PBRT_LIGHT_POINT;
        lights[1].type = PBRT_LIGHT_DIFFUSE_AREA;
        lights[1].shape = 0;
        meshes[0].n_vertices = 3;
        meshes[0].n_triangles = 1;
        d.film.crop_max_x = 4;
        d.film.crop_max_y = 3;
        link();
    }
    void link() {
        d.n_shapes = (int32_t)shapes.size();
        d.n_materials = (int32_t)materials.size();
        d.n_prims = (int32_t)prims.size();
        d.n_nodes = (int32_t)nodes.size();
        d.n_lights = (int32_t)lights.size();
        d.n_meshes = (int32_t)meshes.size();
        d.shapes = shapes.data();
        d.materials = materials.data();
        d.prims = prims.data();
        d.nodes = nodes.data();
        d.lights = lights.data();
        meshes[0].p = p.data();
        meshes[0].indices = indices.data();
        d.meshes = meshes.data();
    }
};
template <class F>
static void refused(int code, F mutate) {
    Scene s;
    mutate(s);
    CHECK(validate_scene(&s.d) == code);
}
static void test_validate_scene() {
    {
        Scene s;
        CHECK(validate_scene(&s.d) == PBRT_OK);
        s.d.n_meshes = 0;   // and without meshes
        s.d.meshes = nullptr;
        CHECK(validate_scene(&s.d) == PBRT_OK);
    }
    CHECK(validate_scene(nullptr) == PBRT_E_INVALID);
    refused(PBRT_E_INVALID, [](Scene& s) { s.d.n_prims = -1; });
    refused(PBRT_E_INVALID, [](Scene& s) { s.d.n_lights = -1; });
    refused(PBRT_E_UNSUPPORTED, [](Scene& s) { s.d.n_nodes = 32768; });   // 15-bit node index; refused before a node is read
    refused(PBRT_E_INVALID, [](Scene& s) { s.prims[1].shape = 2; });
    refused(PBRT_E_INVALID, [](Scene& s) { s.prims[0].shape = -1; });
    refused(PBRT_E_INVALID, [](Scene& s) { s.prims[1].material = 2; });
    refused(PBRT_E_INVALID, [](Scene& s) { s.prims[0].kind = 0; });
    refused(PBRT_E_UNSUPPORTED, [](Scene& s) { s.shapes[1].type = 99; });
    refused(PBRT_E_INVALID, [](Scene& s) { s.nodes[2].n_prims = 2; });   // a leaf's range past n_prims
    refused(PBRT_E_INVALID, [](Scene& s) { s.nodes[1].offset = 2; });
    refused(PBRT_E_INVALID, [](Scene& s) { s.nodes[0].offset = 3; });    // a second child past the nodes
    refused(PBRT_E_INVALID, [](Scene& s) { s.nodes[0].axis = 3; });
    refused(PBRT_E_UNSUPPORTED, [](Scene& s) { s.materials[0].type = 3; });
    refused(PBRT_E_UNSUPPORTED, [](Scene& s) { s.materials[1].type = -1; });
    refused(PBRT_E_INVALID, [](Scene& s) { s.d.n_meshes = -1; });
    refused(PBRT_E_INVALID, [](Scene& s) { s.d.meshes = nullptr; });
    refused(PBRT_E_INVALID, [](Scene& s) { s.meshes[0].material = 2; });
    refused(PBRT_E_INVALID, [](Scene& s) { s.meshes[0].n_vertices = -1; });
    refused(PBRT_E_INVALID, [](Scene& s) { s.meshes[0].p = nullptr; });
    refused(PBRT_E_INVALID, [](Scene& s) { s.meshes[0].indices = nullptr; });
    refused(PBRT_E_INVALID, [](Scene& s) { s.indices[2] = 3; s.link(); });    // a mesh index out of range
    refused(PBRT_E_INVALID, [](Scene& s) { s.indices[0] = -1; s.link(); });
    refused(PBRT_E_UNSUPPORTED, [](Scene& s) { s.lights[0].type = 0; });
    refused(PBRT_E_UNSUPPORTED, [](Scene& s) { s.lights[1].shape = 2; });
    refused(PBRT_E_UNSUPPORTED, [](Scene& s) { s.lights[1].shape = 1; });   // an area light on a disk
    refused(PBRT_E_INVALID, [](Scene& s) { s.d.film.crop_max_x = 0; });
    refused(PBRT_E_INVALID, [](Scene& s) { s.d.film.crop_min_y = 3; });
    {   // the content hash: the same bytes hash alike, any record's change shows
        Scene a, b;
        CHECK(scene_content_hash(&a.d) == scene_content_hash(&b.d));
        b.nodes[2].bmax[1] += 1;
        CHECK(scene_content_hash(&a.d) != scene_content_hash(&b.d));
        Scene c;
        c.p[4] = 1.f;
        CHECK(scene_content_hash(&a.d) != scene_content_hash(&c.d));
    }
    section("validate_scene");
}

// ---------------------------------------------------------------- schedule.h
static double factor(int w) { return w == 8 ? 2.3 : w == 4 ? 1.8 : w == 2 ? 1.3 : 1.0; }
static int64_t check_learn(const std::vector<uint32_t>& t, const std::vector<uint8_t>& kw, int ci_wps, int n_simd,
                           int64_t override_k) {
    std::vector<uint32_t> order(3, 77u);
    const int64_t heavy = learn_order(t, kw, ci_wps, n_simd, override_k, order);
    const size_t n = t.size();
    CHECK(order.size() == n);
    std::vector<double> cost(n);
    double sum = 0;
    for (size_t i = 0; i < n; i++) {
        cost[i] = (double)t[i] * factor(i < kw.size() ? kw[i] : 1);
        sum += cost[i];
    }
    std::vector<bool> seen(n, false);
    for (size_t k = 0; k < n; k++) {
        CHECK(order[k] < n && !seen[order[k]]);   // a permutation
        seen[order[k]] = true;
        if (k > 0) {
            CHECK(cost[order[k - 1]] >= cost[order[k]]);                                     // heaviest first
            if (cost[order[k - 1]] == cost[order[k]]) CHECK(order[k - 1] < order[k]);       // ties keep index order
        }
    }
    const double thr = 0.7 * sum / ((double)ci_wps * (double)n_simd);
    int64_t above = 0;
    for (size_t i = 0; i < n; i++) above += cost[i] > thr;
    const int64_t cap = (int64_t)n > (int64_t)ci_wps * n_simd ? n_simd / 16 : n_simd / 4;
    CHECK(heavy == (override_k >= 0 ? override_k : std::min(above, cap)));
    return heavy;
}
static void test_schedule() {
    std::mt19937 rng(20260002);
    const uint8_t waves[] = {1, 2, 4, 8};
    for (int rep = 0; rep < 200; rep++) {
        const size_t n = 1 + rng() % 400;
        std::vector<uint32_t> t(n);
        std::vector<uint8_t> kw(rep % 3 == 0 ? n / 2 : n);   // a short list: the slots past it ran at 1 wave
        for (auto& x : t) x = rep % 2 ? (uint32_t)(rng() % 8) * 1000u : (uint32_t)rng();   // many ties, or none
        if (rep % 5 == 0) t[rng() % n] = 0xFFFFFFFFu;
        for (auto& w : kw) w = waves[rng() % 4];
        check_learn(t, kw, 2 + (int)(rng() % 2), 16 << (rng() % 6), -1);
    }
    {   // the cap: n_simd / 4 up to ci_wps * n_simd tiles, n_simd / 16 from one more on
        const int n_simd = 32, wps = 3;
        const std::vector<uint32_t> at(96, 500u), past(97, 500u);   // equal costs: every tile is above 0.7x the mean
        CHECK(check_learn(at, {}, wps, n_simd, -1) == 8);
        CHECK(check_learn(past, {}, wps, n_simd, -1) == 2);
        CHECK(check_learn(past, {}, wps, n_simd, 5) == 5);    // the override wins
        CHECK(check_learn(past, {}, wps, n_simd, 0) == 0);
        CHECK(check_learn(at, {}, wps, n_simd, 40) == 40);
        std::vector<uint32_t> three(96, 10u);   // fewer heavy tiles than the cap
        three[5] = three[50] = three[95] = 100000u;
        CHECK(check_learn(three, {}, wps, n_simd, -1) == 3);
    }
    CHECK(check_learn({}, {}, 3, 1024, -1) == 0);
    {   // the process cache: by key and size; full, it starts over
        sched_cache_clear();
        SchedEntry e;
        CHECK(!sched_cache_get(1, 3, e));
        sched_cache_put(1, {2, 0, 1}, 1);
        CHECK(sched_cache_get(1, 3, e) && e.order == std::vector<uint32_t>({2, 0, 1}) && e.heavy_k == 1);
        CHECK(!sched_cache_get(1, 4, e) && !sched_cache_get(2, 3, e));
        for (uint64_t k = 2; k <= kSchedCacheMax; k++) sched_cache_put(k, {0}, 0);
        CHECK(sched_cache_get(1, 3, e));
        sched_cache_put(1, {1, 0, 2}, 2);   // a key it holds: kept
        CHECK(sched_cache_get(2, 1, e) && sched_cache_get(1, 3, e) && e.heavy_k == 2);
        sched_cache_put(1000, {0}, 0);      // a new one
        CHECK(!sched_cache_get(1, 3, e) && sched_cache_get(1000, 1, e));
        sched_cache_clear();
        CHECK(!sched_cache_get(1000, 1, e));
    }
    section("schedule");
}

// ---------------------------------------------------------------- Knobs::from_env
extern char** environ;
static Knobs with_env(const char* name, const char* value) {
    setenv(name, value, 1);
    const Knobs k = Knobs::from_env();
    unsetenv(name);
    return k;
}
static void test_knobs() {
    std::vector<std::string> mine;
    for (char** e = environ; *e; e++)
        if (std::strncmp(*e, "PBRT_", 5) == 0) mine.push_back(std::string(*e).substr(0, std::strcspn(*e, "=")));
    for (const std::string& n : mine) unsetenv(n.c_str());
    const Knobs d = Knobs::from_env();
    CHECK(d.ci_waves == 0 && d.ci_stride == 0 && d.ci_heavy_waves == 4 && !d.ci_light_kw && d.ci_split8 == 32);
    CHECK(d.ci_eu == 0 && d.ci_heavy == -1 && d.ci_split && d.ci_order && d.ci_probe && d.ci_order_cache);
    CHECK(d.sp_window && d.ci_scap == -1 && d.ci_nps == 8 && d.paths_overlap == 5 && d.paths_overlap_all);
    CHECK(!d.gate_hold && !d.paths_s1d_lds && d.paths_ci == -1 && d.paths_wf == -1 && !d.pw_sort && d.pw_gb == 24.0);
    CHECK(d.wave_buffer_gb == 0 && !d.ci_dense && d.cull_group == 4 && d.cull_min == 2 && d.cull_groups);
    CHECK(with_env("PBRT_CI_WAVES", "3").ci_waves == 0);   // not 1, 2, 4 or 8: ignored
    CHECK(with_env("PBRT_CI_WAVES", "8").ci_waves == 8);
    CHECK(with_env("PBRT_PATHS_OVERLAP", "99").paths_overlap == 16);
    CHECK(with_env("PBRT_PATHS_OVERLAP", "-3").paths_overlap == 0);
    CHECK(with_env("PBRT_CULL_GROUP", "1").cull_group == 2);
    CHECK(with_env("PBRT_CI_HEAVY_WAVES", "5").ci_heavy_waves == 4);
    CHECK(with_env("PBRT_CI_HEAVY_WAVES", "8").ci_heavy_waves == 8);
    CHECK(with_env("PBRT_PATHS_S1D", "lds").paths_s1d_lds);
    CHECK(!with_env("PBRT_PATHS_S1D", "global").paths_s1d_lds);
    CHECK(!with_env("PBRT_CULL_GROUPS", "0").cull_groups);
    CHECK(with_env("PBRT_CULL_GROUPS", "1").cull_groups);
    CHECK(with_env("PBRT_CI_HEAVY", "7").ci_heavy == 7);
    CHECK(Knobs::from_env().ci_heavy == -1);   // nothing is left set
    section("knobs");
}

int main() {
    test_dev_order();
    test_cull_groups();
    test_validate_scene();
    test_schedule();
    test_knobs();
    return 0;
}
