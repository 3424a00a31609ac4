// bvh_tables.h — the sizes and bit fields of the BVH visit tables that the host
// builds (scene_tables.h) and the kernels read (pbrt_path.h). No HIP.
#pragma once

#include <cstdint>

namespace pbrt {

// BVH nodes staged in LDS by kernels whose scene fits (README / Cornell: <= 45 nodes).
constexpr int kLdsNodes = 64;
// Entry i of an octant's preorder visit table (dev_order) holds
//   bits  0-14  the node index (pbrt_bvh_node order)
//   bit   15    a hit at this interior node would push past the [64] stack
//               (bvh.go:670: the reference panics there)
//   bits 16-31  the table index that follows the node's subtree (its skip)
constexpr uint32_t kOrdNode = 0x7FFFu, kOrdOverflow = 0x8000u;
// Leaf culling groups of an LDS-staged tree (cull_groups), at most.
constexpr int kMaxCullGroups = 16;

}  // namespace pbrt
