// group_map.h — how a device group (pbrt_gpu_group, include/pbrt_gpu.h) splits
// a frame's tiles over its members. The host split (group.hip, one
// pbrt_render_desc per member) and the merge kernel (k_merge_film_group, which
// finds a tile's film) both go through this header, so they cannot disagree.
// Plain C++ with no dependency, host and device: tests/group_map_check.cpp
// compiles it on its own.
//
// The caller's render desc names the tiles t_k = begin + k * stride < end
// (pbrt_render_desc: tile_end <= 0 or past the frame means all tiles). Tile t_k
// goes to member k mod N as that member's slot k div N, so member m renders
// {tile_begin: begin + m * stride, tile_end: end, tile_stride: stride * N}
// through the single-context path, whose slot s is its s-th tile.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PBRT_GROUP_HD __host__ __device__
#else
#define PBRT_GROUP_HD
#endif

namespace pbrtgroup {

struct GroupMap {
    int64_t begin, end, stride;   // the caller's subset, normalised: 0 <= begin, end <= total tiles, stride >= 1
    int64_t n_tiles;              // tiles of the subset (k = 0 .. n_tiles - 1)
    int32_t n_members;            // N
    int32_t pad0;
};

// the subset of a frame of total_tiles tiles that (tile_begin, tile_end,
// tile_stride) names, normalised as the single-context path reads them
PBRT_GROUP_HD inline GroupMap group_map_make(int64_t total_tiles, int64_t tile_begin, int64_t tile_end,
                                             int64_t tile_stride, int32_t n_members) {
    GroupMap g;
    g.begin = tile_begin < 0 ? 0 : tile_begin;
    g.end = tile_end > 0 && tile_end < total_tiles ? tile_end : total_tiles;
    g.stride = tile_stride > 0 ? tile_stride : 1;
    g.n_tiles = g.begin < g.end ? (g.end - g.begin + g.stride - 1) / g.stride : 0;
    g.n_members = n_members > 0 ? n_members : 1;
    g.pad0 = 0;
    return g;
}

// member m's tile subset, as the fields of its pbrt_render_desc
PBRT_GROUP_HD inline void group_member_tiles(const GroupMap& g, int32_t m, int64_t& tile_begin, int64_t& tile_end,
                                             int64_t& tile_stride) {
    tile_begin = g.begin + (int64_t)m * g.stride;
    tile_end = g.end;
    tile_stride = g.stride * g.n_members;
}

// slots member m renders
PBRT_GROUP_HD inline int64_t group_member_slots(const GroupMap& g, int32_t m) {
    return g.n_tiles > m ? (g.n_tiles - m + g.n_members - 1) / g.n_members : 0;
}

// which member renders tile, and as which of its slots; false: the tile is not in the subset
PBRT_GROUP_HD inline bool group_locate(const GroupMap& g, int64_t tile, int32_t& member, int64_t& slot) {
    if (tile < g.begin || tile >= g.end || (tile - g.begin) % g.stride != 0) return false;
    const int64_t k = (tile - g.begin) / g.stride;
    member = (int32_t)(k % g.n_members);
    slot = k / g.n_members;
    return true;
}

}  // namespace pbrtgroup
