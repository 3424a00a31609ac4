// tests/group_map_check.cpp — host check of the device group's tile mapping
// (go-pbrt_amd/csrc/group_map.h): for every frame of 1..40 tiles, tile_begin
// 0..3, tile_stride 1..3, tile_end in {0, total - 1, total} and 1..8 members,
//   - the members' own enumerations (each member's render desc read the way the
//     single-context path reads one: t = begin, begin + stride, ... < end)
//     partition the caller's subset;
//   - a member's slots are dense from 0 (its s-th tile is its slot s, and
//     group_member_slots counts them);
//   - group_locate gives, for every tile of the subset, the member that
//     enumerates it and its position in that member's enumeration, and rejects
//     every tile outside the subset.
// Compiled with -fsanitize=address,undefined and run by tests/test_group_abi.py;
// prints "cases=.. tiles=.. bad=..".
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../go-pbrt_amd/csrc/group_map.h"

using namespace pbrtgroup;

// the single-context path's reading of a render desc's tile subset
static std::vector<int64_t> enumerate(int64_t total, int64_t tile_begin, int64_t tile_end, int64_t tile_stride) {
    const int64_t begin = tile_begin < 0 ? 0 : tile_begin;
    const int64_t end = tile_end > 0 && tile_end < total ? tile_end : total;
    const int64_t stride = tile_stride > 0 ? tile_stride : 1;
    std::vector<int64_t> t;
    for (int64_t x = begin; x < end; x += stride) t.push_back(x);
    return t;
}

int main() {
    long cases = 0, tiles = 0, bad = 0;
    for (int64_t total = 1; total <= 40; total++)
        for (int64_t begin = 0; begin <= 3; begin++)
            for (int64_t stride = 1; stride <= 3; stride++)
                for (int64_t end : {(int64_t)0, total - 1, total})
                    for (int32_t n = 1; n <= 8; n++) {
                        cases++;
                        const std::vector<int64_t> want = enumerate(total, begin, end, stride);
                        const GroupMap g = group_map_make(total, begin, end, stride, n);
                        if (g.n_tiles != (int64_t)want.size()) bad++;
                        std::vector<int> owner((size_t)total, -1);
                        std::vector<int64_t> slot_of((size_t)total, -1);
                        for (int32_t m = 0; m < n; m++) {
                            int64_t mb, me, ms;
                            group_member_tiles(g, m, mb, me, ms);
                            // a member's tile_end must mean to it what end means to the group:
                            // never 0 ("all tiles") unless the group's own end is the whole frame
                            const std::vector<int64_t> mine = enumerate(total, mb, me, ms);
                            if ((int64_t)mine.size() != group_member_slots(g, m)) bad++;
                            for (size_t s = 0; s < mine.size(); s++) {   // slots dense from 0: position s is slot s
                                const int64_t t = mine[s];
                                if (owner[(size_t)t] != -1) bad++;       // two members render one tile
                                owner[(size_t)t] = m;
                                slot_of[(size_t)t] = (int64_t)s;
                            }
                        }
                        std::vector<char> in_subset((size_t)total, 0);
                        for (int64_t t : want) in_subset[(size_t)t] = 1;
                        for (int64_t t = -1; t <= total; t++) {
                            int32_t m = -7;
                            int64_t s = -7;
                            const bool found = group_locate(g, t, m, s);
                            const bool expect = t >= 0 && t < total && in_subset[(size_t)t];
                            if (found != expect) {
                                bad++;
                                continue;
                            }
                            if (t >= 0 && t < total && !expect && owner[(size_t)t] != -1) bad++;   // rendered, not in the subset
                            if (!found) continue;
                            tiles++;
                            if (m != owner[(size_t)t] || s != slot_of[(size_t)t]) bad++;
                        }
                    }
    std::printf("cases=%ld tiles=%ld bad=%ld\n", cases, tiles, bad);
    return bad == 0 ? 0 : 1;
}
