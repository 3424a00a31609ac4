// k_group.hip — the film merge of a device group (pbrt_gpu_group, group.hip)
#pragma clang fp contract(off)

#include "group.h"

namespace pbrtk {

// k_merge_film over the tile films of every member of a device group, run on
// the leader once all members' frames have ended. A film pixel's thread walks
// the 3x3 tiles around its own in ascending tile index, exactly as k_merge_film
// does, applies the same RGBToXYZ to each contribution and adds them in the
// same order; only where a tile's film lives differs: member and slot come from
// group_locate (group_map.h, which also made the members' tile subsets), and
// films.p[member] is that member's tile films -- the leader's own, a peer
// pointer, or a staging copy. So the sums are, bit for bit, the ones a single
// context computes for the same frame. Every tile-film pixel is read once.
// Unlike k_merge_film it tests no cancel_seen flag: it is launched only after the
// host has every member's result, so the host skips the launch for a cancelled
// or panicked frame (and a staged member's flag is not readable from the leader).
__global__ __launch_bounds__(256) void k_merge_film_group(const pbrt_film_desc* __restrict__ film_desc, RenderParams rp,
                                                          pbrtgroup::GroupMap gm, GroupFilms films,
                                                          double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rp.film_w * rp.film_h) return;
    const pbrt_film_desc& f = *film_desc;
    const int64_t x = rp.film_min_x + i % rp.film_w, y = rp.film_min_y + i / rp.film_w;
    const int64_t tx = (x - rp.film_min_x) / rp.tile_size, ty = (y - rp.film_min_y) / rp.tile_size;
    double v0 = 0, v1 = 0, v2 = 0;
    for (int64_t dy = -1; dy <= 1; dy++) {
        for (int64_t dx = -1; dx <= 1; dx++) {
            int64_t cx = tx + dx, cy = ty + dy;
            if (cx < 0 || cy < 0 || cx >= rp.ntx || cy >= rp.nty) continue;
            int64_t tile = cy * rp.ntx + cx;
            int32_t member;
            int64_t slot;
            if (!pbrtgroup::group_locate(gm, tile, member, slot)) continue;
            int64_t x0, y0, x1, y1, px0, py0, px1, py1;
            tile_bounds(rp, tile, x0, y0, x1, y1);
            film_tile_bounds(f, x0, y0, x1, y1, px0, py0, px1, py1);
            if (x < px0 || x >= px1 || y < py0 || y >= py1) continue;
            const double* c = films.p[member] + slot * (rp.slot_w * rp.slot_h * 3) +
                              ((x - px0) + (y - py0) * (px1 - px0)) * 3;
            // spectrum.go:35-41 RGBToXYZ
            v0 += 0.412453 * c[0] + 0.357580 * c[1] + 0.180423 * c[2];
            v1 += 0.212671 * c[0] + 0.715160 * c[1] + 0.072169 * c[2];
            v2 += 0.019334 * c[0] + 0.119193 * c[1] + 0.950227 * c[2];
        }
    }
    out[i * 3 + 0] = v0;
    out[i * 3 + 1] = v1;
    out[i * 3 + 2] = v2;
}

}  // namespace pbrtk
