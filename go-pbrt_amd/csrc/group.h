// group.h — what the device group (group.hip, k_group.hip) shares with the
// single-context code of render.hip.
#pragma once

#include "group_map.h"
#include "render_common.h"

namespace pbrtk {

// the members' tile films as the leader's merge kernel reads them: a member's
// own d_films (the leader's, or a peer pointer) or its staging copy on the leader
struct GroupFilms {
    const double* p[PBRT_GROUP_MAX];
};

// a member context's state after its frame (render.hip: group_member_view)
struct GroupMemberView {
    int device;                         // HIP ordinal the context lives on
    const double* d_films;              // its tile films, rp.n_slots slots of rp.slot_w * rp.slot_h * 3 doubles
    const pbrt_film_desc* d_film;       // the film descriptor in its device memory
    const pbrt_film_desc* host_film;    // and on the host
    RenderParams rp;                    // parameters of its last frame
};

}  // namespace pbrtk

pbrtk::GroupMemberView pbrt_group_member_view(const pbrt_gpu_ctx* c);
