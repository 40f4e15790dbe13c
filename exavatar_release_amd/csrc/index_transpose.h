// The transposed index table every gather-style backward of the library reads, stated once.  Host code only.
//
// `idx` holds n_slots indices into [0, n_targets).  For every target v, entries[offsets[v] .. offsets[v + 1]) lists the
// slots e with idx[e] == v in ASCENDING e -- for a [rows, K] table that is ascending row, then slot.  With `skip_minus_one`
// a slot that holds -1 names no target and is left out.  offsets [n_targets + 1] and entries [n_slots] are the caller's;
// entries past offsets[n_targets] are not written.  Returns -1, or the first slot whose index is not accepted (nothing
// useful is left in offsets / entries then).  exa_mesh_vertex_faces, exa_mesh_neighbor_transpose and
// exa_mesh_flip_symmetry_plan (include/exa_mesh.h) are this function behind their own argument checks and messages.
#pragma once
#include <stdint.h>

namespace exa {

inline int64_t index_transpose(int32_t n_targets, int64_t n_slots, const int32_t* idx, bool skip_minus_one,
                               int32_t* offsets, int32_t* entries) {
    for (int32_t v = 0; v <= n_targets; ++v) offsets[v] = 0;
    for (int64_t e = 0; e < n_slots; ++e) {
        if (skip_minus_one && idx[e] == -1) continue;
        if (idx[e] < 0 || idx[e] >= n_targets) return e;
        offsets[idx[e] + 1]++;
    }
    for (int32_t v = 0; v < n_targets; ++v) offsets[v + 1] += offsets[v];
    // ascending slot per target: walk the slots in order, each target's cursor starts at its offset
    for (int64_t e = 0; e < n_slots; ++e) {
        if (skip_minus_one && idx[e] == -1) continue;
        entries[offsets[idx[e]]++] = (int32_t)e;
    }
    for (int32_t v = n_targets; v > 0; --v) offsets[v] = offsets[v - 1];
    offsets[0] = 0;
    return -1;
}

}  // namespace exa
