// The house scan, shared by binning.hip and densify.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace exa {

// Wave-wide inclusive scans on the DPP path of the VALU: the value of the lane `d` below inside a row of 16 lanes (row_shr,
// d = 1 2 4 8), then lane 15 of rows 0 and 2 added to all of rows 1 and 3 (row_bcast:15), then lane 31 to the upper half
// (row_bcast:31) -- six dependent VALU operations.  A lane without a source (the first d of a row, the rows a row mask
// leaves out) receives the zero passed as the old value.  Through __shfl_up the same six steps are six dependent
// ds_bpermute round trips through the LDS crossbar (twelve for 64 bits); in cell_scatter_kernel, three scans deep, that
// chain and not the barriers was what the scan phases took (phase probe, profiles/scatter_overlap_ab.md).  Integer sums
// in another order: the same result.  All 64 lanes of the wave must be active, as before.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_or_zero(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, false);
}
constexpr int DPP_ROW_SHR = 0x110, DPP_ROW_BCAST15 = 0x142, DPP_ROW_BCAST31 = 0x143;
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
    v += dpp_or_zero<DPP_ROW_SHR + 1, 0xf>(v);
    v += dpp_or_zero<DPP_ROW_SHR + 2, 0xf>(v);
    v += dpp_or_zero<DPP_ROW_SHR + 4, 0xf>(v);
    v += dpp_or_zero<DPP_ROW_SHR + 8, 0xf>(v);
    v += dpp_or_zero<DPP_ROW_BCAST15, 0xa>(v);
    v += dpp_or_zero<DPP_ROW_BCAST31, 0xc>(v);
    return v;
}

}  // namespace exa
