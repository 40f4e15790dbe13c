// Host-side plumbing shared by the library's C ABIs (include/exa_*.h): error text, launch checks, sizes.
//
// Every ABI keeps its own thread-local message buffer -- what its *_last_error() returns -- so that a failing call of
// one ABI leaves the others' messages alone (autograd runs backward on its own thread, hence thread-local).  One line,
// EXA_ABI_STATUS("exa_knn"), in an ABI's source defines that buffer and the three functions the source reports with:
//   fail(code, what)      "exa_knn: <what>", returns code
//   fail_hip(e, where)    "exa_knn: HIP error <e> (<text>) in <where>", returns (int)e
//   launched(kernel)      0, or fail_hip() of hipGetLastError() for the kernel just enqueued
// An ABI spread over several sources, every stage's entry points next to its kernels, defines the buffer in one of them and
// says EXA_ABI_STATUS_SHARED(...) in the others, inside the same named namespace: exa_mesh (exa_mesh_impl; the buffer is
// mesh_raster.hip's) and exa_raster (exa_raster_impl; the buffer is api.hip's).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

namespace exa {

constexpr int ABI_ERR_BYTES = 512;

inline int abi_fail(char (&err)[ABI_ERR_BYTES], const char* abi, int code, const char* what) {
    snprintf(err, sizeof(err), "%s: %s", abi, what);
    return code;
}

inline int abi_fail_hip(char (&err)[ABI_ERR_BYTES], const char* abi, hipError_t e, const char* where) {
    snprintf(err, sizeof(err), "%s: HIP error %d (%s) in %s", abi, (int)e, hipGetErrorString(e), where);
    return (int)e;
}

// workspace sections start on 256-byte boundaries (also used by the raster core's device-side carving, common.h)
__host__ __device__ inline uint64_t align256(uint64_t v) { return (v + 255) & ~uint64_t(255); }

// workgroups of `block` threads that cover n items
inline unsigned ceil_div(int64_t n, int64_t block) { return (unsigned)((n + block - 1) / block); }

}  // namespace exa

#define EXA_ABI_STATUS(ABI)                                                                                            \
    thread_local char g_err[exa::ABI_ERR_BYTES] = "";                                                                  \
    EXA_ABI_STATUS_FUNCTIONS(ABI)

// A second source of the same ABI (same namespace): the buffer is the first source's, the three functions are the same.
#define EXA_ABI_STATUS_SHARED(ABI)                                                                                     \
    extern thread_local char g_err[exa::ABI_ERR_BYTES];                                                                \
    EXA_ABI_STATUS_FUNCTIONS(ABI)

#define EXA_ABI_STATUS_FUNCTIONS(ABI)                                                                                  \
    inline int fail(int code, const char* what) { return exa::abi_fail(g_err, ABI, code, what); }                      \
    inline int fail_hip(hipError_t e, const char* where) { return exa::abi_fail_hip(g_err, ABI, e, where); }           \
    inline int launched(const char* kernel) {                                                                          \
        const hipError_t e = hipGetLastError();                                                                        \
        return e == hipSuccess ? 0 : fail_hip(e, kernel);                                                              \
    }
