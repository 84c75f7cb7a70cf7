// Host-side launch plumbing every translation unit shares: the opt-in to more than 48 KB of dynamic LDS and the "CU count x occupancy"
// query behind the persistent grids.  Host only; the clamps (tile counts, max_grid, oversubscription, overrides) stay with the callers,
// because the grid fixes the number of partial-gradient rows and with it the bits of the results.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/rulgnn.h"

namespace rulgnn {

constexpr size_t MAX_LDS_BYTES = 160 * 1024;        // LDS of one gfx950 compute unit: the most one workgroup can ask for
constexpr size_t DEFAULT_LDS_BYTES = 48 * 1024;     // what a kernel may request without raising its attribute

// Call before a launch that requests `bytes` of dynamic LDS.  RULGNN_EUNSUPPORTED (nothing touched) above `cap`, RULGNN_EHIP when the
// runtime refuses the raise.  The attribute belongs to one kernel on one device, so the raise is asked of the runtime on every call for
// the kernel and the current device: any memo would have to be keyed by (kernel address, device), never by the kernel's type -- kernels
// that differ only in template arguments share their pointer type -- and never process-wide.
[[nodiscard]] inline int allow_dynamic_lds(const void* kernel, size_t bytes, size_t cap = MAX_LDS_BYTES) {
    if (bytes > cap) return RULGNN_EUNSUPPORTED;
    if (bytes > DEFAULT_LDS_BYTES && hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess)
        return RULGNN_EHIP;
    return RULGNN_OK;
}
template <typename... A>
[[nodiscard]] inline int allow_dynamic_lds(void (*kernel)(A...), size_t bytes, size_t cap = MAX_LDS_BYTES) {
    return allow_dynamic_lds(reinterpret_cast<const void*>(kernel), bytes, cap);
}

// The one way to launch a kernel (with launch_checked_ev, aux_stream.hpp): drop any stale error of the caller's earlier HIP calls, launch,
// report this launch's own error.  Every launch's status is checked (RULGNN_TRY) or returned; [[nodiscard]] and -Werror=unused-result hold
// the callers to it, tests/test_launch_sites_cpu.py keeps raw launches out of the other files.  The arguments convert to the kernel's
// parameter types at the launch; a kernel's default arguments do not exist behind the pointer and have to be passed.
template <typename... P, typename... A>
[[nodiscard]] inline int launch_checked(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t stream, const A&... args) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(kernel, grid, block, lds, stream, args...);
    return hipGetLastError() == hipSuccess ? RULGNN_OK : RULGNN_EHIP;
}

// Compute units of the current device; 256 when the query fails (`ok`, if given, says whether it succeeded).
inline int device_cu_count(bool* ok = nullptr) {
    int dev = 0, v = 0;
    const bool got = hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0;
    if (ok) *ok = got;
    return got ? v : 256;
}

// What is co-resident: the device's CU count and the workgroups of (kernel, block, lds) one CU holds.  A failed or empty occupancy
// answer counts as one workgroup per CU, a failed device query as 256 CUs -- unless `strict` (launches that need every workgroup
// resident, such as cooperative ones): then a failed query is RULGNN_EHIP and per_cu < 1 RULGNN_EUNSUPPORTED.
struct Residency {
    int cus, per_cu;
};
inline int residency(const void* kernel, int block, size_t lds, Residency* r, bool strict = false) {
    bool cus_ok = false;
    r->cus = device_cu_count(&cus_ok);
    r->per_cu = 0;
    if (strict && !cus_ok) return RULGNN_EHIP;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&r->per_cu, kernel, block, lds) != hipSuccess || r->per_cu < 1) {
        if (strict) return RULGNN_EUNSUPPORTED;
        r->per_cu = 1;
    }
    return RULGNN_OK;
}
template <typename... A>
inline Residency residency(void (*kernel)(A...), int block, size_t lds) {
    Residency r;
    (void)residency(reinterpret_cast<const void*>(kernel), block, lds, &r);
    return r;
}

}  // namespace rulgnn
