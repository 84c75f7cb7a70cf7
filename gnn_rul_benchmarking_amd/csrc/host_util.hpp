// Host-side plumbing the family drivers share, next to launch.hpp: the return-on-error macro, the workspace carver
// and its typed read-back, the dropout constants and the "resident rows" clamp.  Host only: nothing here is compiled for the device.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "launch.hpp"

// Evaluate the call once; leave the enclosing function with its code unless that is RULGNN_OK.  (Variadic: a call may carry the commas
// of a template argument list.)
#define RULGNN_TRY(...)                    \
    do {                                   \
        const int rc_ = (__VA_ARGS__);     \
        if (rc_ != RULGNN_OK) return rc_;  \
    } while (0)

namespace rulgnn {

// Every workspace region starts on a 256-byte boundary.
inline size_t ws_align(size_t v) { return (v + 255) & ~(size_t)255; }

// Carves a workspace into regions: each take returns the region's byte offset and moves the running offset to the next 256-byte
// boundary behind it.  The family *Ws structs keep the offsets under their names; total() is the size the workspace query reports.
struct WsCarver {
    size_t o = 0;
    size_t take_bytes(size_t n) {
        const size_t at = o;
        o = ws_align(o + n);
        return at;
    }
    template <typename T>
    size_t take(size_t count) {
        return take_bytes(count * sizeof(T));
    }
    size_t total() const { return o; }
};

// The caller's workspace, read back by the offsets a WsCarver handed out: ws.at<float>(w.cat).
struct Workspace {
    char* base;
    explicit Workspace(void* p) : base(static_cast<char*>(p)) {}
    template <typename T>
    T* at(size_t off) const {
        return reinterpret_cast<T*>(base + off);
    }
};

// Inverted dropout with probability p as the kernels apply it: drop where the 32-bit counter hash is below `thr` = round(p * 2^32)
// (at most 2^32 - 1), scale the kept values by 1 / (1 - p).  p <= 0 drops nothing.  oracle/stgcn_oracle.py restates it bit for bit.
struct DropoutConst {
    uint32_t thr;
    float scale;
};
inline DropoutConst dropout_const(float p) {
    if (!(p > 0.f)) return {0u, 1.0f};
    const uint64_t ti = (uint64_t)((double)p * 4294967296.0 + 0.5);
    return {ti > 4294967295ull ? 4294967295u : (uint32_t)ti, 1.0f / (1.0f - p)};
}

// Rows of a grid-strided launch that writes one partial-gradient row per workgroup: what is co-resident (residency), at most `items`
// and at most `cap`, at least 1.  `items` and `cap` stay the caller's own: they fix the number of partial rows, and so the bits.
template <typename K>
inline int resident_rows(K kernel, int block, size_t lds, int64_t items, int64_t cap) {
    const Residency r = residency(kernel, block, lds);
    int64_t want = (int64_t)r.cus * r.per_cu;
    if (want > items) want = items;
    if (want > cap) want = cap;
    return want < 1 ? 1 : (int)want;
}

}  // namespace rulgnn
