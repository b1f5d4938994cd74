// sv_pack.h — row packing of the host-buffer entry points.  Pure host code that includes
// nothing from HIP, so a stand-alone program can check it (tests/test_pack_rows.py).
#pragma once
#include <cstdint>
#include <cstring>

namespace svc {
// H rows of row_bytes bytes, `stride` bytes apart in src, back to back into dst.
inline void pack_rows(uint8_t* dst, const uint8_t* src, int H, size_t row_bytes, size_t stride) {
    if (stride == row_bytes) {
        std::memcpy(dst, src, (size_t)H * row_bytes);
        return;
    }
    for (size_t y = 0; y < (size_t)H; ++y) std::memcpy(dst + y * row_bytes, src + y * stride, row_bytes);
}
}  // namespace svc
