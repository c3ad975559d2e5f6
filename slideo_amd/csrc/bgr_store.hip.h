// bgr_store.hip.h — the store of the kernels whose thread owns four consecutive BGR8 pixels of a destination row (reduce.hip.h,
// frame_region.hip.h).  Host + device, as frame_region.hip.h's thread body is.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BGR_HD __host__ __device__ __forceinline__
#else
#define BGR_HD inline
#endif

namespace slideo {

// `cnt` pixels (b | g << 8 | r << 16 each) to d: 3 dwords when all 4 are there and d is dword-aligned, bytes otherwise
BGR_HD void bgr_store4(uint8_t* d, const uint32_t (&p)[4], int cnt, bool dwords) {
    if (dwords && cnt == 4) {
        uint32_t* q = reinterpret_cast<uint32_t*>(d);
        q[0] = p[0] | (p[1] << 24);                   // b0 g0 r0 b1
        q[1] = (p[1] >> 8) | (p[2] << 16);            // g1 r1 b2 g2
        q[2] = (p[2] >> 16) | (p[3] << 8);            // r2 b3 g3 r3
        return;
    }
    for (int i = 0; i < cnt; ++i) { d[3 * i] = (uint8_t)p[i]; d[3 * i + 1] = (uint8_t)(p[i] >> 8); d[3 * i + 2] = (uint8_t)(p[i] >> 16); }
}

}  // namespace slideo
