// frame_list.hip.h — the planes of a DEVICE frame list gathered into the library's own staged layout (include/slideo_amd.h "Frame
// lists"; the layout: frame_settings.h FrameListPlan, the same a host list's copies fill).
//
//   frame_gather_kernel   every plane of every frame of a unit, one launch   (HBM: the frames' bytes in, the same out)
// Launched for device lists alone (stage_orb.hip launch_frame_gather).  No arithmetic: bytes move.  No LDS, no atomics.
// Grid (row chunks, staged planes, frames), block GATHER_TX x GATHER_TY = 64 lanes along a row x 4 rows: a wave is one row at a time,
// a block walks the GATHER_ROWS rows of its chunk.  The block's plane address comes out of the pointer table (3 addresses per frame,
// device memory) and its stride, rows and row bytes out of the arguments: all uniform over the block, scalar loads.
// Per row the path is chosen from the row's source and destination addresses, uniform over the wave:
//   16   the two are congruent mod 16: up to 15 head bytes, to the next 16-byte boundary of the source, by bytes (lane x moves byte
//        x); then 16-byte loads and stores, lanes 64 units apart; then the ragged tail of up to 15 bytes by bytes
//   4    congruent mod 4 only: the same with dwords (head and tail up to 3 bytes)
//   1    else: bytes, lanes 64 apart
// The usual sizes (row bytes and plane sizes multiples of 16, as 1920x1080 has them) stage every plane at a 16-byte aligned base with
// 16-byte aligned rows, so an aligned source takes path 16 throughout; the tight layout of an odd size does not, and pays by path.
// Hard rules: no multi-byte load or store at an address that is not a multiple of its size (head and tail are single bytes of
// different lanes: nothing the vectoriser could merge); no byte outside [row start, row start + row bytes) of a source row is read.
// The per-thread body is a host + device function: tools/frame_list_hostcheck.cpp runs it lane by lane on the CPU.
#pragma once
#include <cstdint>

#include "frame_settings.h"
#include "slideo_amd.h"

namespace slideo {

constexpr int GATHER_TX = 64, GATHER_TY = 4, GATHER_ROWS = 16;       // a block: 64 lanes x 4 rows, 16 rows per chunk

#if defined(__HIPCC__)
#define GATHER_HD __host__ __device__ __forceinline__
#else
#define GATHER_HD inline
#endif

struct GatherArgs {
    const uint8_t* const* tab;       // frame i's three plane addresses at tab[3i .. 3i + 2] (device memory; the host check: host)
    uint8_t* dst;                    // staged frames, dst_frame_stride apart
    int64_t dst_frame_stride;
    int n_planes;
    int k[3], rows[3];               // per staged plane: which of the frame's addresses, rows
    int row_bytes[3];
    int64_t src_stride[3], dst_ofs[3];
};

// the tally of the host check: rows by path, rows with head bytes, rows with a ragged tail
struct GatherTally { unsigned long long rows16 = 0, rows4 = 0, rows1 = 0, heads = 0, tails = 0; };

inline GatherArgs frame_gather_args(const FrameListPlan& P, const uint8_t* const* tab, uint8_t* dst) {
    GatherArgs a{};
    a.tab = tab; a.dst = dst; a.dst_frame_stride = P.frame_bytes; a.n_planes = P.n_planes;
    for (int j = 0; j < 3; ++j) {
        a.k[j] = P.k[j]; a.rows[j] = P.rows[j]; a.row_bytes[j] = (int)P.row_bytes[j];
        a.src_stride[j] = P.src_stride[j]; a.dst_ofs[j] = P.dst_ofs[j];
    }
    return a;
}
inline int frame_gather_chunks(const GatherArgs& a) {
    int rows = 0;
    for (int j = 0; j < a.n_planes; ++j) rows = a.rows[j] > rows ? a.rows[j] : rows;
    return (rows + GATHER_ROWS - 1) / GATHER_ROWS;
}

// the 16-byte unit (the host build's sanitizer checks its alignment as it checks the dword's)
struct alignas(16) GatherQuad { uint32_t x, y, z, w; };

// One thread of the launch grid: lane tx of thread row ty, chunk `chunk` of staged plane j of frame z
GATHER_HD void frame_gather_thread(const GatherArgs& a, int chunk, int j, int z, int tx, int ty, GatherTally* tally) {
    if (j >= a.n_planes) return;
    const uint8_t* sbase = a.tab[3 * (int64_t)z + a.k[j]];
    uint8_t* dbase = a.dst + (int64_t)z * a.dst_frame_stride + a.dst_ofs[j];
    const int rb = a.row_bytes[j], rows = a.rows[j];
    const int64_t ss = a.src_stride[j];
    const int r1 = chunk * GATHER_ROWS + GATHER_ROWS < rows ? chunk * GATHER_ROWS + GATHER_ROWS : rows;
    for (int row = chunk * GATHER_ROWS + ty; row < r1; row += GATHER_TY) {
        const uint8_t* s = sbase + (int64_t)row * ss;
        uint8_t* d = dbase + (int64_t)row * rb;
        const uintptr_t rel = (uintptr_t)s - (uintptr_t)d;
        const int unit = (rel & 15) == 0 ? 16 : (rel & 3) == 0 ? 4 : 1;
        if (unit == 1) {
            for (int x = tx; x < rb; x += GATHER_TX) d[x] = s[x];
            if (tally && tx == 0) ++tally->rows1;
            continue;
        }
        int head = (int)((0 - (uintptr_t)s) & (uintptr_t)(unit - 1));
        if (head > rb) head = rb;
        const int body = (rb - head) / unit, tail = rb - head - body * unit;
        if (tx < head) d[tx] = s[tx];
        const uint8_t* sb = s + head;
        uint8_t* db = d + head;
        if (unit == 16) {
            for (int u = tx; u < body; u += GATHER_TX)
                reinterpret_cast<GatherQuad*>(db)[u] = reinterpret_cast<const GatherQuad*>(sb)[u];
        } else {
            for (int u = tx; u < body; u += GATHER_TX)
                reinterpret_cast<uint32_t*>(db)[u] = reinterpret_cast<const uint32_t*>(sb)[u];
        }
        if (tx < tail) db[body * unit + tx] = sb[body * unit + tx];
        if (tally && tx == 0) {
            ++(unit == 16 ? tally->rows16 : tally->rows4);
            tally->heads += head > 0; tally->tails += tail > 0;
        }
    }
}

#if defined(__HIPCC__)
// grid (frame_gather_chunks, n_planes, n), block (GATHER_TX, GATHER_TY)
__global__ __launch_bounds__(GATHER_TX * GATHER_TY) void frame_gather_kernel(GatherArgs a) {
    frame_gather_thread(a, blockIdx.x, blockIdx.y, blockIdx.z, threadIdx.x, threadIdx.y, nullptr);
}
#endif

}  // namespace slideo
