// gate_anchor.hip.h — kernels of the gate reference SLIDEO_GATE_ANCHOR (stage_gate_anchor.hip; include/slideo_amd.h "Gate reference").
// The table <a'_i, a'_j> of a unit's frames, i < j, is the SSD-table engine's frame_gram_kernel (ssd_table.hip.h).
//
//   gate_anchor_kernel        one wave walks the table: a frame is compared with the last flagged frame before it
//   gate_anchor_state_kernel  the unit's last anchor's small image -> the gate state
//
// sum (a - b)^2 = |a'|^2 + |b'|^2 - 2 <a', b'> with x' = x - 128, exact in integers; under the gate's weights the operand is zero at
// the masked bytes and the norms run over the valid ones, so the same expression is the SSD over the valid bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace slideo {

constexpr int ANCHOR_STATE_BLOCK = 256;

// One wave.  The anchor rule over a unit of n frames: frame j is compared with the last flagged frame before it — the carried anchor
// (the gate state: its SSDs against every frame of the unit are carried[0 .. n)) until a frame of the unit is flagged, then that
// frame a: ssd = norm[a] + norm[j] - 2 dot[a * n + j] (a < j).  changed = ssd >= thr in 64-bit integers (thr = slideo_changed_ssd_threshold;
// INT64_MAX: never); force0 (no gate state): frame 0 is changed with SSD 0 and is the first anchor.
// With anchor a and next frame i the 64 lanes test frames i .. i + 63; a ballot finds the first flagged one, f: the frames before f
// are unchanged, f is changed and becomes the anchor, the walk continues at f + 1.  Without one the 64 frames are unchanged.
// Written, with ordinary vector stores, what gate_kernel writes: flags[n], the ascending kept list idx, *count — device memory — and
// the pinned record h_head = {count, n}, h_ssd (per frame the SSD against ITS anchor), h_idx, h_flag; and *anchor_out = the last
// flagged frame of the unit, -1 when there is none.
__global__ __launch_bounds__(64) void gate_anchor_kernel(const unsigned long long* __restrict__ dot, const long long* __restrict__ norm,
                                                         const unsigned long long* __restrict__ carried, int n, long long thr, int force0,
                                                         uint8_t* __restrict__ flags, int32_t* __restrict__ idx, uint32_t* __restrict__ count,
                                                         uint32_t* __restrict__ h_head, unsigned long long* __restrict__ h_ssd,
                                                         int32_t* __restrict__ h_idx, uint8_t* __restrict__ h_flag, int32_t* __restrict__ anchor_out) {
    const int lane = threadIdx.x;
    int a = -1, i = 0;
    uint32_t k = 0;
    if (force0 && n > 0) {
        if (lane == 0) { flags[0] = 1; h_flag[0] = 1; h_ssd[0] = 0ull; idx[0] = 0; h_idx[0] = 0; }
        a = 0; i = 1; k = 1;
    }
    while (i < n) {
        const int j = i + lane;
        unsigned long long s = 0;
        bool hit = false;
        if (j < n) {
            s = a < 0 ? carried[j] : (unsigned long long)(norm[a] + norm[j] - 2ll * (long long)dot[(size_t)a * n + j]);
            hit = (long long)s >= thr;                                 // (an SSD is at most 255^2 * 3 * sw * sh: far inside int64)
        }
        const unsigned long long b = __ballot(hit);
        const int f = b ? __builtin_ctzll(b) : 64;                     // (wave-uniform)
        if (j < n && lane <= f) {
            const bool mine = lane == f;
            flags[j] = mine ? 1 : 0; h_flag[j] = mine ? 1 : 0;
            h_ssd[j] = s;
            if (mine) { idx[k] = j; h_idx[k] = j; }
        }
        if (f < 64) { a = i + f; i = a + 1; ++k; }
        else i += 64;
    }
    if (lane == 0) {
        *count = k;
        h_head[0] = k; h_head[1] = (uint32_t)n;
        *anchor_out = a;
    }
}

// state[0 .. nbytes) = the small image small + *anchor * stride; *anchor < 0: nothing is written (no frame of the unit was flagged:
// the carried anchor stays).  The source starts at ANY byte alignment and is read as ALIGNED dwords, as ssd_masked_kernel reads its
// images (v_alignbyte_b32 over q[g], q[g + 1], q = p - (p & 3)): the body stops one dword early, so q[g + 1] never passes the
// image's end, and q[0] begins at most 3 bytes in front of the image (inside the unit's buffer of small images, whose base is
// 256-byte aligned).  The 4 .. 7 ragged bytes are copied as bytes.  state: 4-byte aligned.  Any grid; block ANCHOR_STATE_BLOCK.
__global__ __launch_bounds__(ANCHOR_STATE_BLOCK) void gate_anchor_state_kernel(const uint8_t* __restrict__ small, int64_t stride,
                                                                               const int32_t* __restrict__ anchor, int64_t nbytes,
                                                                               uint8_t* __restrict__ state) {
    const int a = *anchor;
    if (a < 0) return;
    const uint8_t* p = small + (int64_t)a * stride;
    const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 3);
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p - sh);
    uint32_t* d = reinterpret_cast<uint32_t*>(state);
    const int64_t body = nbytes / 4 > 0 ? nbytes / 4 - 1 : 0;          // dwords
    const int64_t t = (int64_t)blockIdx.x * ANCHOR_STATE_BLOCK + threadIdx.x, nt = (int64_t)gridDim.x * ANCHOR_STATE_BLOCK;
    for (int64_t g = t; g < body; g += nt) d[g] = __builtin_amdgcn_alignbyte(q[g + 1], q[g], sh);
    for (int64_t b = body * 4 + t; b < nbytes; b += nt) state[b] = p[b];
}

}  // namespace slideo
