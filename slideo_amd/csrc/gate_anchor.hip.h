// gate_anchor.hip.h — kernels of the gate reference SLIDEO_GATE_ANCHOR (stage_gate_anchor.hip; include/slideo_amd.h "Gate reference").
//
//   frame_gram_kernel         <a'_i, a'_j> of a unit's frames for i < j on v_mfma_i32_32x32x32_i8: page_ssd_kernel's symmetric case on
//                             the same centred operand (direct.hip.h: layout, K granule, the i32 accumulator's K chunk)
//   gate_anchor_kernel        one wave walks the table: a frame is compared with the last flagged frame before it
//   gate_anchor_state_kernel  the unit's last anchor's small image -> the gate state
//
// sum (a - b)^2 = |a'|^2 + |b'|^2 - 2 <a', b'> with x' = x - 128, exact in integers; under the gate's weights the operand is zero at
// the masked bytes and the norms run over the valid ones, so the same expression is the SSD over the valid bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace slideo {

constexpr int GRAM_BLOCK = 256;
constexpr int GRAM_TILE = 64;              // rows per wave on either side: 2 MFMA tiles (direct.hip.h DIRECT_TILE)
constexpr int GRAM_KGRAN = 128;            // K granule of the operand (DIRECT_KGRAN)
constexpr int GRAM_KCHUNK_MAX = 65536;     // a wave's K chunk: 65 536 products of at most 2^14 stay inside +-2^30 (DIRECT_KCHUNK_MAX)
constexpr int ANCHOR_STATE_BLOCK = 256;

typedef int gram_v4i __attribute__((ext_vector_type(4)));
typedef int gram_v16i __attribute__((ext_vector_type(16)));

struct GramAcc { gram_v16i c00, c01, c10, c11; };

// nsteps 32-byte K steps of the 64 x 64 tile: rows a0 (32-row tile), a0 + rstride (the next one) against columns b0, b0 + rstride.
// page_ssd_kernel's loop: four K steps per iteration in two pairs whose operand registers take turns, so a wave always has loads in
// flight while it multiplies.  DIAG: the row and column tiles are the same — their operand KiB are loaded ONCE, and the product
// below the diagonal (c10) is not computed.
template <bool DIAG>
__device__ __forceinline__ void gram_accumulate(const uint4* __restrict__ a0, const uint4* __restrict__ b0, size_t rstride, int nsteps, GramAcc& c) {
    const uint4* a1 = a0 + rstride;
    const uint4* b1 = b0 + rstride;
    struct Pair { uint4 a0, a1, a2, a3, b0, b1, b2, b3; };
    auto ld = [&](int s) {
        const size_t o = (size_t)s * 64;
        Pair p;
        p.a0 = a0[o]; p.a1 = a1[o]; p.a2 = a0[o + 64]; p.a3 = a1[o + 64];
        if (DIAG) { p.b0 = p.a0; p.b1 = p.a1; p.b2 = p.a2; p.b3 = p.a3; }
        else { p.b0 = b0[o]; p.b1 = b1[o]; p.b2 = b0[o + 64]; p.b3 = b1[o + 64]; }
        return p;
    };
    auto v4 = [](const uint4& u) { const gram_v4i v = {(int)u.x, (int)u.y, (int)u.z, (int)u.w}; return v; };
    auto mul = [&](const Pair& p) {
        c.c00 = __builtin_amdgcn_mfma_i32_32x32x32_i8(v4(p.a0), v4(p.b0), c.c00, 0, 0, 0);
        c.c01 = __builtin_amdgcn_mfma_i32_32x32x32_i8(v4(p.a0), v4(p.b1), c.c01, 0, 0, 0);
        if (!DIAG) c.c10 = __builtin_amdgcn_mfma_i32_32x32x32_i8(v4(p.a1), v4(p.b0), c.c10, 0, 0, 0);
        c.c11 = __builtin_amdgcn_mfma_i32_32x32x32_i8(v4(p.a1), v4(p.b1), c.c11, 0, 0, 0);
        c.c00 = __builtin_amdgcn_mfma_i32_32x32x32_i8(v4(p.a2), v4(p.b2), c.c00, 0, 0, 0);
        c.c01 = __builtin_amdgcn_mfma_i32_32x32x32_i8(v4(p.a2), v4(p.b3), c.c01, 0, 0, 0);
        if (!DIAG) c.c10 = __builtin_amdgcn_mfma_i32_32x32x32_i8(v4(p.a3), v4(p.b2), c.c10, 0, 0, 0);
        c.c11 = __builtin_amdgcn_mfma_i32_32x32x32_i8(v4(p.a3), v4(p.b3), c.c11, 0, 0, 0);
    };
    Pair x = ld(0);
    for (int s = 0; s < nsteps; s += 4) {          // (nsteps is a multiple of 4: behind the last pair the loads repeat the iteration's own first pair)
        const Pair y = ld(s + 2);
        __builtin_amdgcn_sched_barrier(0);
        mul(x);
        __builtin_amdgcn_sched_barrier(0);
        x = ld(s + 4 < nsteps ? s + 4 : s);
        __builtin_amdgcn_sched_barrier(0);
        mul(y);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// dot[i * n + j] += sum over this block's K chunk of a'[i][k] * a'[j][k] for i < j < n; the entries with i >= j are never written.
// a: the centred operand of the n frames ([rows_pad][kp], rows_pad a multiple of GRAM_TILE, direct.hip.h's layout).
// grid (ceil(n / 128), ceil(n / 128), K chunks), block 256: wave w holds the 64 x 64 tile of row tile 2 x + (w & 1) and column tile
// 2 y + (w >> 1).  A wave whose tile lies outside n x n or wholly below the diagonal (column tile < row tile) leaves at once; a
// diagonal tile loads its operand once.  kchunk: a multiple of GRAM_KGRAN, at most GRAM_KCHUNK_MAX, so an i32 accumulator stays
// inside +-2^30 and is drained once, with one non-returning 64-bit vector atomic per element (`dot` is zeroed on the stream in
// front; two's complement: the order of the adds does not matter).  No LDS, no barrier.
__global__ __launch_bounds__(GRAM_BLOCK, 2) void frame_gram_kernel(const uint4* __restrict__ a, int n, int64_t kp, int64_t kchunk,
                                                                   unsigned long long* __restrict__ dot) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int rt = blockIdx.x * 2 + (w & 1), ct = blockIdx.y * 2 + (w >> 1);
    if (rt * GRAM_TILE >= n || ct * GRAM_TILE >= n || ct < rt) return;
    const int64_t steps = kp / 32;
    const int64_t s0 = (int64_t)blockIdx.z * (kchunk / 32);
    const int64_t s1 = s0 + kchunk / 32 < steps ? s0 + kchunk / 32 : steps;
    const int nsteps = (int)(s1 - s0);                                 // (at most GRAM_KCHUNK_MAX / 32; a multiple of GRAM_KGRAN / 32 = 4)
    if (nsteps < 4) return;
    const size_t rstride = (size_t)steps * 64;                         // uint4s of one 32-row tile
    const uint4* a0 = a + ((size_t)(2 * rt) * (size_t)steps + (size_t)s0) * 64 + lane;
    const uint4* b0 = a + ((size_t)(2 * ct) * (size_t)steps + (size_t)s0) * 64 + lane;
    GramAcc c;
    c.c00 = gram_v16i{0}; c.c01 = gram_v16i{0}; c.c10 = gram_v16i{0}; c.c11 = gram_v16i{0};
    const bool diag = rt == ct;                                        // (wave-uniform)
    if (diag) gram_accumulate<true>(a0, b0, rstride, nsteps, c);
    else gram_accumulate<false>(a0, b0, rstride, nsteps, c);
    // C / D: column (B's row) = lane & 31, row (A's) = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    const int col = lane & 31, rbase = 4 * (lane >> 5);
    auto drain = [&](const gram_v16i& v, int rx, int cy) {
        const int j = ct * GRAM_TILE + cy * 32 + col;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int i = rt * GRAM_TILE + rx * 32 + (reg & 3) + 8 * (reg >> 2) + rbase;
            if (i < j && j < n)
                (void)__hip_atomic_fetch_add(dot + (size_t)i * n + j, (unsigned long long)(long long)v[reg], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    };
    drain(c.c00, 0, 0); drain(c.c01, 0, 1);
    if (!diag) drain(c.c10, 1, 0);
    drain(c.c11, 1, 1);
}

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
