// ssd_table.hip.h — the integer SSD of many small images against many small images on the int8 matrix cores (stage_ssd_table.hip):
// the engine under the direct page look-up (frames x pages, stage_direct.hip) and the gate reference ANCHOR (frames x frames,
// stage_gate_anchor.hip).
//
//   direct_centre_kernel<WEIGHTED, STORE>  small images (any byte alignment) -> the centred i8 operand + |x'|^2 per image; WEIGHTED:
//                         under the gate's byte weights, the operand zero at the masked bytes and the norm over the valid ones;
//                         STORE false: the norms alone (the pages' masked norms)
//   page_ssd_kernel       <a', b'> of every row of a with every row of b on v_mfma_i32_32x32x32_i8, split over K, the partial sums
//                         added to i64 with non-returning vector atomics
//   frame_gram_kernel     the symmetric case, <a'_i, a'_j> for i < j alone
//
// With every byte centred, x' = x - 128 (one XOR 0x80), sum (a - b)^2 = |a'|^2 + |b'|^2 - 2 <a', b'> is exact in integers; with one
// operand zero at the masked bytes and the norms over the valid ones the same expression is the SSD over the valid bytes.
// Operand layout, both sides: a [rows_pad][kp] i8 matrix, rows_pad a multiple of SSD_TILE, kp of SSD_KGRAN, zero (the
// centred zero) behind a row's last byte and in the pad rows, stored as the MFMA reads it: per 32-row tile and 32-byte K step one
// 1 KiB block, the 16 bytes K = 32 s + 16 h .. of row r at uint4 index (tile * kp / 32 + s) * 64 + h * 32 + r.  A wave's operand
// load is then ONE contiguous KiB, lane l its own 16 bytes; which 16 of a step's 32 K values a lane half holds does not matter
// to a sum over K as long as both operands agree.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace slideo {

constexpr int SSD_BLOCK = 256;
constexpr int SSD_TILE = 64;               // rows of either operand per wave: 2 MFMA tiles
constexpr int SSD_KGRAN = 128;             // K granule: rows are padded to it, K chunks are multiples of it
constexpr int SSD_KCHUNK_MAX = 65536;      // one i32 accumulator holds 131 071 products of +-128: a wave's K chunk stays at half of that
static_assert(SSD_KGRAN == 128, "direct_centre_kernel and ssd_accumulate walk K in groups of four 32-byte steps");

typedef int ssd_v4i __attribute__((ext_vector_type(4)));
typedef int ssd_v16i __attribute__((ext_vector_type(16)));

// The 32-row tile blockIdx.x of the operand `out` (grid (rows_pad / 32, K slices), kp a multiple of SSD_KGRAN): lane l of a wave
// holds row 32 tile + (l & 31) and the half h = l >> 5 of a 32-byte K step, so a wave's store of a step is the step's ONE
// contiguous KiB, as ssd_accumulate loads it.  A wave takes groups of four consecutive steps (one 128-byte line of each of its
// rows), the groups dealt round robin over the grid's waves.  Rows < n come from the L bytes at
// src + (ofs ? ofs[row] : row * stride), the others are zero.  The source is read as ALIGNED dwords whatever its byte alignment, as
// ssd_masked_kernel reads it (v_alignbyte_b32 over the dword pair q[g], q[g + 1], q = p - (p & 3)): a 16-byte piece at K takes
// dwords K / 4 .. K / 4 + 4, whose last byte is K + 19 - (p & 3) at most, so pieces with K + 20 <= L never pass the image's end;
// q[0] begins at most 3 bytes in front of the image (inside its allocation: device buffers are 256-byte aligned).  The last
// one or two pieces are read as bytes.
// Every byte has a weight w (0xFF valid, 0x00 masked): the stored operand is (x ^ 0x80) & w, so a masked byte is the centred zero,
// and norm[row] (zeroed on the stream in front) += sum over the valid bytes of x'^2 of the pieces a wave wrote: per piece, with
// xm = x & w, sum xm^2 - 256 sum xm + 16384 * (valid bytes), the sums as 4 x u8 dot products (a masked byte adds 0 to each of the
// three; a sum of squares, so never negative); one non-returning 64-bit vector atomic per row and wave.
// WEIGHTED: w = wgt[0 .. L) (one array for all rows, 16-byte aligned, readable up to L + 4; the direct scope SLIDEO_DIRECT_VALID and
// the gate's mask scope), 0 behind L.  The weights of a 16-byte piece at K (a multiple of 16) are ONE aligned 16-byte load, taken
// where the row's dwords are (K + 20 <= L, so it ends inside L + 4); the last pieces read them as bytes.  Not WEIGHTED: wgt is never
// read; every byte is valid and a byte behind L is 128, the centred zero — it adds 128^2 - 256 * 128 + 16384 = 0 to the norm.
// STORE false: the norms alone (`out` is not touched).  No LDS.
template <bool WEIGHTED, bool STORE>
__global__ __launch_bounds__(SSD_BLOCK) void direct_centre_kernel(const uint8_t* __restrict__ src, int64_t stride, const long long* __restrict__ ofs,
                                                                  int n, int64_t L, int64_t kp, const uint8_t* __restrict__ wgt,
                                                                  uint4* __restrict__ out, unsigned long long* __restrict__ norm) {
    const int lane = threadIdx.x & 63, h = lane >> 5;
    const int r = blockIdx.x * 32 + (lane & 31);
    const int64_t steps = kp / 32;
    uint4* o = STORE ? out + (size_t)blockIdx.x * (size_t)steps * 64 + lane : nullptr;
    const int64_t groups = steps / 4;                                  // (SSD_KGRAN / 32 = 4 steps per granule)
    const int64_t g0 = (int64_t)blockIdx.y * (SSD_BLOCK / 64) + (threadIdx.x >> 6), gstep = (int64_t)gridDim.y * (SSD_BLOCK / 64);
    const bool live = r < n;
    const uint8_t* p = live ? src + (ofs ? (int64_t)ofs[r] : (int64_t)r * stride) : src;
    const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 3);
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p - sh);
    // what a byte is where none is loaded (a pad row, behind L): weight 0 — or, without weights, weight 0xFF on the centred zero
    constexpr uint32_t W0 = WEIGHTED ? 0u : 0xFFFFFFFFu, XPAD = WEIGHTED ? 0u : 0x80808080u;
    unsigned long long sq = 0;
    for (int64_t g = g0; g < groups; g += gstep) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int64_t s = g * 4 + t, c = 2 * s + h, k = c * 16;
            uint32_t x[4] = {XPAD, XPAD, XPAD, XPAD}, w[4] = {W0, W0, W0, W0};
            if (live) {
                if (k + 20 <= L) {
                    const uint32_t* d = q + c * 4;
                    const uint32_t d0 = d[0], d1 = d[1], d2 = d[2], d3 = d[3], d4 = d[4];
                    x[0] = __builtin_amdgcn_alignbyte(d1, d0, sh); x[1] = __builtin_amdgcn_alignbyte(d2, d1, sh);
                    x[2] = __builtin_amdgcn_alignbyte(d3, d2, sh); x[3] = __builtin_amdgcn_alignbyte(d4, d3, sh);
                    if constexpr (WEIGHTED) {
                        const uint4 wv = reinterpret_cast<const uint4*>(wgt)[c];
                        w[0] = wv.x; w[1] = wv.y; w[2] = wv.z; w[3] = wv.w;
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        uint32_t v = 0, u = 0;
#pragma unroll
                        for (int b = 0; b < 4; ++b) {
                            const int64_t i = k + j * 4 + b;
                            // (one meaning in two forms: written the other way round either instance takes more registers)
                            if constexpr (WEIGHTED) {
                                if (i < L) { v |= (uint32_t)p[i] << (8 * b); u |= (uint32_t)wgt[i] << (8 * b); }
                            } else {
                                v |= (uint32_t)(i < L ? p[i] : (uint8_t)128) << (8 * b);
                            }
                        }
                        x[j] = v;
                        if constexpr (WEIGHTED) w[j] = u;
                    }
                }
                uint32_t s2 = 0, s1 = 0, nv = WEIGHTED ? 0u : 16u;     // (16 bytes: at most 16 * 65 025, 16 * 255 and 16)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t xm = x[j] & w[j];
                    s2 = __builtin_amdgcn_udot4(xm, xm, s2, false);
                    s1 = __builtin_amdgcn_udot4(xm, 0x01010101u, s1, false);
                    if constexpr (WEIGHTED) nv = __builtin_amdgcn_udot4(w[j] & 0x01010101u, 0x01010101u, nv, false);
                }
                sq += s2 + 16384u * nv - 256u * s1;
            }
            if constexpr (STORE)
                o[(size_t)s * 64] = make_uint4((x[0] ^ 0x80808080u) & w[0], (x[1] ^ 0x80808080u) & w[1], (x[2] ^ 0x80808080u) & w[2],
                                               (x[3] ^ 0x80808080u) & w[3]);
        }
    }
    sq += __shfl_xor(sq, 32);
    if (live && h == 0) (void)__hip_atomic_fetch_add(norm + r, sq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct SsdAcc { ssd_v16i c00, c01, c10, c11; };

// nsteps 32-byte K steps of the 64 x 64 tile: rows a0 (32-row tile), a0 + rstride (the next one) against columns b0, b0 + rstride.
// Four K steps per iteration (nsteps is a multiple of SSD_KGRAN / 32 = 4) in two pairs whose operand registers take turns: pair y is
// loaded in front of pair x's eight MFMAs, the next iteration's pair x in front of pair y's, so a wave always has eight 16-byte
// loads in flight while it multiplies and no register is copied.  Behind the chunk's last pair the loads repeat the iteration's own
// first pair (in bounds, unused).  Per K step: four contiguous 1 KiB loads, four v_mfma_i32_32x32x32_i8.
// DIAG: the row and column tiles are the same — their operand KiB are loaded ONCE, and the product below the diagonal (c10) is not
// computed.
template <bool DIAG>
__device__ __forceinline__ void ssd_accumulate(const uint4* __restrict__ a0, const uint4* __restrict__ b0, size_t rstride, int nsteps, SsdAcc& c) {
    const uint4* a1 = a0 + rstride;
    const uint4* b1 = b0 + rstride;
    struct Pair { uint4 a0, a1, a2, a3, b0, b1, b2, b3; };
    auto ld = [&](int s) {
        const size_t o = (size_t)s * 64;
        Pair p;
        p.a0 = a0[o]; p.a1 = a1[o]; p.a2 = a0[o + 64]; p.a3 = a1[o + 64];
        if constexpr (DIAG) { p.b0 = p.a0; p.b1 = p.a1; p.b2 = p.a2; p.b3 = p.a3; }
        else { p.b0 = b0[o]; p.b1 = b1[o]; p.b2 = b0[o + 64]; p.b3 = b1[o + 64]; }
        return p;
    };
    auto mac = [](ssd_v16i& acc, const uint4& u, const uint4& v) {
        const ssd_v4i x = {(int)u.x, (int)u.y, (int)u.z, (int)u.w}, y = {(int)v.x, (int)v.y, (int)v.z, (int)v.w};
        acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(x, y, acc, 0, 0, 0);
    };
    auto mul = [&](const Pair& p) {
        mac(c.c00, p.a0, p.b0);
        mac(c.c01, p.a0, p.b1);
        if constexpr (!DIAG) mac(c.c10, p.a1, p.b0);
        mac(c.c11, p.a1, p.b1);
        mac(c.c00, p.a2, p.b2);
        mac(c.c01, p.a2, p.b3);
        if constexpr (!DIAG) mac(c.c10, p.a3, p.b2);
        mac(c.c11, p.a3, p.b3);
    };
    Pair x = ld(0);
    for (int s = 0; s < nsteps; s += 4) {
        const Pair y = ld(s + 2);
        __builtin_amdgcn_sched_barrier(0);                             // (the loads stay in front of the other pair's MFMAs)
        mul(x);
        __builtin_amdgcn_sched_barrier(0);
        x = ld(s + 4 < nsteps ? s + 4 : s);
        __builtin_amdgcn_sched_barrier(0);
        mul(y);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// dot[i * np + j] += sum over this block's K chunk of a'[i][k] * b'[j][k], i < n rows of a, j < np rows of b.
// grid (ceil(n / 128), ceil(np / 128), K chunks), block 256: wave w holds the 64 x 64 tile of row tile 2 x + (w & 1) and column
// tile 2 y + (w >> 1) — 2 x 2 MFMA tiles, 64 accumulator registers — so every operand KiB a wave loads is loaded by one other
// wave of its block too (L1).  kchunk: a multiple of SSD_KGRAN, at most SSD_KCHUNK_MAX, so an accumulator stays inside +-2^30 and
// is drained once, at the end, with one non-returning 64-bit vector atomic per element (`dot` is zeroed on the stream in front;
// two's complement: the order of the adds does not matter).  An atomic instruction covers two 256-byte row segments of dot.
// No LDS, no barrier: waves whose tile lies outside n x np leave at once.
// SYM (b == a, np == n): the entries with i < j alone; the others are never written.  A wave whose tile lies wholly below the
// diagonal (column tile < row tile) leaves at once; a diagonal tile loads its operand once and skips c10.
template <bool SYM>
__device__ __forceinline__ void ssd_table_tile(const uint4* __restrict__ a, int n, const uint4* __restrict__ b, int np, int64_t kp, int64_t kchunk,
                                               unsigned long long* __restrict__ dot) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int rt = blockIdx.x * 2 + (w & 1), ct = blockIdx.y * 2 + (w >> 1);
    if (rt * SSD_TILE >= n || ct * SSD_TILE >= np || (SYM && ct < rt)) return;
    const int64_t steps = kp / 32;
    const int64_t s0 = (int64_t)blockIdx.z * (kchunk / 32);
    const int64_t s1 = s0 + kchunk / 32 < steps ? s0 + kchunk / 32 : steps;
    const int nsteps = (int)(s1 - s0);                                 // (at most SSD_KCHUNK_MAX / 32; a multiple of SSD_KGRAN / 32 = 4)
    if (nsteps < 4) return;
    const size_t rstride = (size_t)steps * 64;                         // uint4s of one 32-row tile
    const uint4* a0 = a + ((size_t)(2 * rt) * (size_t)steps + (size_t)s0) * 64 + lane;
    const uint4* b0 = b + ((size_t)(2 * ct) * (size_t)steps + (size_t)s0) * 64 + lane;
    SsdAcc c;
    c.c00 = ssd_v16i{0}; c.c01 = ssd_v16i{0}; c.c10 = ssd_v16i{0}; c.c11 = ssd_v16i{0};
    const bool diag = SYM && rt == ct;                                 // (wave-uniform)
    if (diag) ssd_accumulate<true>(a0, b0, rstride, nsteps, c);
    else ssd_accumulate<false>(a0, b0, rstride, nsteps, c);
    // C / D: column (B's row) = lane & 31, row (A's) = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    const int col = lane & 31, rbase = 4 * (lane >> 5);
    auto drain = [&](const ssd_v16i& v, int rx, int cy) {
        const int j = ct * SSD_TILE + cy * 32 + col;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int i = rt * SSD_TILE + rx * 32 + (reg & 3) + 8 * (reg >> 2) + rbase;
            if ((SYM ? i < j : i < n) && j < np)
                (void)__hip_atomic_fetch_add(dot + (size_t)i * np + j, (unsigned long long)(long long)v[reg], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    };
    drain(c.c00, 0, 0); drain(c.c01, 0, 1);
    if (!diag) drain(c.c10, 1, 0);
    drain(c.c11, 1, 1);
}

// every frame (a, n rows) against every page of the class (b, np rows)
__global__ __launch_bounds__(SSD_BLOCK, 2) void page_ssd_kernel(const uint4* __restrict__ a, int n, const uint4* __restrict__ b, int np, int64_t kp,
                                                                int64_t kchunk, unsigned long long* __restrict__ dot) {
    ssd_table_tile<false>(a, n, b, np, kp, kchunk, dot);
}

// a unit's frames against each other, i < j
__global__ __launch_bounds__(SSD_BLOCK, 2) void frame_gram_kernel(const uint4* __restrict__ a, int n, int64_t kp, int64_t kchunk,
                                                                  unsigned long long* __restrict__ dot) {
    ssd_table_tile<true>(a, n, a, n, kp, kchunk, dot);
}

}  // namespace slideo
