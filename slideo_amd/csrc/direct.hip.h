// direct.hip.h — kernels of the direct page look-up (stage_direct.hip; include/slideo_amd.h "Direct page look-up").
//
//   direct_centre_kernel  small images (any byte alignment) -> the centred i8 operand of page_ssd_kernel + |x'|^2 per image:
//                         the deck's pages once per size class, a gated unit's frames once per unit
//   direct_centre_valid_kernel  the same under the gate's byte weights (the direct scope SLIDEO_DIRECT_VALID): the frames' operand
//                         zero at the masked bytes and the norm over the valid bytes; without the store, the pages' masked norms
//   page_ssd_kernel       <a', b'> of every frame with every page of the class on v_mfma_i32_32x32x32_i8, split over K, the
//                         partial sums added to i64 with non-returning vector atomics
//   direct_best_kernel    per frame: ssd(p) = |a'|^2 + |b'|^2 - 2 <a', b'> over the eligible pages, the smallest one and the
//                         lowest page that attains it (the tap: every page's ssd)
//   direct_gate_kernel    one block, behind gate_kernel: the direct frames leave the kept list, the unit's pinned record grows
//
// With every byte centred, x' = x - 128 (one XOR 0x80), sum (a - b)^2 = |a'|^2 + |b'|^2 - 2 <a', b'> is exact in integers.
// Operand layout, both sides: a [rows_pad][kp] i8 matrix, rows_pad a multiple of DIRECT_TILE, kp of DIRECT_KGRAN, zero (the
// centred zero) behind a row's last byte and in the pad rows, stored as the MFMA reads it: per 32-row tile and 32-byte K step one
// 1 KiB block, the 16 bytes K = 32 s + 16 h .. of row r at uint4 index (tile * kp / 32 + s) * 64 + h * 32 + r.  A wave's operand
// load is then ONE contiguous KiB, lane l its own 16 bytes; which 16 of a step's 32 K values a lane half holds does not matter
// to a sum over K as long as both operands agree.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace slideo {

constexpr int DIRECT_BLOCK = 256;
constexpr int DIRECT_TILE = 64;            // rows of either operand per wave: 2 MFMA tiles
constexpr int DIRECT_KGRAN = 128;          // K granule: rows are padded to it, K chunks are multiples of it
constexpr int DIRECT_KCHUNK_MAX = 65536;   // one i32 accumulator holds 131 071 products of +-128: a wave's K chunk stays at half of that
static_assert(DIRECT_KGRAN == 128, "direct_centre_kernel and page_ssd_kernel walk K in groups of four 32-byte steps");

typedef int direct_v4i __attribute__((ext_vector_type(4)));
typedef int direct_v16i __attribute__((ext_vector_type(16)));

struct DirectBest { unsigned long long ssd; int32_t page; int32_t _pad; };

// What direct_gate_kernel appends to a gated unit's pinned record (at `rec`, 8-byte aligned behind gate_kernel's): the reduced
// kept count, then per frame the best SSD (u64), its page (i32) and the direct flag (u8; 1 only for a changed frame).
struct DirectHostRec { uint32_t kept, n; };
inline __host__ __device__ size_t direct_rec_ssd_ofs() { return 8; }
inline __host__ __device__ size_t direct_rec_page_ofs(int n) { return 8 + (size_t)n * 8; }
inline __host__ __device__ size_t direct_rec_flag_ofs(int n) { return 8 + (size_t)n * 12; }
inline __host__ __device__ size_t direct_rec_bytes(int n) { return 8 + (size_t)n * 13; }

// The 32-row tile blockIdx.x of the operand `out` (grid (rows_pad / 32, K slices), kp a multiple of DIRECT_KGRAN): lane l of a wave
// holds row 32 tile + (l & 31) and the half h = l >> 5 of a 32-byte K step, so a wave's store of a step is the step's ONE
// contiguous KiB, as page_ssd_kernel loads it.  A wave takes groups of four consecutive steps (one 128-byte line of each of its
// rows), the groups dealt round robin over the grid's waves.  Rows < n come from the L bytes at
// src + (ofs ? ofs[row] : row * stride), the others are zero.  The source is read as ALIGNED dwords whatever its byte alignment, as
// ssd_masked_kernel reads it (v_alignbyte_b32 over the dword pair q[g], q[g + 1], q = p - (p & 3)): a 16-byte piece at K takes
// dwords K / 4 .. K / 4 + 4, whose last byte is K + 19 - (p & 3) at most, so pieces with K + 20 <= L never pass the image's end;
// q[0] begins at most 3 bytes in front of the image (inside its allocation: device buffers are 256-byte aligned).  The last
// one or two pieces are read as bytes, 128 (centred zero) behind the end.
// norm[row] (zeroed on the stream in front) += sum x'^2 of the pieces a wave wrote: per piece sum x^2 - 256 sum x + 16 * 16384 (a
// sum of 16 squares, so never negative; a pad byte adds 0), the two sums as 4 x u8 dot products; one non-returning 64-bit vector
// atomic per row and wave.  No LDS.
__global__ __launch_bounds__(DIRECT_BLOCK) void direct_centre_kernel(const uint8_t* __restrict__ src, int64_t stride, const long long* __restrict__ ofs,
                                                                     int n, int64_t L, int64_t kp, uint4* __restrict__ out,
                                                                     unsigned long long* __restrict__ norm) {
    const int lane = threadIdx.x & 63, h = lane >> 5;
    const int r = blockIdx.x * 32 + (lane & 31);
    const int64_t steps = kp / 32;
    uint4* o = out + (size_t)blockIdx.x * (size_t)steps * 64 + lane;
    const int64_t groups = steps / 4;                                  // (DIRECT_KGRAN / 32 = 4 steps per granule)
    const int64_t g0 = (int64_t)blockIdx.y * (DIRECT_BLOCK / 64) + (threadIdx.x >> 6), gstep = (int64_t)gridDim.y * (DIRECT_BLOCK / 64);
    const bool live = r < n;
    const uint8_t* p = live ? src + (ofs ? (int64_t)ofs[r] : (int64_t)r * stride) : src;
    const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 3);
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p - sh);
    unsigned long long sq = 0;
    for (int64_t g = g0; g < groups; g += gstep) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int64_t s = g * 4 + t, c = 2 * s + h, k = c * 16;
            uint32_t w[4] = {0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u};
            if (live) {
                if (k + 20 <= L) {
                    const uint32_t* d = q + c * 4;
                    const uint32_t d0 = d[0], d1 = d[1], d2 = d[2], d3 = d[3], d4 = d[4];
                    w[0] = __builtin_amdgcn_alignbyte(d1, d0, sh); w[1] = __builtin_amdgcn_alignbyte(d2, d1, sh);
                    w[2] = __builtin_amdgcn_alignbyte(d3, d2, sh); w[3] = __builtin_amdgcn_alignbyte(d4, d3, sh);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        uint32_t v = 0;
#pragma unroll
                        for (int b = 0; b < 4; ++b) {
                            const int64_t i = k + j * 4 + b;
                            v |= (uint32_t)(i < L ? p[i] : (uint8_t)128) << (8 * b);
                        }
                        w[j] = v;
                    }
                }
                uint32_t s2 = 0, s1 = 0;                               // (16 bytes: at most 16 * 65 025 and 16 * 255)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    s2 = __builtin_amdgcn_udot4(w[j], w[j], s2, false);
                    s1 = __builtin_amdgcn_udot4(w[j], 0x01010101u, s1, false);
                }
                sq += s2 + 262144u - 256u * s1;
            }
            o[(size_t)s * 64] = make_uint4(w[0] ^ 0x80808080u, w[1] ^ 0x80808080u, w[2] ^ 0x80808080u, w[3] ^ 0x80808080u);
        }
    }
    sq += __shfl_xor(sq, 32);
    if (live && h == 0) (void)__hip_atomic_fetch_add(norm + r, sq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// direct_centre_kernel's job under the gate's byte weights wgt[0 .. L) (0xFF valid, 0x00 masked; one array for all rows, 16-byte
// aligned, readable up to L + 4): the direct scope SLIDEO_DIRECT_VALID.  Same grid, same operand layout, same aligned-dword reads
// of the rows.  The stored operand is (x ^ 0x80) & w, so a masked byte is the centred zero and <a'_m, b'> against the UNMASKED page
// operand is the sum over the valid bytes of a' b'.  norm[row] += sum over the valid bytes of x'^2: per piece, with xm = x & w,
// sum xm^2 - 256 sum xm + 16384 * (valid bytes), the sums as 4 x u8 dot products (a masked byte adds 0 to each of the three).  The
// weights of a 16-byte piece at K (a multiple of 16) are ONE aligned 16-byte load; it is taken where the row's dwords are
// (K + 20 <= L, so it ends inside L + 4).  The last pieces read row and weights as bytes, weight 0 behind the end.
// STORE = false: the norms alone (the pages' masked norms; `out` is not touched).  No LDS.
template <bool STORE>
__global__ __launch_bounds__(DIRECT_BLOCK) void direct_centre_valid_kernel(const uint8_t* __restrict__ src, int64_t stride, const long long* __restrict__ ofs,
                                                                           int n, int64_t L, int64_t kp, const uint8_t* __restrict__ wgt,
                                                                           uint4* __restrict__ out, unsigned long long* __restrict__ norm) {
    const int lane = threadIdx.x & 63, h = lane >> 5;
    const int r = blockIdx.x * 32 + (lane & 31);
    const int64_t steps = kp / 32;
    uint4* o = STORE ? out + (size_t)blockIdx.x * (size_t)steps * 64 + lane : nullptr;
    const int64_t groups = steps / 4;
    const int64_t g0 = (int64_t)blockIdx.y * (DIRECT_BLOCK / 64) + (threadIdx.x >> 6), gstep = (int64_t)gridDim.y * (DIRECT_BLOCK / 64);
    const bool live = r < n;
    const uint8_t* p = live ? src + (ofs ? (int64_t)ofs[r] : (int64_t)r * stride) : src;
    const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 3);
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p - sh);
    const uint4* wq = reinterpret_cast<const uint4*>(wgt);
    unsigned long long sq = 0;
    for (int64_t g = g0; g < groups; g += gstep) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int64_t s = g * 4 + t, c = 2 * s + h, k = c * 16;
            uint32_t x[4] = {0u, 0u, 0u, 0u}, w[4] = {0u, 0u, 0u, 0u};
            if (live) {
                if (k + 20 <= L) {
                    const uint32_t* d = q + c * 4;
                    const uint32_t d0 = d[0], d1 = d[1], d2 = d[2], d3 = d[3], d4 = d[4];
                    const uint4 wv = wq[c];
                    x[0] = __builtin_amdgcn_alignbyte(d1, d0, sh); x[1] = __builtin_amdgcn_alignbyte(d2, d1, sh);
                    x[2] = __builtin_amdgcn_alignbyte(d3, d2, sh); x[3] = __builtin_amdgcn_alignbyte(d4, d3, sh);
                    w[0] = wv.x; w[1] = wv.y; w[2] = wv.z; w[3] = wv.w;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        uint32_t v = 0, u = 0;
#pragma unroll
                        for (int b = 0; b < 4; ++b) {
                            const int64_t i = k + j * 4 + b;
                            if (i < L) { v |= (uint32_t)p[i] << (8 * b); u |= (uint32_t)wgt[i] << (8 * b); }
                        }
                        x[j] = v; w[j] = u;
                    }
                }
                uint32_t s2 = 0, s1 = 0, nv = 0;                       // (16 bytes: at most 16 * 65 025, 16 * 255 and 16)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t xm = x[j] & w[j];
                    s2 = __builtin_amdgcn_udot4(xm, xm, s2, false);
                    s1 = __builtin_amdgcn_udot4(xm, 0x01010101u, s1, false);
                    nv = __builtin_amdgcn_udot4(w[j] & 0x01010101u, 0x01010101u, nv, false);
                }
                sq += s2 + 16384u * nv - 256u * s1;                    // (a sum of squares over the valid bytes: never negative)
            }
            if (STORE)
                o[(size_t)s * 64] = make_uint4((x[0] ^ 0x80808080u) & w[0], (x[1] ^ 0x80808080u) & w[1], (x[2] ^ 0x80808080u) & w[2],
                                               (x[3] ^ 0x80808080u) & w[3]);
        }
    }
    sq += __shfl_xor(sq, 32);
    if (live && h == 0) (void)__hip_atomic_fetch_add(norm + r, sq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// dot[f * np + c] += sum over this block's K chunk of a'[f][k] * b'[c][k], f < n frames, c < np pages of the class.
// grid (ceil(n / 128), ceil(np / 128), K chunks), block 256: wave w holds the 64 x 64 tile of frame tile 2 x + (w & 1) and page
// tile 2 y + (w >> 1) — 2 x 2 MFMA tiles, 64 accumulator registers — so every operand KiB a wave loads is loaded by one other
// wave of its block too (L1).  Per 32-byte K step: four contiguous 1 KiB loads, four v_mfma_i32_32x32x32_i8.  kchunk: a multiple
// of DIRECT_KGRAN, at most DIRECT_KCHUNK_MAX, so an accumulator stays inside +-2^30 and is drained once, at the end, with one
// non-returning 64-bit vector atomic per element (`dot` is zeroed on the stream in front; two's complement: the order of the
// adds does not matter).  An atomic instruction covers two 256-byte row segments of dot.  No LDS, no barrier: waves whose tile
// lies outside n x np leave at once.
__global__ __launch_bounds__(DIRECT_BLOCK, 2) void page_ssd_kernel(const uint4* __restrict__ a, int n, const uint4* __restrict__ b, int np, int64_t kp,
                                                                int64_t kchunk, unsigned long long* __restrict__ dot) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int ft = blockIdx.x * 2 + (w & 1), pt = blockIdx.y * 2 + (w >> 1);
    if (ft * DIRECT_TILE >= n || pt * DIRECT_TILE >= np) return;
    const int64_t steps = kp / 32;
    const int64_t s0 = (int64_t)blockIdx.z * (kchunk / 32);
    const int64_t s1 = s0 + kchunk / 32 < steps ? s0 + kchunk / 32 : steps;
    const uint4* a0 = a + ((size_t)(2 * ft) * (size_t)steps + (size_t)s0) * 64 + lane;
    const uint4* a1 = a0 + (size_t)steps * 64;
    const uint4* b0 = b + ((size_t)(2 * pt) * (size_t)steps + (size_t)s0) * 64 + lane;
    const uint4* b1 = b0 + (size_t)steps * 64;
    direct_v16i c00 = {0}, c01 = {0}, c10 = {0}, c11 = {0};
    const int nsteps = (int)(s1 - s0);                                 // (at most DIRECT_KCHUNK_MAX / 32)
    if (nsteps < 4) return;
    // Four K steps per iteration (kp, kchunk and so s0 and nsteps are multiples of DIRECT_KGRAN / 32 = 4) in two pairs whose
    // operand registers take turns: pair y is loaded in front of pair x's eight MFMAs, the next iteration's pair x in front of
    // pair y's, so a wave always has eight 16-byte loads in flight while it multiplies and no register is copied.  Behind the
    // chunk's last pair the loads repeat the iteration's own first pair (in bounds, unused).
    struct Pair { uint4 a0, a1, b0, b1, a2, a3, b2, b3; };
    auto ld = [&](int s) {
        const size_t o = (size_t)s * 64;
        return Pair{a0[o], a1[o], b0[o], b1[o], a0[o + 64], a1[o + 64], b0[o + 64], b1[o + 64]};
    };
    auto v4 = [](const uint4& u) { const direct_v4i v = {(int)u.x, (int)u.y, (int)u.z, (int)u.w}; return v; };
    auto mul = [&](const Pair& p) {
        c00 = __builtin_amdgcn_mfma_i32_32x32x32_i8(v4(p.a0), v4(p.b0), c00, 0, 0, 0);
        c01 = __builtin_amdgcn_mfma_i32_32x32x32_i8(v4(p.a0), v4(p.b1), c01, 0, 0, 0);
        c10 = __builtin_amdgcn_mfma_i32_32x32x32_i8(v4(p.a1), v4(p.b0), c10, 0, 0, 0);
        c11 = __builtin_amdgcn_mfma_i32_32x32x32_i8(v4(p.a1), v4(p.b1), c11, 0, 0, 0);
        c00 = __builtin_amdgcn_mfma_i32_32x32x32_i8(v4(p.a2), v4(p.b2), c00, 0, 0, 0);
        c01 = __builtin_amdgcn_mfma_i32_32x32x32_i8(v4(p.a2), v4(p.b3), c01, 0, 0, 0);
        c10 = __builtin_amdgcn_mfma_i32_32x32x32_i8(v4(p.a3), v4(p.b2), c10, 0, 0, 0);
        c11 = __builtin_amdgcn_mfma_i32_32x32x32_i8(v4(p.a3), v4(p.b3), c11, 0, 0, 0);
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
    // C / D: column (B's row: the page) = lane & 31, row (A's: the frame) = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    const int col = lane & 31, rbase = 4 * (lane >> 5);
    auto drain = [&](const direct_v16i& c, int fx, int py) {
        const int page = pt * DIRECT_TILE + py * 32 + col;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int frame = ft * DIRECT_TILE + fx * 32 + (reg & 3) + 8 * (reg >> 2) + rbase;
            if (frame < n && page < np)
                (void)__hip_atomic_fetch_add(dot + (size_t)frame * np + page, (unsigned long long)(long long)c[reg], __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT);
        }
    };
    drain(c00, 0, 0); drain(c01, 0, 1); drain(c10, 1, 0); drain(c11, 1, 1);
}

// Frame blockIdx.x (grid n, block 256): ssd(c) = anorm + bnorm[c] - 2 dot[c] for the class positions c = elig[0 .. ne) (ascending,
// so ascending deck pages = pages[c]); best[frame] = the smallest and the lowest page with it (UINT64_MAX, -1 when ne == 0).
// ssd_out (the tap; null in the gated path): ssd_out[frame * ssd_pitch + pages[c]] = ssd(c).
__global__ __launch_bounds__(DIRECT_BLOCK) void direct_best_kernel(const unsigned long long* __restrict__ dot, int np, const long long* __restrict__ anorm,
                                                                   const long long* __restrict__ bnorm, const int32_t* __restrict__ pages,
                                                                   const int32_t* __restrict__ elig, int ne, DirectBest* __restrict__ best,
                                                                   unsigned long long* __restrict__ ssd_out, int ssd_pitch) {
    __shared__ unsigned long long rs[DIRECT_BLOCK / 64];
    __shared__ int32_t rc[DIRECT_BLOCK / 64];
    const int f = blockIdx.x;
    const long long an = anorm[f];
    unsigned long long bs = ~0ull;
    int32_t bc = 0x7FFFFFFF;
    for (int e = threadIdx.x; e < ne; e += DIRECT_BLOCK) {             // (a thread's own e ascend: < keeps its first minimum)
        const int32_t c = elig[e];
        const unsigned long long s = (unsigned long long)(an + bnorm[c] - 2ll * (long long)dot[(size_t)f * np + c]);
        if (ssd_out) ssd_out[(size_t)f * ssd_pitch + pages[c]] = s;
        if (s < bs) { bs = s; bc = c; }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long os = __shfl_xor(bs, d);
        const int32_t oc = __shfl_xor(bc, d);
        if (os < bs || (os == bs && oc < bc)) { bs = os; bc = oc; }
    }
    if ((threadIdx.x & 63) == 0) { rs[threadIdx.x >> 6] = bs; rc[threadIdx.x >> 6] = bc; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < DIRECT_BLOCK / 64; ++k)
            if (rs[k] < bs || (rs[k] == bs && rc[k] < bc)) { bs = rs[k]; bc = rc[k]; }
        DirectBest r;
        r.ssd = bs; r.page = ne > 0 ? pages[bc] : -1; r._pad = 0;
        best[f] = r;
    }
}

// One block, behind gate_kernel on the unit's stream.  Frame j of the kept list idx[0 .. *count) is DIRECT iff
// best[j].ssd <= thr (slideo_direct_ssd_threshold, in 64-bit integers; thr < 0: never).  The direct frames leave the list in
// place — the rest keeps its ascending order: a wave-ballot prefix scan per chunk of DIRECT_BLOCK entries, the waves' totals
// through LDS, the carry from chunk to chunk; every entry of a chunk is read before any is written, and an entry is written at or
// below where it was read — and *count and the pinned record's list h_idx follow.  rec (pinned, direct_rec_*): the reduced
// count, then best SSD, page and direct flag of all n frames.  Ordinary vector stores throughout.
__global__ __launch_bounds__(DIRECT_BLOCK) void direct_gate_kernel(const DirectBest* __restrict__ best, int n, long long thr,
                                                                   int32_t* __restrict__ idx, uint32_t* __restrict__ count, int32_t* __restrict__ h_idx,
                                                                   uint8_t* __restrict__ rec) {
    __shared__ uint32_t wtot[DIRECT_BLOCK / 64];
    __shared__ uint32_t carry;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned long long* h_ssd = reinterpret_cast<unsigned long long*>(rec + direct_rec_ssd_ofs());
    int32_t* h_page = reinterpret_cast<int32_t*>(rec + direct_rec_page_ofs(n));
    uint8_t* h_flag = rec + direct_rec_flag_ofs(n);
    const uint32_t k = *count;
    if (threadIdx.x == 0) carry = 0;
    for (int i = threadIdx.x; i < n; i += DIRECT_BLOCK) {
        const DirectBest b = best[i];
        h_ssd[i] = b.ssd; h_page[i] = b.page; h_flag[i] = 0;
    }
    __syncthreads();                                                   // (count is read by all, the flags are cleared)
    for (uint32_t base = 0; base < k; base += DIRECT_BLOCK) {
        const uint32_t i = base + threadIdx.x;
        int32_t j = -1;
        bool keep = false, direct = false;
        if (i < k) {
            j = idx[i];
            direct = thr >= 0 && best[j].ssd <= (unsigned long long)thr;
            keep = !direct;
        }
        const unsigned long long b = __ballot(keep);
        if (lane == 0) wtot[w] = (uint32_t)__popcll(b);
        __syncthreads();
        uint32_t ofs = carry, all = 0;
        for (int q = 0; q < DIRECT_BLOCK / 64; ++q) { if (q < w) ofs += wtot[q]; all += wtot[q]; }
        if (direct) h_flag[j] = 1;
        if (keep) {
            const uint32_t r = ofs + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
            idx[r] = j; h_idx[r] = j;
        }
        __syncthreads();                                               // (every thread has read carry and wtot)
        if (threadIdx.x == 0) carry += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        *count = carry;
        DirectHostRec r{carry, (uint32_t)n};
        *reinterpret_cast<DirectHostRec*>(rec) = r;
    }
}

}  // namespace slideo
