// gate_anchor.hip.h — kernels of the gate reference SLIDEO_GATE_ANCHOR, with and without a gate settle (stage_gate_anchor.hip;
// include/slideo_amd.h "Gate reference", "Gate settle").  Plain ANCHOR is the settle rule with a cap of zero and no previous-frame
// state: a frame that is away from the anchor is matched at once.
// The table <a'_i, a'_j> of a unit's frames, i < j, is the SSD-table engine's frame_gram_kernel (ssd_table.hip.h); under a settle
// its sub-diagonal gives every frame's SSD against the frame before it.
//
//   gate_carried_ssd_kernel   the unit's n frames against the carried anchor and, under a settle, frame 0 against the carried
//                             previous frame: n (+ 1) pairs in one launch, every pair cut across several blocks
//   gate_settle_kernel        one wave walks the table: away / still / deferral count -> what gate_kernel writes
//   gate_settle_state_kernel  the unit's last anchor and, under a settle, its last frame and the deferral count -> the gate state
//   gate_recall_kernel        ("Gate memory") one wave walks the table with the last M matched frames in its lanes: recalled /
//                             matched / deferred, and which earlier frame every frame stands behind
//   gate_memory_state_kernel  the slots the unit's matches took, the previous frame and the ring's head, count, anchor and d -> the state
//
// sum (a - b)^2 = |a'|^2 + |b'|^2 - 2 <a', b'> with x' = x - 128, exact in integers; under the gate's weights the operand is zero at
// the masked bytes and the norms run over the valid ones, so the same expression is the SSD over the valid bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

namespace slideo {

constexpr int CARRIED_SSD_BLOCK = 256;
constexpr int ANCHOR_STATE_BLOCK = 256;
constexpr int64_t CARRIED_SSD_DRAIN = 4096;     // dwords per thread between two drains of the u32 partial sums

// Pair y of gridDim.y, blockIdx.y: y < n: (anchor, small + y * L); y == n: (prev, small) — launched with n + 1 rows under a settle,
// with n rows and prev null without one.  out[y] += the sum over the pair's L bytes of
// (a - b)^2 — MASKED: over the bytes whose weight is 0xFF (gate_valid_kernel's weights: 4-byte aligned, zero-padded to whole
// dwords).  out is zeroed on the same stream in front of the launch; the blocks of a pair (gridDim.x of them, any number >= 1) each
// take a contiguous run of the body's dwords and add their total with ONE 64-bit vector atomic whose result is not used; integer
// sums make the order irrelevant.  Block 0 of a pair also takes the ragged tail.
// Every image starts at ANY byte alignment and is read as ALIGNED dwords, as ssd_masked_kernel reads its images: dword g of the
// image at p is bytes s .. s + 3 of q[g], q[g + 1], q = p - s, s = p & 3 (v_alignbyte_b32).  q[0] begins at most 3 bytes in front of
// the image (inside its allocation) and the body stops one dword early, so q[g + 1] never passes the image's end; the 4 .. 7 ragged
// bytes are read as bytes.  Per dword sum (a_k - b_k)^2 = a.a + b.b - 2 a.b as three 4 x u8 dot products, exact; the u32 partials
// take 520 200 per dword at most and are drained into u64 every CARRIED_SSD_DRAIN dwords of a thread.  LDS: the four waves' totals.
template <bool MASKED>
__global__ __launch_bounds__(CARRIED_SSD_BLOCK) void gate_carried_ssd_kernel(const uint8_t* __restrict__ anchor, const uint8_t* __restrict__ prev,
                                                                             const uint8_t* __restrict__ small, int64_t L, int n,
                                                                             const uint8_t* __restrict__ weights,
                                                                             unsigned long long* __restrict__ out) {
    __shared__ unsigned long long red[CARRIED_SSD_BLOCK / 64];
    const int y = blockIdx.y;
    const uint8_t* pa = y < n ? anchor : prev;
    const uint8_t* pb = small + (y < n ? (int64_t)y * L : 0);
    const uint32_t sa = (uint32_t)(reinterpret_cast<uintptr_t>(pa) & 3), sb = (uint32_t)(reinterpret_cast<uintptr_t>(pb) & 3);
    const uint32_t* qa = reinterpret_cast<const uint32_t*>(pa - sa);
    const uint32_t* qb = reinterpret_cast<const uint32_t*>(pb - sb);
    const uint32_t* qw = reinterpret_cast<const uint32_t*>(weights);
    const int64_t body = L / 4 > 0 ? L / 4 - 1 : 0;                    // dwords
    const int64_t per = (body + gridDim.x - 1) / gridDim.x;            // this block's run of them
    const int64_t lo = (int64_t)blockIdx.x * per;
    const int64_t hi = lo + per < body ? lo + per : body;
    unsigned long long s = 0;
    for (int64_t g0 = lo; g0 < hi; g0 += CARRIED_SSD_DRAIN * CARRIED_SSD_BLOCK) {
        const int64_t g1 = g0 + CARRIED_SSD_DRAIN * CARRIED_SSD_BLOCK < hi ? g0 + CARRIED_SSD_DRAIN * CARRIED_SSD_BLOCK : hi;
        uint32_t sq = 0, cr = 0;
        for (int64_t g = g0 + threadIdx.x; g < g1; g += CARRIED_SSD_BLOCK) {
            uint32_t am = __builtin_amdgcn_alignbyte(qa[g + 1], qa[g], sa);
            uint32_t bm = __builtin_amdgcn_alignbyte(qb[g + 1], qb[g], sb);
            if (MASKED) { const uint32_t w = qw[g]; am &= w; bm &= w; }
            sq = __builtin_amdgcn_udot4(am, am, sq, false);
            sq = __builtin_amdgcn_udot4(bm, bm, sq, false);
            cr = __builtin_amdgcn_udot4(am, bm, cr, false);
        }
        s += (unsigned long long)sq - 2ull * cr;                       // (a.a + b.b >= 2 a.b term by term)
    }
    if (blockIdx.x == 0)
        for (int64_t i = body * 4 + threadIdx.x; i < L; i += CARRIED_SSD_BLOCK)
            if (!MASKED || weights[i]) { const int d = (int)pa[i] - (int)pb[i]; s += (unsigned)(d * d); }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
#pragma unroll
        for (int k = 0; k < CARRIED_SSD_BLOCK / 64; ++k) t += red[k];
        atomicAdd(out + y, t);                                         // (result unused: a non-returning global atomic)
    }
}

// The deferral count in front of the frame at window position pos (0 .. 64): the run of away frames that ends in front of it — the
// ones of `away` below pos, counted down from pos - 1 —, extended by the carried count d when the run reaches the window's start,
// capped at max_defer.  (d <= max_defer <= INT32_MAX and pos <= 64: inside u32.)
__device__ inline uint32_t settle_run(unsigned long long away, int pos, uint32_t d, uint32_t max_defer) {
    const unsigned long long below = pos >= 64 ? ~0ull : (1ull << pos) - 1ull;
    const unsigned long long stop = ~away & below;                     // the frames below pos that are not away
    const uint32_t run = stop ? (uint32_t)(pos - 1 - (63 - __builtin_clzll(stop))) : (uint32_t)pos + d;
    return run < max_defer ? run : max_defer;
}

// One wave.  The anchor rule over a unit of n frames, with or without a settle (include/slideo_amd.h "Gate reference", "Gate
// settle").  For frame j:
//   ssd_a  against the anchor: carried[j] while no frame of the unit was matched (the carried anchor: the gate state), then the
//          matched frame a: norm[a] + norm[j] - 2 dot[a * n + j] (a < j);                         away  = ssd_a >= thr_c
//   ssd_p  against the frame before: carried[n] for frame 0 (the carried previous frame), else the table's sub-diagonal
//          norm[j - 1] + norm[j] - 2 dot[(j - 1) * n + j];                                        still = ssd_p <  thr_s
//   matched = away && (still || d >= max_defer), d the deferral count in front of j (*d_in in front of frame 0); a matched frame is
//   the anchor from then on and d = 0; an away frame that is not matched is deferred: d = min(d + 1, max_defer); !away: d = 0.
// Comparisons in 64-bit integers (thr_c = slideo_changed_ssd_threshold; INT64_MAX: never).
// max_defer == 0 — plain ANCHOR, and a settle with a cap of 0 — makes d >= max_defer always true: matched = away and d = 0.  The
// walk then takes a wave-uniform shortcut, one scalar branch in front of the loop: neither *d_in (which may be null) nor ssd_p —
// carried[n] and the sub-diagonal — is read and the first ballot is the matched lanes, so a step has ONE dependent table read and
// one ballot.
// force0 (the state "none"): frame 0 is matched with SSD 0 and is the first anchor, nothing carried is read.
// With anchor a, count d and next frame i the 64 lanes test frames i .. i + 63; one ballot gives `away`, from which every lane has
// its d (settle_run), a second the matched lanes: the first, f, is the next anchor, the lanes below it are unchanged or deferred
// (flag 0 either way), the walk continues at f + 1 with d = 0.  Without one the 64 frames are written and d carried on.
// Written, with ordinary vector stores, what gate_kernel writes: flags[n], the ascending kept list idx, *count — device memory — and
// the pinned record h_head = {count, n}, h_ssd (per frame ssd_a: the SSD against ITS anchor), h_idx, h_flag; and *anchor_out = the
// unit's last matched frame, -1 when there is none, and *d_out.
__global__ __launch_bounds__(64) void gate_settle_kernel(const unsigned long long* __restrict__ dot, const long long* __restrict__ norm,
                                                         const unsigned long long* __restrict__ carried, int n, long long thr_c, long long thr_s,
                                                         uint32_t max_defer, const uint32_t* __restrict__ d_in, int force0,
                                                         uint8_t* __restrict__ flags, int32_t* __restrict__ idx, uint32_t* __restrict__ count,
                                                         uint32_t* __restrict__ h_head, unsigned long long* __restrict__ h_ssd,
                                                         int32_t* __restrict__ h_idx, uint8_t* __restrict__ h_flag, int32_t* __restrict__ anchor_out,
                                                         uint32_t* __restrict__ d_out) {
    const int lane = threadIdx.x;
    // `defer` is a constant at each of the two uses below: the loop is compiled once without and once with the deferral's reads
    auto walk = [&](const bool defer) __attribute__((always_inline)) {
        int a = -1, i = 0;
        uint32_t k = 0, d = 0;
        if (force0) {
            if (n > 0) {
                if (lane == 0) { flags[0] = 1; h_flag[0] = 1; h_ssd[0] = 0ull; idx[0] = 0; h_idx[0] = 0; }
                a = 0; i = 1; k = 1;
            }
        } else if (defer) {
            d = *d_in;
            if (d > max_defer) d = max_defer;
        }
        while (i < n) {
            const int j = i + lane;
            unsigned long long s = 0;
            bool away = false, still = false;
            if (j < n) {
                s = a < 0 ? carried[j] : (unsigned long long)(norm[a] + norm[j] - 2ll * (long long)dot[(size_t)a * n + j]);
                away = (long long)s >= thr_c;                          // (an SSD is at most 255^2 * 3 * sw * sh: far inside int64)
                if (defer) {
                    const unsigned long long p = j == 0 ? carried[n] : (unsigned long long)(norm[j - 1] + norm[j] - 2ll * (long long)dot[(size_t)(j - 1) * n + j]);
                    still = (long long)p < thr_s;
                }
            }
            const unsigned long long ab = __ballot(away);
            const unsigned long long b = defer ? __ballot(away && (still || settle_run(ab, lane, d, max_defer) >= max_defer)) : ab;
            const int f = b ? __builtin_ctzll(b) : 64;                 // (wave-uniform)
            if (j < n && lane <= f) {
                const bool mine = lane == f;
                flags[j] = mine ? 1 : 0; h_flag[j] = mine ? 1 : 0;
                h_ssd[j] = s;
                if (mine) { idx[k] = j; h_idx[k] = j; }
            }
            if (f < 64) { a = i + f; i = a + 1; ++k; d = 0; }
            else {
                const int left = n - i < 64 ? n - i : 64;              // the window's frames
                if (defer) d = settle_run(ab, left, d, max_defer);
                i += 64;
            }
        }
        if (lane == 0) {
            *count = k;
            h_head[0] = k; h_head[1] = (uint32_t)n;
            *anchor_out = a;
            *d_out = d;
        }
    };
    if (max_defer != 0) walk(true);                                    // (a kernel argument: a scalar branch)
    else walk(false);
}

// anchor_state[0 .. nbytes) = the small image small + *anchor * stride — nothing when *anchor < 0: no frame of the unit was matched,
// the carried anchor stays —, and, with prev_state not null (a settle), prev_state[0 .. nbytes) = the unit's last small image
// small + (n - 1) * stride, always, and *d_state = *d.  Both sources start at ANY byte alignment and are read as ALIGNED dwords, as
// ssd_masked_kernel reads its images (v_alignbyte_b32 over q[g], q[g + 1], q = p - (p & 3)): the body stops one dword early, so
// q[g + 1] never passes the image's end, and q[0] begins at most 3 bytes in front of the image (inside the unit's buffer of small
// images, whose base is 256-byte aligned).  The 4 .. 7 ragged bytes are copied as bytes.  The states: 4-byte aligned.  Any grid;
// block ANCHOR_STATE_BLOCK.
__global__ __launch_bounds__(ANCHOR_STATE_BLOCK) void gate_settle_state_kernel(const uint8_t* __restrict__ small, int64_t stride, int n,
                                                                               const int32_t* __restrict__ anchor, const uint32_t* __restrict__ d,
                                                                               int64_t nbytes, uint8_t* __restrict__ anchor_state,
                                                                               uint8_t* __restrict__ prev_state, uint32_t* __restrict__ d_state) {
    const int a = *anchor;
    const int64_t body = nbytes / 4 > 0 ? nbytes / 4 - 1 : 0;          // dwords
    const int64_t t = (int64_t)blockIdx.x * ANCHOR_STATE_BLOCK + threadIdx.x, nt = (int64_t)gridDim.x * ANCHOR_STATE_BLOCK;
    for (int which = 0; which < 2; ++which) {
        if (which == 0 ? a < 0 : !prev_state) continue;
        const uint8_t* p = small + (int64_t)(which == 0 ? a : n - 1) * stride;
        uint8_t* state = which == 0 ? anchor_state : prev_state;
        const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 3);
        const uint32_t* q = reinterpret_cast<const uint32_t*>(p - sh);
        uint32_t* o = reinterpret_cast<uint32_t*>(state);
        for (int64_t g = t; g < body; g += nt) o[g] = __builtin_amdgcn_alignbyte(q[g + 1], q[g], sh);
        for (int64_t b = body * 4 + t; b < nbytes; b += nt) state[b] = p[b];
    }
    if (prev_state && t == 0) *d_state = *d;
}

// ---- gate memory (include/slideo_amd.h "Gate memory") --------------------------------------------------------------------------------
constexpr int GATE_MEMORY_SLOTS = 64;                                  // SLIDEO_GATE_MEMORY_MAX: one lane per slot
constexpr long long GATE_REF_DEFERRED = -2;                            // SLIDEO_GATE_REF_DEFERRED
// The memory beside its M small images (the gate state, device): a ring of M slots.  Slots 0 .. count - 1 are occupied, ord[] their
// frames' ordinals; head: the slot the next match overwrites (count < M: head == count); anchor: the anchor's slot; d: the deferral
// count (0 without a settle).
struct GateMemoryMeta { long long ord[GATE_MEMORY_SLOTS]; int32_t count, head, anchor; uint32_t d; };
// What a unit's walk leaves for gate_memory_state_kernel: per slot the frame of the unit that occupies it behind the unit (-1: the
// slot keeps what it carried, or nothing), and the ring's count, head, anchor slot and d behind the unit
struct GateMemoryUnit { int32_t occ[GATE_MEMORY_SLOTS]; int32_t count, head, anchor; uint32_t d; };

// One wave, no LDS.  The rule of "Gate memory" over a unit of n frames whose frame 0 has ordinal t0, with a memory of M slots
// (1 <= M <= 64).  Lane l < M holds slot l's occupant: occ < 0 the entry the slot carried (`in`), else frame occ of this unit; ord:
// its ordinal (valid while l < count).  The anchor is a slot, wave-uniform.  SSDs of frame j:
//   against a carried slot c:  mnorm[c] + norm[j] - 2 mdot[j * M + c]
//   against frame a < j of the unit:  norm[a] + norm[j] - 2 dot[a * n + j]                  (the table holds a < j alone)
//   ssd_p against the frame before (max_defer != 0 alone): *prev_ssd0 for frame 0, else the table's sub-diagonal
// A step: the 64 lanes test frames i .. i + 63 against the anchor, one ballot gives `away`; the lanes below the first away frame j
// are unchanged (flag 0, ref = the anchor's ordinal) and d = 0 behind them.  For j every lane computes its occupant's SSD against j;
// a butterfly on (SSD, then the greater ordinal) — ordinals are distinct, so every lane ends with the same entry r — and then
//   ssd_r < thr_c:                      recalled: flag 0, anchor = r's slot, d = 0, ref = r's ordinal;
//   else still || d >= max_defer:       matched: flag 1, slot head := j (its lane takes occ = j, ord = t0 + j), anchor = head,
//                                       head = (head + 1) % M, count = min(count + 1, M), d = 0, ref = t0 + j;
//   else                                deferred: flag 0, d = min(d + 1, max_defer), ref = GATE_REF_DEFERRED;
// and the walk continues at j + 1: a unit with more than M matches overwrites slots inside the walk, and every later frame sees
// exactly the M most recent matches.  max_defer == 0 (no settle, or a cap of 0): d >= max_defer always, neither *prev_ssd0 nor the
// sub-diagonal is read.  force0 (the state "none"): frame 0 is matched with SSD 0 into slot 0, `in` is not read.
// Comparisons in 64-bit integers.  Written with ordinary vector stores: what gate_settle_kernel writes (flags, the kept list idx,
// *count; the pinned h_head = {count, n}, h_ssd — per frame ssd_a against the anchor in force BEFORE it is decided —, h_idx, h_flag),
// ref[n] and its pinned twin h_ref[n], and *out.
__global__ __launch_bounds__(64) void gate_recall_kernel(const unsigned long long* __restrict__ dot, const long long* __restrict__ norm,
                                                         const unsigned long long* __restrict__ mdot, const long long* __restrict__ mnorm,
                                                         const GateMemoryMeta* __restrict__ in, const unsigned long long* __restrict__ prev_ssd0,
                                                         int n, int M, long long t0, long long thr_c, long long thr_s, uint32_t max_defer, int force0,
                                                         uint8_t* __restrict__ flags, int32_t* __restrict__ idx, uint32_t* __restrict__ count,
                                                         uint32_t* __restrict__ h_head, unsigned long long* __restrict__ h_ssd,
                                                         int32_t* __restrict__ h_idx, uint8_t* __restrict__ h_flag, long long* __restrict__ ref,
                                                         long long* __restrict__ h_ref, GateMemoryUnit* __restrict__ out) {
    const int lane = threadIdx.x;
    const bool defer = max_defer != 0;                                 // (a kernel argument: wave-uniform)
    int occ = -1;
    long long ord = LLONG_MIN;
    int cnt = 0, head = 0, anc = 0, i = 0;
    uint32_t k = 0, d = 0;
    if (force0) {
        if (n > 0) {
            if (lane == 0) {
                occ = 0; ord = t0;
                flags[0] = 1; h_flag[0] = 1; h_ssd[0] = 0ull; idx[0] = 0; h_idx[0] = 0; ref[0] = t0; h_ref[0] = t0;
            }
            cnt = 1; head = M > 1 ? 1 : 0; i = 1; k = 1;
        }
    } else {
        cnt = in->count; head = in->head; anc = in->anchor;
        d = in->d < max_defer ? in->d : max_defer;
        if (lane < cnt) ord = in->ord[lane];
    }
    while (i < n) {
        const int ao = __shfl(occ, anc);                                // the anchor's occupant and ordinal
        const long long aord = __shfl(ord, anc);
        const int j = i + lane;
        long long s = 0;
        bool away = false, still = false;
        if (j < n) {
            s = ao < 0 ? mnorm[anc] + norm[j] - 2ll * (long long)mdot[(size_t)j * M + anc]
                       : norm[ao] + norm[j] - 2ll * (long long)dot[(size_t)ao * n + j];
            away = s >= thr_c;
            if (defer) {
                const long long p = j == 0 ? (long long)*prev_ssd0 : norm[j - 1] + norm[j] - 2ll * (long long)dot[(size_t)(j - 1) * n + j];
                still = p < thr_s;
            }
        }
        const unsigned long long ab = __ballot(away), sb = __ballot(still);
        const int f = ab ? __builtin_ctzll(ab) : 64;                   // (wave-uniform)
        if (j < n && lane < f) { flags[j] = 0; h_flag[j] = 0; h_ssd[j] = (unsigned long long)s; ref[j] = aord; h_ref[j] = aord; }
        if (f == 64) { d = 0; i += 64; continue; }                     // (the window holds at least one frame, and none is away)
        if (f > 0) d = 0;
        const int jf = i + f;                                          // the away frame: every slot's occupant against it
        const long long sf = __shfl(s, f);
        long long e = LLONG_MAX, eo = LLONG_MIN;
        int es = lane;
        if (lane < cnt) {
            e = occ < 0 ? mnorm[lane] + norm[jf] - 2ll * (long long)mdot[(size_t)jf * M + lane]
                        : norm[occ] + norm[jf] - 2ll * (long long)dot[(size_t)occ * n + jf];
            eo = ord;
        }
#pragma unroll
        for (int x = 32; x > 0; x >>= 1) {
            const long long oe = __shfl_xor(e, x), oo = __shfl_xor(eo, x);
            const int os = __shfl_xor(es, x);
            if (oe < e || (oe == e && oo > eo)) { e = oe; eo = oo; es = os; }
        }
        int fl = 0;
        long long r;
        if (e < thr_c) { anc = es; d = 0; r = eo; }
        else if (((sb >> f) & 1ull) || d >= max_defer) {
            fl = 1;
            if (lane == head) { occ = jf; ord = t0 + jf; }
            anc = head;
            head = head + 1 < M ? head + 1 : 0;
            cnt = cnt < M ? cnt + 1 : M;
            d = 0; r = t0 + jf;
        } else { d = d + 1 < max_defer ? d + 1 : max_defer; r = GATE_REF_DEFERRED; }
        if (lane == 0) {
            flags[jf] = (uint8_t)fl; h_flag[jf] = (uint8_t)fl; h_ssd[jf] = (unsigned long long)sf; ref[jf] = r; h_ref[jf] = r;
            if (fl) { idx[k] = jf; h_idx[k] = jf; }
        }
        k += (uint32_t)fl;
        i = jf + 1;
    }
    out->occ[lane] = lane < M ? occ : -1;
    if (lane == 0) {
        *count = k;
        h_head[0] = k; h_head[1] = (uint32_t)n;
        out->count = cnt; out->head = head; out->anchor = anc; out->d = d;
    }
}

// blockIdx.y = y.  y < M, slot y: when its occupant behind the unit is a frame of the unit (u->occ[y] >= 0) that frame's small image
// small + occ * stride -> mem + y * mem_stride and meta->ord[y] = t0 + occ; a slot that keeps what it carried is not touched.
// y == M (launched with M + 1 rows under a settle, prev_state not null): the unit's last small image -> prev_state.  Block (0, 0)
// also writes the ring's count, head, anchor slot and d.  nbytes per image; the sources start at ANY byte alignment and are read as
// ALIGNED dwords exactly as gate_settle_state_kernel reads them (the body stops one dword early, the 4 .. 7 ragged bytes are copied
// as bytes); mem, mem_stride and prev_state: 4-byte aligned.  Grid (any, M [+ 1]); block ANCHOR_STATE_BLOCK.
__global__ __launch_bounds__(ANCHOR_STATE_BLOCK) void gate_memory_state_kernel(const uint8_t* __restrict__ small, int64_t stride, int n, int M,
                                                                               long long t0, const GateMemoryUnit* __restrict__ u, int64_t nbytes,
                                                                               uint8_t* __restrict__ mem, int64_t mem_stride,
                                                                               uint8_t* __restrict__ prev_state, GateMemoryMeta* __restrict__ meta) {
    const int y = blockIdx.y;
    const int src = y < M ? u->occ[y] : n - 1;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (y < M && src >= 0) meta->ord[y] = t0 + src;
        if (y == 0) { meta->count = u->count; meta->head = u->head; meta->anchor = u->anchor; meta->d = u->d; }
    }
    if (src < 0 || src >= n || (y >= M && !prev_state)) return;
    const uint8_t* p = small + (int64_t)src * stride;
    uint8_t* state = y < M ? mem + (int64_t)y * mem_stride : prev_state;
    const int64_t body = nbytes / 4 > 0 ? nbytes / 4 - 1 : 0;          // dwords
    const int64_t t = (int64_t)blockIdx.x * ANCHOR_STATE_BLOCK + threadIdx.x, nt = (int64_t)gridDim.x * ANCHOR_STATE_BLOCK;
    const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 3);
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p - sh);
    uint32_t* o = reinterpret_cast<uint32_t*>(state);
    for (int64_t g = t; g < body; g += nt) o[g] = __builtin_amdgcn_alignbyte(q[g + 1], q[g], sh);
    for (int64_t b = body * 4 + t; b < nbytes; b += nt) state[b] = p[b];
}

}  // namespace slideo
