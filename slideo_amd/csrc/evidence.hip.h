// evidence.hip.h — the match evidence map (include/slideo_amd.h "Match evidence map"): where the keypoints of matched frames fall,
// and which of them the winning page's final transform explains.
//
//   evidence_kernel   grid: the unit's frames, block EV_THREADS; launched by unit_verify behind verdict_kernel on the unit's stream,
//                     only while a session is open.  Per frame: the verdict decides whether the frame contributes; the winner's slot
//                     in FrameCands::page[] gives its transform and its run of votes; every vote of the run is tested in f64 and
//                     sets its keypoint's bit in an LDS bitset (ds_or, no return value); then every keypoint adds 1 to seen[cell]
//                     and, with its bit set, to hit[cell] (integer global atomics whose result is not read).  Integer adds commute:
//                     the units in flight share one accumulator and the counts do not depend on their order.
//                     A frame with more than EV_BITS (2048) keypoints is walked in windows of EV_BITS keypoints, the votes once per window.
//                     The unit's flags word is read first: a unit whose run raised a re-run bit (the RNG stream, the keypoint
//                     capacity) leaves without counting; the run whose verdicts are returned raises none.
// The per-frame body is two host + device functions, one per phase, which a thread of the block (or, on the host, every thread
// index in turn: tools/evidence_hostcheck.cpp) calls with its index; the kernel puts its barriers between them.
// evidence_mask / evidence_box: the two pure host functions of the header, plain C++.
#pragma once
#include <stdint.h>

#include <vector>

#include "slideo_amd.h"
#include "types.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define EV_HD __host__ __device__ __forceinline__
#else
#define EV_HD inline
#endif

namespace slideo {

constexpr int EV_THREADS = 256;
constexpr int EV_BITS = 2048;                        // keypoints per window of the LDS bitset (256 B): an ORB-1000 frame is one window
constexpr int EV_WORDS = EV_BITS / 32;
constexpr uint32_t EV_MAX_FRAMES = 1u << 20;         // frames_counted of a session

struct EvVote { uint32_t x, y; };      // = uint2: a vote as vote_kernel writes it
struct EvXY { float x, y; };           // = float2: a train row's page coordinates

struct EvidenceArgs {
    const slideo_verdict* verdicts;      // the unit's, as verdict_kernel left them
    const FrameCands* fcs;
    const uint32_t* qofs;                // [n + 1] the frames' keypoint offsets
    const slideo_keypoint* kp;
    const EvXY* page_xy;           // per train row
    const EvVote* votes;              // (keypoint in frame, train row), a frame's at qofs[f] * k
    const uint32_t* flags;               // the unit's flags word (null: none to look at)
    uint32_t rerun_mask;                 // its bits that send the unit through the pipeline again
    int32_t k, model, min_inliers;
    double thr2;                         // ransac_threshold^2
    int32_t aw, ah, cell, gw, gh;
    uint32_t* seen;                      // [gh][gw]
    uint32_t* hit;
};

// what a frame contributes with: its keypoints, the winner's transform and its run of votes.  n == 0: nothing.
struct EvidenceFrame {
    uint32_t q0, n;
    const double* M;
    const EvVote* votes;
    int32_t count;
};

EV_HD EvidenceFrame evidence_frame(const EvidenceArgs& a, int f) {
    EvidenceFrame e{};
    if (a.flags && (a.flags[0] & a.rerun_mask)) return e;
    const slideo_verdict v = a.verdicts[f];
    if (v.page_idx < 0 || v.inliers < a.min_inliers) return e;
    const FrameCands& fc = a.fcs[f];
    int slot = -1;
    const int nc = fc.ncand < MAXC ? fc.ncand : MAXC;
    for (int j = 0; j < nc; ++j) if (fc.page[j] == v.page_idx) { slot = j; break; }
    if (slot < 0) return e;
    e.q0 = a.qofs[f]; e.n = a.qofs[f + 1] - e.q0;
    e.M = fc.M[slot];
    e.votes = a.votes + (size_t)e.q0 * a.k + fc.ofs[slot];
    e.count = fc.count[slot];
    return e;
}

// the hit test of the definition, in f64
EV_HD bool evidence_passes(const EvidenceArgs& a, const double* M, float x_, float y_, float X_, float Y_) {
    const double x = x_, y = y_, X = X_, Y = Y_;
    double px = M[0] * x + M[1] * y + M[2], py = M[3] * x + M[4] * y + M[5];
    if (a.model == 1) {
        const double w = M[6] * x + M[7] * y + M[8];
        if (w == 0.0) return false;
        px /= w; py /= w;
    }
    const double dx = px - X, dy = py - Y;
    return dx * dx + dy * dy <= a.thr2;
}

// phase 1 of a window [base, base + EV_BITS) of the frame's keypoints: thread tid of nt tests its share of the winner's votes
// bits: EV_WORDS words, zero before the phase
template <class Or>
EV_HD void evidence_votes(const EvidenceArgs& a, const EvidenceFrame& e, uint32_t base, int tid, int nt, uint32_t* bits, Or&& set_bits) {
    for (int i = tid; i < e.count; i += nt) {
        const EvVote v = e.votes[i];
        if (v.x < base || v.x >= e.n || v.x - base >= (uint32_t)EV_BITS) continue;
        const slideo_keypoint q = a.kp[e.q0 + v.x];
        const EvXY p = a.page_xy[v.y];
        if (evidence_passes(a, e.M, p.x, p.y, q.x, q.y)) set_bits(&bits[(v.x - base) >> 5], 1u << ((v.x - base) & 31));
    }
}

// phase 2 of the window: thread tid of nt counts its share of the window's keypoints
template <class Add>
EV_HD void evidence_count(const EvidenceArgs& a, const EvidenceFrame& e, uint32_t base, int tid, int nt, const uint32_t* bits, Add&& add) {
    const uint32_t end = e.n - base < (uint32_t)EV_BITS ? e.n : base + (uint32_t)EV_BITS;
    for (uint32_t q = base + (uint32_t)tid; q < end; q += (uint32_t)nt) {
        const slideo_keypoint kq = a.kp[e.q0 + q];
        // (a keypoint outside the analysed image — the caller's own features may hold any float — has no cell)
        if (!(kq.x >= 0.f && kq.x < (float)a.aw && kq.y >= 0.f && kq.y < (float)a.ah)) continue;
        const int cx = (int)kq.x / a.cell, cy = (int)kq.y / a.cell;
        if (cx >= a.gw || cy >= a.gh) continue;
        const size_t c = (size_t)cy * a.gw + cx;
        add(&a.seen[c]);
        if (bits[(q - base) >> 5] >> ((q - base) & 31) & 1u) add(&a.hit[c]);
    }
}

#if defined(__HIPCC__)
__global__ __launch_bounds__(EV_THREADS) void evidence_kernel(EvidenceArgs a) {
    __shared__ uint32_t bits[EV_WORDS];
    const int f = blockIdx.x, tid = threadIdx.x;
    const EvidenceFrame e = evidence_frame(a, f);          // (block-uniform: every thread reads the same words)
    if (e.n == 0) return;
    for (uint32_t base = 0; base < e.n; base += EV_BITS) {
        for (int i = tid; i < EV_WORDS; i += EV_THREADS) bits[i] = 0;
        __syncthreads();
        evidence_votes(a, e, base, tid, EV_THREADS, bits, [](uint32_t* p, uint32_t v) { atomicOr(p, v); });
        __syncthreads();
        evidence_count(a, e, base, tid, EV_THREADS, bits, [](uint32_t* p) { atomicAdd(p, 1u); });
        __syncthreads();
    }
}
#endif

// ---- the two pure host functions ---------------------------------------------------------------------------------------------------
inline bool evidence_cell_ok(int cell) { return cell == 16 || cell == 32 || cell == 64; }

// mask_out: ah rows of aw bytes, `stride` apart.  The Chebyshev dilation is a row pass, then a column pass (a square is separable)
inline void evidence_mask(const uint32_t* seen, const uint32_t* hit, int gw, int gh, int cell, int aw, int ah, uint32_t min_seen, uint32_t min_hit_ppm,
                          int grow, uint8_t* mask_out, int64_t stride) {
    const size_t nc = (size_t)gw * gh;
    std::vector<uint8_t> keep(nc), rows(nc), grown(nc);
    for (size_t c = 0; c < nc; ++c)
        keep[c] = !(seen[c] >= min_seen && (uint64_t)hit[c] * 1000000u < (uint64_t)min_hit_ppm * seen[c]);
    for (int y = 0; y < gh; ++y)
        for (int x = 0; x < gw; ++x) {
            uint8_t k = 0;
            const int x0 = x - grow < 0 ? 0 : x - grow, x1 = x + grow >= gw ? gw - 1 : x + grow;
            for (int u = x0; u <= x1 && !k; ++u) k = keep[(size_t)y * gw + u];
            rows[(size_t)y * gw + x] = k;
        }
    for (int y = 0; y < gh; ++y)
        for (int x = 0; x < gw; ++x) {
            uint8_t k = 0;
            const int y0 = y - grow < 0 ? 0 : y - grow, y1 = y + grow >= gh ? gh - 1 : y + grow;
            for (int v = y0; v <= y1 && !k; ++v) k = rows[(size_t)v * gw + x];
            grown[(size_t)y * gw + x] = k;
        }
    for (int y = 0; y < ah; ++y) {
        uint8_t* row = mask_out + (int64_t)y * stride;
        const uint8_t* g = grown.data() + (size_t)(y / cell) * gw;
        for (int x = 0; x < aw; ++x) row[x] = g[x / cell] ? 255 : 0;
    }
}

inline void evidence_box(const uint32_t* seen, const uint32_t* hit, int gw, int gh, int cell, int aw, int ah, uint32_t min_hits, uint32_t min_hit_ppm,
                         int32_t* box4) {
    int x0 = gw, y0 = gh, x1 = -1, y1 = -1;
    for (int y = 0; y < gh; ++y)
        for (int x = 0; x < gw; ++x) {
            const size_t c = (size_t)y * gw + x;
            if (hit[c] >= min_hits && (uint64_t)hit[c] * 1000000u >= (uint64_t)min_hit_ppm * seen[c]) {
                x0 = x < x0 ? x : x0; y0 = y < y0 ? y : y0; x1 = x > x1 ? x : x1; y1 = y > y1 ? y : y1;
            }
        }
    if (x1 < 0) { box4[0] = box4[1] = box4[2] = box4[3] = -1; return; }
    const int64_t bx1 = (int64_t)(x1 + 1) * cell, by1 = (int64_t)(y1 + 1) * cell;
    box4[0] = x0 * cell; box4[1] = y0 * cell;
    box4[2] = (int32_t)(bx1 < aw ? bx1 : aw); box4[3] = (int32_t)(by1 < ah ? by1 : ah);
}

}  // namespace slideo
