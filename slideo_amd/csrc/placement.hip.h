// placement.hip.h — the match placement map (include/slideo_amd.h "Match placement map"): per cell of the analysed image, where the
// matched keypoints lie in the frame and where their page points lie on the unit slide, summed in integers; and the quad fitted to them.
//
//   placement_kernel   grid: the unit's frames, block PL_THREADS; launched by unit_verify behind verdict_kernel (and evidence_kernel and
//                      tone_kernel) on the unit's stream, only while a session is open.  Per frame:
//                        the contributor   the candidate slot with a model and the most inliers (placement_frame: the tone table's rule;
//                                          block-uniform), the unit's flags word read first;
//                      then, by windows of PL_WIN keypoints (an ORB-1000 frame is one window):
//                        phase 1           every vote of the contributor's run is tested in f64; a passing vote applies an LDS 64-bit
//                                          unsigned min (result unused) to its keypoint's slot with the bit pattern of d2, which orders
//                                          as d2 does for non-negative finite doubles;
//                        phase 2           the votes whose d2 equals their slot's minimum apply an LDS 32-bit unsigned min with the
//                                          train row: the smallest d2, ties to the smallest row, whatever the votes' order;
//                        phase 3           one thread per keypoint with a winner computes the five addends and issues five 64-bit
//                                          global atomic adds whose result is not read.
//                      LDS: PL_WIN * (8 + 4) bytes = 24 KB.  No compare-and-swap loop.  Integer adds commute: the units in flight share
//                      one accumulator and no order enters.  A unit that is run again leaves without counting (evidence_kernel's rule).
// The per-frame body is host + device functions which a thread of the block (or, on the host, every thread index in turn:
// tools/placement_hostcheck.cpp) calls with its index; the kernel puts its barriers between them.
// placement_quad: the pure host function of the header, float64, a Householder QR with column pivoting.
#pragma once
#include <stdint.h>

#include <cmath>
#include <vector>

#include "tone.hip.h"

namespace slideo {

constexpr int PL_THREADS = 256;
constexpr int PL_WIN = 2048;                              // keypoints per window: 16 KB of d2 slots and 8 KB of row slots
constexpr int64_t PL_MAX_FRAMES = (int64_t)1 << 20;       // frames through a session
constexpr unsigned long long PL_NONE64 = ~0ull;           // a d2 slot without a passing vote (above every finite double's pattern)
constexpr uint32_t PL_NONE32 = 0xFFFFFFFFu;

struct PlacementArgs {
    EvidenceArgs ev;                     // fcs, qofs, kp, page_xy, votes, flags, rerun_mask, k, model (the others unused)
    const PageInfo* pageinfo;
    double reach2;                       // reach * reach
    int32_t aw, ah, cell, gw, gh, min_inliers;
    unsigned long long* acc;             // {n | sfx | sfy | su | sv} of gw * gh each, then frames_counted
};

// the contributor of a frame: its page's full size, its transform and its run of votes.  slot < 0: none
struct PlacementFrame {
    int32_t slot, pw, ph, count;
    uint32_t q0, n;
    const double* M;
    const EvVote* votes;
};

EV_HD PlacementFrame placement_frame(const PlacementArgs& a, int f) {
    PlacementFrame e{};
    e.slot = -1;
    if (a.ev.flags && (a.ev.flags[0] & a.ev.rerun_mask)) return e;
    const FrameCands& fc = a.ev.fcs[f];
    const int nc = fc.ncand < MAXC ? fc.ncand : MAXC;
    int best = -1;
    for (int j = 0; j < nc; ++j) {
        if (fc.inliers[j] < a.min_inliers || !tone_slot_found(fc, j, a.ev.model)) continue;
        if (best < 0 || fc.inliers[j] > fc.inliers[best]) best = j;
    }
    if (best < 0) return e;
    const PageInfo pi = a.pageinfo[fc.page[best]];
    e.slot = best; e.pw = pi.w; e.ph = pi.h; e.count = fc.count[best];
    e.q0 = a.ev.qofs[f]; e.n = a.ev.qofs[f + 1] - e.q0;
    e.M = fc.M[best];
    e.votes = a.ev.votes + (size_t)e.q0 * a.ev.k + fc.ofs[best];
    return e;
}

// the residual of the definition in f64 (the evidence map's arithmetic) -> whether the vote passes, and d2's bit pattern
EV_HD bool placement_d2(const PlacementArgs& a, const double* M, float x_, float y_, float X_, float Y_, unsigned long long* bits) {
    const double x = x_, y = y_, X = X_, Y = Y_;
    double px = M[0] * x + M[1] * y + M[2], py = M[3] * x + M[4] * y + M[5];
    if (a.ev.model == 1) {
        const double w = M[6] * x + M[7] * y + M[8];
        if (w == 0.0) return false;
        px /= w; py /= w;
    }
    const double dx = px - X, dy = py - Y;
    const double d2 = dx * dx + dy * dy;
    if (!(d2 <= a.reach2) || !(d2 <= 1.7976931348623157e308)) return false;      // (a NaN fails the first test, an infinity the second)
    __builtin_memcpy(bits, &d2, 8);
    return true;
}

// a vote of the run inside the window [base, base + PL_WIN) -> its pattern; false: outside, or it does not pass
EV_HD bool placement_vote(const PlacementArgs& a, const PlacementFrame& e, uint32_t base, const EvVote v, unsigned long long* bits) {
    if (v.x < base || v.x >= e.n || v.x - base >= (uint32_t)PL_WIN) return false;
    const slideo_keypoint q = a.ev.kp[e.q0 + v.x];
    const EvXY p = a.ev.page_xy[v.y];
    return placement_d2(a, e.M, p.x, p.y, q.x, q.y, bits);
}

// phase 1 of a window: thread tid of nt tests its share of the run.  d2min: PL_WIN slots, PL_NONE64 before the phase
template <class Min64>
EV_HD void placement_nearest(const PlacementArgs& a, const PlacementFrame& e, uint32_t base, int tid, int nt, unsigned long long* d2min, Min64&& min64) {
    for (int i = tid; i < e.count; i += nt) {
        const EvVote v = e.votes[i];
        unsigned long long bits;
        if (placement_vote(a, e, base, v, &bits)) min64(&d2min[v.x - base], bits);
    }
}

// phase 2 of the window: the votes at their slot's minimum.  tmin: PL_WIN slots, PL_NONE32 before the phase
template <class Min32>
EV_HD void placement_rows(const PlacementArgs& a, const PlacementFrame& e, uint32_t base, int tid, int nt, const unsigned long long* d2min, uint32_t* tmin,
                          Min32&& min32) {
    for (int i = tid; i < e.count; i += nt) {
        const EvVote v = e.votes[i];
        unsigned long long bits;
        if (placement_vote(a, e, base, v, &bits) && bits == d2min[v.x - base]) min32(&tmin[v.x - base], v.y);
    }
}

// phase 3 of the window: thread tid of nt adds its share of the window's keypoints
template <class Add64>
EV_HD void placement_sums(const PlacementArgs& a, const PlacementFrame& e, uint32_t base, int tid, int nt, const unsigned long long* d2min, const uint32_t* tmin,
                          Add64&& add64) {
    if (e.pw < 2 || e.ph < 2) return;                    // (a page one pixel wide or high has no unit slide)
    const uint32_t end = e.n - base < (uint32_t)PL_WIN ? e.n : base + (uint32_t)PL_WIN;
    const size_t nc = (size_t)a.gw * a.gh;
    for (uint32_t q = base + (uint32_t)tid; q < end; q += (uint32_t)nt) {
        if (d2min[q - base] == PL_NONE64) continue;
        const uint32_t t = tmin[q - base];
        if (t == PL_NONE32) continue;
        const slideo_keypoint kq = a.ev.kp[e.q0 + q];
        if (!(kq.x >= 0.f && kq.x < (float)a.aw && kq.y >= 0.f && kq.y < (float)a.ah)) continue;
        const EvXY p = a.ev.page_xy[t];
        const double x = p.x, y = p.y;
        if (!(x >= 0.0 && x <= (double)(e.pw - 1) && y >= 0.0 && y <= (double)(e.ph - 1))) continue;
        const int cx = (int)kq.x / a.cell, cy = (int)kq.y / a.cell;
        if (cx >= a.gw || cy >= a.gh) continue;
        const size_t c = (size_t)cy * a.gw + cx;
        const double fx = __builtin_rint((double)kq.x * 16.0), fy = __builtin_rint((double)kq.y * 16.0);
        const double u = __builtin_rint(x / (double)(e.pw - 1) * 1048576.0), v = __builtin_rint(y / (double)(e.ph - 1) * 1048576.0);
        add64(a.acc + c, 1ull);
        add64(a.acc + nc + c, (unsigned long long)fx);
        add64(a.acc + 2 * nc + c, (unsigned long long)fy);
        add64(a.acc + 3 * nc + c, (unsigned long long)u);
        add64(a.acc + 4 * nc + c, (unsigned long long)v);
    }
}

#if defined(__HIPCC__)
__global__ __launch_bounds__(PL_THREADS) void placement_kernel(PlacementArgs a) {
    __shared__ unsigned long long d2min[PL_WIN];
    __shared__ uint32_t tmin[PL_WIN];
    const int f = blockIdx.x, tid = threadIdx.x;
    const PlacementFrame e = placement_frame(a, f);        // (block-uniform: every thread reads the same words)
    if (e.slot < 0) return;
    if (tid == 0) atomicAdd(a.acc + 5 * (size_t)a.gw * a.gh, 1ull);
    if (e.n == 0 || e.count <= 0) return;
    for (uint32_t base = 0; base < e.n; base += PL_WIN) {
        for (int i = tid; i < PL_WIN; i += PL_THREADS) { d2min[i] = PL_NONE64; tmin[i] = PL_NONE32; }
        __syncthreads();
        placement_nearest(a, e, base, tid, PL_THREADS, d2min, [](unsigned long long* p, unsigned long long v) { atomicMin(p, v); });
        __syncthreads();
        placement_rows(a, e, base, tid, PL_THREADS, d2min, tmin, [](uint32_t* p, uint32_t v) { atomicMin(p, v); });
        __syncthreads();
        placement_sums(a, e, base, tid, PL_THREADS, d2min, tmin, [](unsigned long long* p, unsigned long long v) { atomicAdd(p, v); });
        __syncthreads();
    }
}
#endif

// ---- the pure host function ----------------------------------------------------------------------------------------------------
struct PlacementPoint { double u, v, X, Y; };

// H (h8 == 1) of the points under the header's two equations per point, in the least-squares sense: Householder QR with column
// pivoting of the 2N x 8 system.  false: a diagonal entry of R below 1e-10 of the largest (rank deficient)
inline bool placement_fit(const std::vector<PlacementPoint>& pts, double s, double* H) {
    const size_t rows = 2 * pts.size();
    if (rows < 8) return false;
    std::vector<double> A(rows * 8), b(rows);
    for (size_t i = 0; i < pts.size(); ++i) {
        const PlacementPoint& p = pts[i];
        const double xh = p.X / s, yh = p.Y / s;
        double* r0 = &A[2 * i * 8];
        double* r1 = r0 + 8;
        r0[0] = p.u; r0[1] = p.v; r0[2] = 1; r0[3] = 0; r0[4] = 0; r0[5] = 0; r0[6] = -xh * p.u; r0[7] = -xh * p.v;
        r1[0] = 0; r1[1] = 0; r1[2] = 0; r1[3] = p.u; r1[4] = p.v; r1[5] = 1; r1[6] = -yh * p.u; r1[7] = -yh * p.v;
        b[2 * i] = xh; b[2 * i + 1] = yh;
    }
    int perm[8] = {0, 1, 2, 3, 4, 5, 6, 7};
    double first = 0;
    for (int k = 0; k < 8; ++k) {
        int piv = k;
        double best = -1;
        for (int j = k; j < 8; ++j) {
            double nj = 0;
            for (size_t r = (size_t)k; r < rows; ++r) nj += A[r * 8 + j] * A[r * 8 + j];
            if (nj > best) { best = nj; piv = j; }
        }
        if (piv != k) {
            for (size_t r = 0; r < rows; ++r) std::swap(A[r * 8 + k], A[r * 8 + piv]);
            std::swap(perm[k], perm[piv]);
        }
        const double norm = std::sqrt(best);
        if (k == 0) first = norm;
        if (!(norm > 1e-10 * first) || !(first > 0)) return false;
        const double akk = A[(size_t)k * 8 + k];
        const double alpha = akk > 0 ? -norm : norm;
        std::vector<double> w(rows - (size_t)k);
        w[0] = akk - alpha;
        for (size_t r = (size_t)k + 1; r < rows; ++r) w[r - (size_t)k] = A[r * 8 + k];
        double ww = 0;
        for (double x : w) ww += x * x;
        if (ww > 0) {
            for (int j = k; j < 8; ++j) {
                double d = 0;
                for (size_t r = (size_t)k; r < rows; ++r) d += w[r - (size_t)k] * A[r * 8 + j];
                d = 2 * d / ww;
                for (size_t r = (size_t)k; r < rows; ++r) A[r * 8 + j] -= d * w[r - (size_t)k];
            }
            double d = 0;
            for (size_t r = (size_t)k; r < rows; ++r) d += w[r - (size_t)k] * b[r];
            d = 2 * d / ww;
            for (size_t r = (size_t)k; r < rows; ++r) b[r] -= d * w[r - (size_t)k];
        }
    }
    double z[8];
    for (int k = 7; k >= 0; --k) {
        double v = b[(size_t)k];
        for (int j = k + 1; j < 8; ++j) v -= A[(size_t)k * 8 + j] * z[j];
        z[k] = v / A[(size_t)k * 8 + k];
    }
    for (int k = 0; k < 8; ++k) H[perm[k]] = z[k];
    H[8] = 1.0;
    for (int k = 0; k < 8; ++k) if (!std::isfinite(H[k])) return false;
    return true;
}

// s * H applied to (u, v); false: w == 0 or a non-finite result
inline bool placement_apply(const double* H, double s, double u, double v, double* X, double* Y) {
    const double w = H[6] * u + H[7] * v + 1.0;
    if (w == 0.0) return false;
    *X = s * ((H[0] * u + H[1] * v + H[2]) / w);
    *Y = s * ((H[3] * u + H[4] * v + H[5]) / w);
    return std::isfinite(*X) && std::isfinite(*Y);
}

// the header's slideo_placement_quad behind its argument checks; false: fewer than 4 points at a stage, a rank-deficient system
// or a non-finite result (nothing is written)
inline bool placement_quad(const uint64_t* n, const uint64_t* sfx, const uint64_t* sfy, const uint64_t* su, const uint64_t* sv, int gw, int gh, int aw, int ah,
                           uint64_t min_count, double trim_px, int rounds, double* quad8, double* H9, int32_t* cells_used, double* rms_px) {
    std::vector<PlacementPoint> pts;
    for (size_t c = 0; c < (size_t)gw * gh; ++c) {
        if (n[c] < min_count) continue;
        const double k = (double)n[c];
        pts.push_back(PlacementPoint{(double)su[c] / k / 1048576.0, (double)sv[c] / k / 1048576.0, (double)sfx[c] / k / 16.0, (double)sfy[c] / k / 16.0});
    }
    const double s = (double)(aw > ah ? aw : ah);
    double H[9];
    if (pts.size() < 4 || !placement_fit(pts, s, H)) return false;
    auto residual = [&](const PlacementPoint& p, double* r) {
        double X, Y;
        if (!placement_apply(H, s, p.u, p.v, &X, &Y)) return false;
        *r = std::sqrt((X - p.X) * (X - p.X) + (Y - p.Y) * (Y - p.Y));
        return true;
    };
    for (int round = 0; round < rounds; ++round) {
        std::vector<PlacementPoint> kept;
        for (const PlacementPoint& p : pts) {
            double r;
            if (residual(p, &r) && r <= trim_px) kept.push_back(p);
        }
        if (kept.size() == pts.size()) break;
        pts.swap(kept);
        if (pts.size() < 4 || !placement_fit(pts, s, H)) return false;
    }
    double ss = 0, q[8];
    for (const PlacementPoint& p : pts) {
        double r;
        if (!residual(p, &r)) return false;
        ss += r * r;
    }
    const double cu[4] = {0, 1, 1, 0}, cv[4] = {0, 0, 1, 1};
    for (int i = 0; i < 4; ++i)
        if (!placement_apply(H, s, cu[i], cv[i], &q[2 * i], &q[2 * i + 1])) return false;
    for (int i = 0; i < 8; ++i) quad8[i] = q[i];
    for (int i = 0; i < 9; ++i) H9[i] = H[i];
    *cells_used = (int32_t)pts.size();
    *rms_px = std::sqrt(ss / (double)pts.size());
    return true;
}

}  // namespace slideo
