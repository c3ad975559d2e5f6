// placement_lens.h — the pure host function behind slideo_placement_lens (include/slideo_amd.h "Placement lens"): the joint fit of
// a homography and the frame lens's radial terms to the placement session's cell means, float64, damped Gauss-Newton with an
// analytic Jacobian.  Plain C++ (no device): the points and the linear start are placement.hip.h's, the monotonicity rule
// frame_settings.h's.  The restatement is tests/frame_lens_ref.py placement_lens.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "frame_settings.h"
#include "placement.hip.h"

namespace slideo {

constexpr double PLENS_LAMBDA0 = 1e-3, PLENS_LAMBDA_MIN = 1e-12, PLENS_LAMBDA_MAX = 1e8, PLENS_REL_STOP = 1e-12, PLENS_PIVOT = 1e-12;

struct PlacementLensModel {
    double h[8];            // H = [[h0 h1 h2] [h3 h4 h5] [h6 h7 1]]: (u, v) -> ideal pixel / s
    double k[2];
    double s, cx, cy, q;
    int np;                 // 9 or 10 parameters
};

// D(s H(u, v)) and, J non-null, its derivatives by the parameters (J[0 .. np): x, J[np .. 2 np): y); false: w == 0 or not finite
inline bool plens_eval(const PlacementLensModel& m, double u, double v, double* X, double* Y, double* r2_out, double* J) {
    const double* h = m.h;
    const double w = h[6] * u + h[7] * v + 1.0;
    if (w == 0.0) return false;
    const double Px = m.s * ((h[0] * u + h[1] * v + h[2]) / w), Py = m.s * ((h[3] * u + h[4] * v + h[5]) / w);
    const double a = Px - m.cx, b = Py - m.cy;
    const double r2 = (a * a + b * b) * m.q;
    const double g = 1.0 + r2 * (m.k[0] + r2 * m.k[1]);
    *X = m.cx + a * g; *Y = m.cy + b * g;
    if (r2_out) *r2_out = r2;
    if (!std::isfinite(*X) || !std::isfinite(*Y)) return false;
    if (!J) return true;
    const double gp = m.k[0] + 2.0 * m.k[1] * r2;              // dg / dr2
    const double xx = g + 2.0 * m.q * gp * a * a, xy = 2.0 * m.q * gp * a * b, yy = g + 2.0 * m.q * gp * b * b;      // dD / dP
    const double su = m.s * u / w, sv = m.s * v / w, s1 = m.s / w;
    const double dPx[8] = {su, sv, s1, 0, 0, 0, -Px * u / w, -Px * v / w}, dPy[8] = {0, 0, 0, su, sv, s1, -Py * u / w, -Py * v / w};
    double* Jx = J;
    double* Jy = J + m.np;
    for (int i = 0; i < 8; ++i) { Jx[i] = xx * dPx[i] + xy * dPy[i]; Jy[i] = xy * dPx[i] + yy * dPy[i]; }
    Jx[8] = a * r2; Jy[8] = b * r2;
    if (m.np == 10) { Jx[9] = a * r2 * r2; Jy[9] = b * r2 * r2; }
    return true;
}

inline bool plens_cost(const PlacementLensModel& m, const std::vector<PlacementPoint>& pts, double* cost) {
    double c = 0;
    for (const PlacementPoint& p : pts) {
        double X, Y;
        if (!plens_eval(m, p.u, p.v, &X, &Y, nullptr, nullptr)) return false;
        c += (X - p.X) * (X - p.X) + (Y - p.Y) * (Y - p.Y);
    }
    *cost = c;
    return std::isfinite(c);
}

// A x = b of n <= 10 unknowns, A symmetric positive definite, by Cholesky on the matrix scaled to a unit diagonal; false: a
// diagonal entry that is not positive, or a pivot at or below `pivot`
inline bool plens_solve(const double* A, const double* b, int n, double pivot, double* x) {
    double d[10], L[100], y[10];
    for (int i = 0; i < n; ++i) { if (!(A[i * n + i] > 0.0) || !std::isfinite(A[i * n + i])) return false; d[i] = 1.0 / std::sqrt(A[i * n + i]); }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j) {
            double v = A[i * n + j] * d[i] * d[j];
            for (int k = 0; k < j; ++k) v -= L[i * n + k] * L[j * n + k];
            if (i == j) { if (!(v > pivot)) return false; L[i * n + i] = std::sqrt(v); }
            else L[i * n + j] = v / L[j * n + j];
        }
    for (int i = 0; i < n; ++i) { double v = b[i] * d[i]; for (int k = 0; k < i; ++k) v -= L[i * n + k] * y[k]; y[i] = v / L[i * n + i]; }
    for (int i = n - 1; i >= 0; --i) { double v = y[i]; for (int k = i + 1; k < n; ++k) v -= L[k * n + i] * x[k]; x[i] = v / L[i * n + i]; }
    for (int i = 0; i < n; ++i) { x[i] *= d[i]; if (!std::isfinite(x[i])) return false; }
    return true;
}

// The normal equations of the points at m: A = J^T J, g = J^T r (r = D(P) - (X, Y)); false: a point without an image
inline bool plens_normal(const PlacementLensModel& m, const std::vector<PlacementPoint>& pts, double* A, double* g) {
    const int n = m.np;
    for (int i = 0; i < n * n; ++i) A[i] = 0;
    for (int i = 0; i < n; ++i) g[i] = 0;
    double J[20];
    for (const PlacementPoint& p : pts) {
        double X, Y;
        if (!plens_eval(m, p.u, p.v, &X, &Y, nullptr, J)) return false;
        const double r[2] = {X - p.X, Y - p.Y};
        for (int e = 0; e < 2; ++e) {
            const double* Je = J + e * n;
            for (int i = 0; i < n; ++i) {
                g[i] += Je[i] * r[e];
                for (int j = 0; j < n; ++j) A[i * n + j] += Je[i] * Je[j];
            }
        }
    }
    return true;
}

// At most `iters` damped steps from m (the header's damping and stopping rule); false: a rank-deficient or non-finite step
inline bool plens_iterate(PlacementLensModel& m, const std::vector<PlacementPoint>& pts, int iters) {
    const int n = m.np;
    double cost, lambda = PLENS_LAMBDA0;
    if (!plens_cost(m, pts, &cost)) return false;
    double A[100], g[10], B[100], ng[10], step[10];
    for (int it = 0; it < iters; ++it) {
        if (cost == 0.0) break;
        if (!plens_normal(m, pts, A, g)) return false;
        for (int i = 0; i < n * n; ++i) B[i] = A[i];
        for (int i = 0; i < n; ++i) { B[i * n + i] += lambda * A[i * n + i]; ng[i] = -g[i]; }
        if (!plens_solve(B, ng, n, 0.0, step)) return false;
        PlacementLensModel t = m;
        for (int i = 0; i < 8; ++i) t.h[i] += step[i];
        t.k[0] += step[8];
        if (n == 10) t.k[1] += step[9];
        double c2;
        if (plens_cost(t, pts, &c2) && c2 < cost) {
            const bool done = cost - c2 <= PLENS_REL_STOP * cost;
            m = t; cost = c2;
            lambda = lambda / 10.0 > PLENS_LAMBDA_MIN ? lambda / 10.0 : PLENS_LAMBDA_MIN;
            if (done) break;
        } else {
            lambda *= 10.0;
            if (lambda > PLENS_LAMBDA_MAX) break;
        }
    }
    // the undamped system at the result has full rank: the fit is determined by the points
    if (!plens_normal(m, pts, A, g)) return false;
    for (int i = 0; i < n; ++i) ng[i] = -g[i];
    return plens_solve(A, ng, n, PLENS_PIVOT, step);
}

// the header's slideo_placement_lens behind its argument checks; false: refused (nothing is written)
inline bool placement_lens(const uint64_t* n, const uint64_t* sfx, const uint64_t* sfy, const uint64_t* su, const uint64_t* sv, int gw, int gh, int aw, int ah,
                           uint64_t min_count, double cx, double cy, double f, int order, double trim_px, int rounds, int iters, double* k2_out,
                           double* quad8, double* H9, int32_t* cells_used, double* rms_px) {
    std::vector<PlacementPoint> pts;
    for (size_t c = 0; c < (size_t)gw * gh; ++c) {
        if (n[c] < min_count) continue;
        const double k = (double)n[c];
        pts.push_back(PlacementPoint{(double)su[c] / k / 1048576.0, (double)sv[c] / k / 1048576.0, (double)sfx[c] / k / 16.0, (double)sfy[c] / k / 16.0});
    }
    const size_t need = (size_t)(4 + order);
    PlacementLensModel m{};
    m.s = (double)(aw > ah ? aw : ah); m.cx = cx; m.cy = cy; m.q = 1.0 / (f * f); m.np = 8 + order;
    double H[9];
    if (pts.size() < need || !placement_fit(pts, m.s, H)) return false;           // the linear start over ALL points, untrimmed
    for (int i = 0; i < 8; ++i) m.h[i] = H[i];
    if (!plens_iterate(m, pts, iters)) return false;
    auto residual = [&](const PlacementPoint& p, double* r) {
        double X, Y;
        if (!plens_eval(m, p.u, p.v, &X, &Y, nullptr, nullptr)) return false;
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
        if (pts.size() < need || !plens_iterate(m, pts, iters)) return false;
    }
    double ss = 0, R2 = 0, q[8];
    for (const PlacementPoint& p : pts) {
        double X, Y, r2;
        if (!plens_eval(m, p.u, p.v, &X, &Y, &r2, nullptr)) return false;
        ss += (X - p.X) * (X - p.X) + (Y - p.Y) * (Y - p.Y);
        if (r2 > R2) R2 = r2;
    }
    if (!frame_lens_monotone(m.k[0], m.k[1], R2)) return false;
    const double Hs[9] = {m.h[0], m.h[1], m.h[2], m.h[3], m.h[4], m.h[5], m.h[6], m.h[7], 1.0};
    const double cu[4] = {0, 1, 1, 0}, cv[4] = {0, 0, 1, 1};
    for (int i = 0; i < 4; ++i)
        if (!placement_apply(Hs, m.s, cu[i], cv[i], &q[2 * i], &q[2 * i + 1])) return false;
    for (int i = 0; i < 8; ++i) quad8[i] = q[i];
    for (int i = 0; i < 9; ++i) H9[i] = i < 6 ? m.s * Hs[i] : Hs[i];
    k2_out[0] = m.k[0]; k2_out[1] = order == 2 ? m.k[1] : 0.0;
    *cells_used = (int32_t)pts.size();
    *rms_px = std::sqrt(ss / (double)pts.size());
    return true;
}

}  // namespace slideo
