// shading_field.h — slideo_shading_field (include/slideo_amd.h "Frame shading", "Match shading map"): the gain field of a shading
// session's per-cell sums.  A pure host function in integers, plain C++ (no HIP include); the session that makes the sums and the
// kernel that applies the field are csrc/shading.hip.h's.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "frame_settings.h"

namespace slideo {

// slideo_shading_field (include/slideo_amd.h "Match shading map"): the field of a session's sums, in integers; false (nothing
// written): a bad argument, sums no session gives, or no valid cell.  Values are Q12 until the last step
inline bool shading_field(const uint64_t* cnt, const uint64_t* sum_f, const uint64_t* sum_p, int gw, int gh, int cell, int64_t min_count,
                          int min_gain_q8, int max_gain_q8, int smooth, uint16_t* gains_out, int32_t* cells_used_out) {
    if (!cnt || !sum_f || !sum_p || !gains_out || !shading_cell_ok(cell) || gw < 1 || gh < 1 || gw > (MAX_DIM + cell - 1) / cell ||
        gh > (MAX_DIM + cell - 1) / cell)
        return false;
    if (min_count < 1 || min_gain_q8 < 1 || min_gain_q8 > 256 || max_gain_q8 < 256 || max_gain_q8 > 65535 || smooth < 0 || smooth > 16) return false;
    const size_t n = (size_t)gw * gh;
    const uint64_t lo = 16u * (uint64_t)min_gain_q8, hi = 16u * (uint64_t)max_gain_q8;
    std::vector<uint64_t> v(n, 0), w(n, 0);
    std::vector<uint8_t> ok(n, 0), ok2;
    int32_t used = 0;
    for (size_t k = 0; k < n; ++k) {
        if (cnt[k] > ((uint64_t)1 << 54) || sum_f[k] > 765u * cnt[k] || sum_p[k] > 765u * cnt[k]) return false;
        if (cnt[k] < (uint64_t)min_count || sum_f[k] < 1) continue;
        // (2 * 4096 * sum_p + sum_f) / (2 * sum_f): sum_p <= 765 * 2^54 keeps the numerator inside 128 bits' lower 78; exact
        const unsigned __int128 r = ((unsigned __int128)8192u * sum_p[k] + sum_f[k]) / ((unsigned __int128)2u * sum_f[k]);
        v[k] = r < lo ? lo : r > hi ? hi : (uint64_t)r;
        ok[k] = 1; ++used;
    }
    if (used == 0) return false;
    // fill: rounds over the invalid cells with a valid 4-neighbour, from the values of the round before
    for (size_t left = n - (size_t)used; left > 0;) {
        w = v; ok2 = ok;
        for (int y = 0; y < gh; ++y)
            for (int x = 0; x < gw; ++x) {
                const size_t k = (size_t)y * gw + x;
                if (ok[k]) continue;
                uint64_t S = 0, c = 0;
                if (x > 0 && ok[k - 1]) { S += v[k - 1]; ++c; }
                if (x + 1 < gw && ok[k + 1]) { S += v[k + 1]; ++c; }
                if (y > 0 && ok[k - gw]) { S += v[k - gw]; ++c; }
                if (y + 1 < gh && ok[k + gw]) { S += v[k + gw]; ++c; }
                if (!c) continue;
                w[k] = (2 * S + c) / (2 * c); ok2[k] = 1; --left;
            }
        v.swap(w); ok.swap(ok2);
    }
    for (int round = 0; round < smooth; ++round) {
        for (int y = 0; y < gh; ++y)
            for (int x = 0; x < gw; ++x) {
                uint64_t S = 0;
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx)
                        S += v[(size_t)std::min(std::max(y + dy, 0), gh - 1) * gw + std::min(std::max(x + dx, 0), gw - 1)];
                w[(size_t)y * gw + x] = (2 * S + 9) / 18;
            }
        v.swap(w);
    }
    for (int j = 0; j <= gh; ++j)
        for (int i = 0; i <= gw; ++i) {
            uint64_t S = 0, c = 0;
            for (int y = j - 1; y <= j; ++y)
                for (int x = i - 1; x <= i; ++x)
                    if (x >= 0 && x < gw && y >= 0 && y < gh) { S += v[(size_t)y * gw + x]; ++c; }
            const uint64_t node = (2 * S + c) / (2 * c), g = (node + 8) >> 4;
            gains_out[(size_t)j * (gw + 1) + i] = (uint16_t)(g < (uint64_t)min_gain_q8 ? (uint64_t)min_gain_q8 : g > (uint64_t)max_gain_q8 ? (uint64_t)max_gain_q8 : g);
        }
    if (cells_used_out) *cells_used_out = used;
    return true;
}

}  // namespace slideo
