// activity_hostcheck — the per-thread bodies of csrc/activity.hip.h (activity_thread, activity_rows_px, activity_cols_px, compiled
// for the host) run lane by lane over their launch grids, for tests/test_activity_abi.py, which compares counts, carried image and
// mask with tests/activity_ref.py.
//   g++ -O1 -g -std=c++17 [-fsanitize=address,undefined] -I slideo_amd/csrc tools/activity_hostcheck.cpp -o hostcheck
//   hostcheck <case> <out>
// <case>: int32 {aw, ah, stride, n, src_offset, delta, have_prev, max_share_ppm, grow}, then (have_prev) the carried image, aw * ah * 3
// bytes, then n frames of ah * stride bytes.  <out>: the counts (u32 aw * ah), the carried image afterwards and, when there is a pair,
// the mask (aw * ah bytes) and int64 {n_active, n_masked}.
// Every buffer is a heap allocation of its exact size — the frames end with the last pixel of the last row, `src_offset` bytes past a
// 16-byte boundary — so that a sanitized build sees any access outside them.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "activity.hip.h"

using namespace slideo;

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: %s <case> <out>\n", argv[0]); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hd[9];
    if (std::fread(hd, 4, 9, f) != 9) return 2;
    const int aw = hd[0], ah = hd[1], stride = hd[2], n = hd[3], ofs = hd[4] & 3, delta = hd[5], have_prev = hd[6], ppm = hd[7], grow = hd[8];
    if (aw < 1 || ah < 1 || stride < aw * 3 || n < 1) return 2;
    const size_t px = (size_t)aw * ah, fb = (size_t)ah * stride;
    const size_t total = fb * (n - 1) + (size_t)(ah - 1) * stride + (size_t)aw * 3;
    uint8_t* last = static_cast<uint8_t*>(std::malloc(px * 3));
    uint32_t* count = static_cast<uint32_t*>(std::calloc(px, 4));
    uint8_t* raw = static_cast<uint8_t*>(std::malloc(ofs + total));
    if (!last || !count || !raw) return 2;
    std::memset(last, 0xEE, px * 3);
    if (have_prev && std::fread(last, 1, px * 3, f) != px * 3) return 2;
    std::vector<uint8_t> file(fb * n);
    if (std::fread(file.data(), 1, file.size(), f) != file.size()) return 2;
    std::fclose(f);
    uint8_t* src = raw + ofs;
    std::memcpy(src, file.data(), total);

    const ActivityArgs a = activity_args(src, (int64_t)fb, stride, aw, ah, n, delta, have_prev != 0, last, count);
    const int gx = ((aw + 3) / 4 + ACT_TX - 1) / ACT_TX, gy = (ah + ACT_TY - 1) / ACT_TY;
    for (int by = 0; by < gy; ++by)
        for (int bx = 0; bx < gx; ++bx)
            for (int ty = 0; ty < ACT_TY; ++ty)
                for (int tx = 0; tx < ACT_TX; ++tx) activity_thread(a, bx * ACT_TX + tx, by * ACT_TY + ty);

    f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(count, 4, px, f) != px || std::fwrite(last, 1, px * 3, f) != px * 3) return 2;
    const int64_t pairs = (int64_t)n - 1 + (have_prev ? 1 : 0);
    int64_t tot[2] = {0, 0};
    if (pairs > 0) {
        uint8_t* rows = static_cast<uint8_t*>(std::malloc(px));
        uint8_t* mask = static_cast<uint8_t*>(std::malloc(px));
        if (!rows || !mask) return 2;
        ActivityMaskArgs k{};
        k.count = count; k.aw = aw; k.ah = ah; k.grow = grow; k.ppm = (uint64_t)ppm; k.pairs = (uint64_t)pairs; k.rows = rows; k.mask = mask;
        const int mx = (aw + ACT_TX - 1) / ACT_TX;
        for (int pass = 0; pass < 2; ++pass)
            for (int by = 0; by < gy; ++by)
                for (int bx = 0; bx < mx; ++bx)
                    for (int ty = 0; ty < ACT_TY; ++ty)
                        for (int tx = 0; tx < ACT_TX; ++tx) {
                            const int x = bx * ACT_TX + tx, y = by * ACT_TY + ty;
                            if (x >= aw || y >= ah) continue;
                            tot[pass] += (pass == 0 ? activity_rows_px(k, x, y) : activity_cols_px(k, x, y)) ? 1 : 0;
                        }
        if (std::fwrite(mask, 1, px, f) != px || std::fwrite(tot, 8, 2, f) != 2) return 2;
        std::free(rows); std::free(mask);
    }
    std::fclose(f);
    std::free(raw); std::free(last); std::free(count);
    std::printf("in4 %d own4 %d pairs %lld active %lld masked %lld\n", a.in4, a.own4, (long long)pairs, (long long)tot[0], (long long)tot[1]);
    return 0;
}
