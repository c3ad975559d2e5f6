// content_hostcheck — the per-thread bodies of csrc/content.hip.h (content_thread, content_px with content_strip, compiled for the
// host) run lane by lane over their launch grids, for tests/test_content_abi.py, which compares lit counts, fills and n_content with
// tests/content_ref.py.  The wave ballot's popcount and the atomics of content_fill_kernel are plain sums here.
//   g++ -O1 -g -std=c++17 [-fsanitize=address,undefined] -I slideo_amd/csrc tools/content_hostcheck.cpp -o hostcheck
//   hostcheck <case> <out>
// <case>: int32 {aw, ah, stride, n, src_offset, level, min_share_ppm, split[4]} — the n frames are observed in launches of split[0],
// split[1], ... frames (zeros end the list; what is left goes into a last launch) —, then n frames of ah * stride bytes.
// <out>: the lit counts (u32 aw * ah), the row fills (u32 ah), the column fills (u32 aw), int64 n_content.
// Every buffer is a heap allocation of its exact size — the frames end with the last pixel of the last row, `src_offset` bytes past a
// 16-byte boundary — so that a sanitized build sees any access outside them.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "content.hip.h"

using namespace slideo;

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: %s <case> <out>\n", argv[0]); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hd[11];
    if (std::fread(hd, 4, 11, f) != 11) return 2;
    const int aw = hd[0], ah = hd[1], stride = hd[2], n = hd[3], ofs = hd[4] & 3, level = hd[5], ppm = hd[6];
    if (aw < 1 || ah < 1 || stride < aw * 3 || n < 1) return 2;
    const size_t px = (size_t)aw * ah, fb = (size_t)ah * stride;
    const size_t total = fb * (n - 1) + (size_t)(ah - 1) * stride + (size_t)aw * 3;
    uint32_t* lit = static_cast<uint32_t*>(std::calloc(px, 4));
    uint8_t* raw = static_cast<uint8_t*>(std::malloc(ofs + total));
    if (!lit || !raw) return 2;
    std::vector<uint8_t> file(fb * n);
    if (std::fread(file.data(), 1, file.size(), f) != file.size()) return 2;
    std::fclose(f);
    uint8_t* src = raw + ofs;
    std::memcpy(src, file.data(), total);

    const int gx = ((aw + 3) / 4 + CNT_TX - 1) / CNT_TX, gy = (ah + CNT_TY - 1) / CNT_TY;
    int in4 = 1, own4 = 1, launches = 0;
    for (int i = 0, k = 0; i < n; ++k) {
        int nb = k < 4 && hd[7 + k] > 0 ? hd[7 + k] : n - i;
        if (nb > n - i) nb = n - i;
        const ContentArgs a = content_args(src + (size_t)i * fb, (int64_t)fb, stride, aw, ah, nb, level, lit);
        in4 &= a.in4; own4 &= a.own4; ++launches;
        for (int by = 0; by < gy; ++by)
            for (int bx = 0; bx < gx; ++bx)
                for (int ty = 0; ty < CNT_TY; ++ty)
                    for (int tx = 0; tx < CNT_TX; ++tx) content_thread(a, bx * CNT_TX + tx, by * CNT_TY + ty);
        i += nb;
    }

    uint32_t* rows = static_cast<uint32_t*>(std::calloc(ah, 4));
    uint32_t* cols = static_cast<uint32_t*>(std::calloc(aw, 4));
    if (!rows || !cols) return 2;
    ContentFillArgs k{};
    k.lit = lit; k.aw = aw; k.ah = ah; k.ppm = (uint64_t)ppm; k.frames = (uint64_t)n; k.row_fill = rows; k.col_fill = cols;
    int64_t n_content = 0;
    const int fx = (aw + CNT_FILL_TX - 1) / CNT_FILL_TX, fy = (ah + CNT_FILL_ROWS - 1) / CNT_FILL_ROWS;
    for (int by = 0; by < fy; ++by)
        for (int bx = 0; bx < fx; ++bx)
            for (int tx = 0; tx < CNT_FILL_TX; ++tx) {
                const int x = bx * CNT_FILL_TX + tx;              // (lanes beyond the last column run too, as on the device)
                int y0, y1;
                content_strip(k, by, y0, y1);
                uint32_t col = 0;
                for (int y = y0; y < y1; ++y)
                    if (content_px(k, x, y)) { ++rows[y]; ++col; ++n_content; }
                if (col) cols[x] += col;
            }

    f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(lit, 4, px, f) != px || std::fwrite(rows, 4, ah, f) != (size_t)ah || std::fwrite(cols, 4, aw, f) != (size_t)aw ||
        std::fwrite(&n_content, 8, 1, f) != 1)
        return 2;
    std::fclose(f);
    std::free(raw); std::free(lit); std::free(rows); std::free(cols);
    std::printf("in4 %d own4 %d launches %d content %lld\n", in4, own4, launches, (long long)n_content);
    return 0;
}
