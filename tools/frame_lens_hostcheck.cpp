// frame_lens_hostcheck — the per-pixel arithmetic of csrc/frame_lens.hip.h (lens_thread, compiled for the host) run lane by lane
// over a whole launch grid, for tests/test_frame_lens_abi.py, which compares the image with tests/frame_lens_ref.py.
//   g++ -O1 -g -std=c++17 -ffp-contract=off [-fsanitize=address,undefined] -I slideo_amd/csrc tools/frame_lens_hostcheck.cpp -o hostcheck
//   hostcheck <case> <out>
// <case>: int32 {sw, sh, stride, dw, dh, n, src_offset, region}, double M[9], double {cx, cy, f, k1, k2}, then n frames of
// sh * stride bytes.  <out>: n images of dh x dw x 3.  Source and destination lie in heap buffers of their exact size: the source's
// base is `src_offset` bytes past a dword boundary and its end is rounded up to one — the device allocation's granularity, which
// the aligned dword loads of the taps rely on, and not a byte more —, so the sanitized build sees every read and write past them.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "frame_lens.hip.h"

using namespace slideo;

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: %s <case> <out>\n", argv[0]); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hd[8];
    double M[9], L[5];
    if (std::fread(hd, 4, 8, f) != 8 || std::fread(M, 8, 9, f) != 9 || std::fread(L, 8, 5, f) != 5) return 2;
    const int sw = hd[0], sh = hd[1], stride = hd[2], dw = hd[3], dh = hd[4], n = hd[5], ofs = hd[6] & 3, region = hd[7];
    const size_t fb = (size_t)sh * stride, total = fb * n;
    uint8_t* raw = static_cast<uint8_t*>(std::aligned_alloc(4, (ofs + total + 3) / 4 * 4));
    uint8_t* src = raw + ofs;
    if (std::fread(src, 1, total, f) != total) return 2;
    std::fclose(f);
    const size_t ob = (size_t)dw * dh * 3 * n;
    uint8_t* out = static_cast<uint8_t*>(std::aligned_alloc(4, (ob + 3) / 4 * 4));
    const LensArgs a = lens_args(region ? M : nullptr, L[0], L[1], 1.0 / (L[2] * L[2]), L[3], L[4], src, (int64_t)fb, stride, sw, sh, out, dw, dh);
    const int gx = ((dw + 3) / 4 + RECT_TX - 1) / RECT_TX, gy = (dh + RECT_TY - 1) / RECT_TY;
    for (int z = 0; z < n; ++z)
        for (int by = 0; by < gy; ++by)
            for (int bx = 0; bx < gx; ++bx)
                for (int ty = 0; ty < RECT_TY; ++ty)
                    for (int tx = 0; tx < RECT_TX; ++tx) {
                        const int tix = bx * RECT_TX + tx, dy = by * RECT_TY + ty;
                        if (region) lens_thread<true>(a, tix, dy, z);
                        else lens_thread<false>(a, tix, dy, z);
                    }
    std::free(raw);
    f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(out, 1, ob, f) != ob) return 2;
    std::fclose(f);
    std::free(out);
    std::printf("region %d out4 %d grid %d x %d x %d\n", region, a.out4, gx, gy, n);
    return 0;
}
