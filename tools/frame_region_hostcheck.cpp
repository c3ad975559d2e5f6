// frame_region_hostcheck — the per-pixel arithmetic of csrc/frame_region.hip.h (rectify_thread, compiled for the host) run lane by
// lane over a whole launch grid, for tests/test_frame_region_abi.py, which compares the image with tests/frame_region_ref.py.
//   g++ -O1 -g -std=c++17 -ffp-contract=off [-fsanitize=address,undefined] -I slideo_amd/csrc tools/frame_region_hostcheck.cpp -o hostcheck
//   hostcheck <case> <out> [kind]
// <case>: int32 {sw, sh, stride, dw, dh, n, src_offset}, double M[9], then n frames of sh * stride bytes.  <out>: n images of
// dh x dw x 3.  kind: force an instance (0 projective, 1 affine) in place of the host's choice.  The source is copied to an
// allocation whose base is `src_offset` bytes past a dword boundary and whose end is rounded up to one — the device allocation's
// granularity, which the aligned dword loads of the taps rely on.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "frame_region.hip.h"

using namespace slideo;

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: %s <case> <out> [kind]\n", argv[0]); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hd[7];
    double M[9];
    if (std::fread(hd, 4, 7, f) != 7 || std::fread(M, 8, 9, f) != 9) return 2;
    const int sw = hd[0], sh = hd[1], stride = hd[2], dw = hd[3], dh = hd[4], n = hd[5], ofs = hd[6] & 3;
    const size_t fb = (size_t)sh * stride, total = fb * n;
    uint8_t* raw = static_cast<uint8_t*>(std::aligned_alloc(4, (ofs + total + 3) / 4 * 4 + 4));
    uint8_t* src = raw + ofs;
    if (std::fread(src, 1, total, f) != total) return 2;
    std::fclose(f);
    std::vector<uint8_t> out((size_t)dw * dh * 3 * n);
    int tx = 0, ty = 0;
    int kind = rect_classify(M, tx, ty);
    if (argc > 3) kind = std::atoi(argv[3]);
    const RectifyArgs a = rect_args(M, kind, tx, ty, src, (int64_t)fb, stride, sw, sh, out.data(), dw, dh);
    const int gx = ((dw + 3) / 4 + RECT_TX - 1) / RECT_TX, gy = (dh + RECT_TY - 1) / RECT_TY;
    for (int z = 0; z < n; ++z)
        for (int by = 0; by < gy; ++by)
            for (int bx = 0; bx < gx; ++bx)
                for (int ty_ = 0; ty_ < RECT_TY; ++ty_)
                    for (int tx_ = 0; tx_ < RECT_TX; ++tx_) {
                        const int tix = bx * RECT_TX + tx_, dy = by * RECT_TY + ty_;
                        if (kind == RECT_TRANSLATE) rectify_thread<RECT_TRANSLATE>(a, tix, dy, z);
                        else if (kind == RECT_AFFINE) rectify_thread<RECT_AFFINE>(a, tix, dy, z);
                        else rectify_thread<RECT_PROJECTIVE>(a, tix, dy, z);
                    }
    std::free(raw);
    f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(out.data(), 1, out.size(), f) != out.size()) return 2;
    std::fclose(f);
    std::printf("kind %d tx %d ty %d bw0 %d out4 %d in4 %d\n", kind, tx, ty, a.bw0, a.out4, a.in4);
    return 0;
}
