// yuv_desc_hostcheck — the per-thread arithmetic of csrc/yuv420.hip.h (yuv_desc_thread, compiled for the host) run lane by lane over
// the whole launch grid, and the host rules of csrc/frame_settings.h that go with it, for tests/test_yuv_desc_abi.py, which compares
// the outcome with tests/yuv_desc_ref.py.
//   g++ -O1 -g -std=c++17 [-fsanitize=address,undefined] -I include -I slideo_amd/csrc tools/yuv_desc_hostcheck.cpp -o hostcheck
//   hostcheck convert <case> <out>
//       <case>: int32 {w, h, n, matrix, range, depth, y_stride, uv_stride, uv_step, src_offset}, int64 {u_offset, v_offset,
//       frame_stride}, then the frames: (n - 1) * frame_stride + span bytes.  <out>: n images of h x w x 3.  The source is copied
//       to `src_offset` bytes past the 16-byte aligned base of an allocation that ends with the last frame byte, and the destination
//       is exact-size too: a load or store past either end is the sanitizer's to report.  Prints the wide-load flags the host chose.
//   hostcheck validate w h y_stride uv_stride u_offset v_offset uv_step frame_stride bytes_per_sample
//       prints "<code> <message>" of yuv420_validate (code 0: "0 <span>")
//   hostcheck propose matrix range depth
//       prints "<code> <message>" of propose_yuv_description, and on success "0 c0 .. c6" of yuv_coefficients
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "frame_settings.h"
#include "yuv420.hip.h"

using namespace slideo;

namespace {

template <int DEPTH>
void run_grid(const YuvArgs& a, const YuvCoef& k, int n) {
    const int gx = ((a.w + 3) / 4 + YUV_TX - 1) / YUV_TX, gy = (a.h / 2 + YUV_TY - 1) / YUV_TY;
    for (int z = 0; z < n; ++z)
        for (int by = 0; by < gy; ++by)
            for (int bx = 0; bx < gx; ++bx)
                for (int ty = 0; ty < YUV_TY; ++ty)
                    for (int tx = 0; tx < YUV_TX; ++tx) yuv_desc_thread<DEPTH>(a, k, bx * YUV_TX + tx, by * YUV_TY + ty, z);
}

int convert(const char* in, const char* outp) {
    FILE* f = std::fopen(in, "rb");
    if (!f) return 2;
    int32_t hd[10];
    int64_t of[3];
    if (std::fread(hd, 4, 10, f) != 10 || std::fread(of, 8, 3, f) != 3) return 2;
    const int w = hd[0], h = hd[1], n = hd[2], matrix = hd[3], range = hd[4], depth = hd[5], ofs = hd[9] & 15;
    slideo_yuv420_layout L{};
    L.y_stride = hd[6]; L.uv_stride = hd[7]; L.uv_step = hd[8]; L.u_offset = of[0]; L.v_offset = of[1];
    const int64_t fs = of[2];
    int64_t span = 0;
    try {
        (void)propose_yuv_description(FrameSettings{}, matrix, range, depth);
        span = yuv420_validate(w, h, &L, n > 1 ? fs : -1, depth == SLIDEO_YUV_DEPTH_8 ? 1 : 2);
    } catch (const Error& e) { std::fprintf(stderr, "%d %s\n", e.code, e.what()); return 3; }
    const size_t total = (size_t)(fs * (n - 1) + span);
    // malloc's blocks are 16-byte aligned: the source starts `ofs` bytes in and ends with the block
    uint8_t* exact = static_cast<uint8_t*>(std::malloc(ofs + total));
    if (!exact || (uintptr_t)exact % 16 != 0) return 2;
    uint8_t* src = exact + ofs;
    if (std::fread(src, 1, total, f) != total) return 2;
    std::fclose(f);
    uint8_t* dst = static_cast<uint8_t*>(std::malloc((size_t)w * h * 3 * n));
    int32_t c[7];
    yuv_coefficients(matrix, range, c);
    const YuvCoef k{c[0], c[1], c[2], c[3], c[4], c[5]};
    const YuvArgs a = yuv_desc_args(depth, src, fs, L, w, h, n, dst);
    if (depth == SLIDEO_YUV_DEPTH_8) run_grid<YUV_D8>(a, k, n);
    else if (depth == SLIDEO_YUV_DEPTH_10_MSB) run_grid<YUV_D10_MSB>(a, k, n);
    else run_grid<YUV_D10_LSB>(a, k, n);
    f = std::fopen(outp, "wb");
    const size_t ob = (size_t)w * h * 3 * n;
    if (!f || std::fwrite(dst, 1, ob, f) != ob) return 2;
    std::fclose(f);
    std::free(dst);
    std::free(exact);
    std::printf("wide_y %d wide_c %d out4 %d\n", a.wide_y, a.wide_c, a.out4);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc >= 4 && !std::strcmp(argv[1], "convert")) return convert(argv[2], argv[3]);
    if (argc >= 11 && !std::strcmp(argv[1], "validate")) {
        slideo_yuv420_layout L{};
        const int w = std::atoi(argv[2]), h = std::atoi(argv[3]);
        L.y_stride = std::atoi(argv[4]); L.uv_stride = std::atoi(argv[5]); L.u_offset = std::atoll(argv[6]); L.v_offset = std::atoll(argv[7]);
        L.uv_step = std::atoi(argv[8]);
        try {
            std::printf("0 %lld\n", (long long)yuv420_validate(w, h, &L, std::atoll(argv[9]), std::atoi(argv[10])));
        } catch (const Error& e) { std::printf("%d %s\n", e.code, e.what()); }
        return 0;
    }
    if (argc >= 5 && !std::strcmp(argv[1], "propose")) {
        try {
            const FrameSettings s = propose_yuv_description(FrameSettings{}, std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]));
            int32_t c[7];
            yuv_coefficients(s.yuv.matrix, s.yuv.range, c);
            std::printf("0 %d %d %d %d %d %d %d\n", c[0], c[1], c[2], c[3], c[4], c[5], c[6]);
        } catch (const Error& e) { std::printf("%d %s\n", e.code, e.what()); }
        return 0;
    }
    std::fprintf(stderr, "usage: %s convert <case> <out> | validate ... | propose matrix range depth\n", argv[0]);
    return 2;
}
