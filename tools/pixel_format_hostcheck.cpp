// pixel_format_hostcheck — the per-thread body of csrc/pixel_format.hip.h (pixels_thread, compiled for the host) run lane by lane over
// the whole launch grid, and the host rules of csrc/frame_settings.h that go with "Frame pixel format", for
// tests/test_pixel_format_abi.py, which compares the outcome with tests/pixel_format_ref.py.
//   g++ -O1 -g -std=c++17 [-fsanitize=address,undefined] -I include -I slideo_amd/csrc tools/pixel_format_hostcheck.cpp -o hostcheck
//   hostcheck convert <case> <out>
//       <case>: int32 {w, h, n, format, stride, src_offset, 0, 0}, int64 {frame_stride}, then the frames: (n - 1) * frame_stride +
//       span bytes.  <out>: n images of h x w x 3.  The source is copied to `src_offset` bytes past the 16-byte aligned base of an
//       allocation that ends with the last frame byte, and the destination is exact-size too: a load or store past either end is
//       the sanitizer's to report, and so is a wide load at an address that is not a multiple of its size.  Prints the paths the
//       host chose: "wide <0|4|8|16> out4 <0|1>".
//   hostcheck validate format w h stride frame_stride
//       prints "<code> <message>" of pixel_format_validate (code 0: "0 <span>")
//   hostcheck set <format> ...
//       walks slideo_matcher_set_pixel_format calls in order over one FrameSettings as settings_commit does (proposal, then the
//       rules between settings; a refused call leaves the record as it was) and prints per call "<code> <message>", then
//       "state <format>"
//   hostcheck info <format>
//       prints "<ok> bytes_per_pixel planes b g r" of pixel_format_info and pixel_format_channels
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "frame_settings.h"
#include "pixel_format.hip.h"

using namespace slideo;

namespace {

template <int FORM>
void run_grid(const PixArgs& a, int n) {
    const int gx = ((a.w + 3) / 4 + YUV_TX - 1) / YUV_TX, gy = (a.h + YUV_TY - 1) / YUV_TY;
    for (int z = 0; z < n; ++z)
        for (int by = 0; by < gy; ++by)
            for (int bx = 0; bx < gx; ++bx)
                for (int ty = 0; ty < YUV_TY; ++ty)
                    for (int tx = 0; tx < YUV_TX; ++tx) pixels_thread<FORM>(a, bx * YUV_TX + tx, by * YUV_TY + ty, z);
}

int convert(const char* in, const char* outp) {
    FILE* f = std::fopen(in, "rb");
    if (!f) return 2;
    int32_t hd[8];
    int64_t fs = 0;
    if (std::fread(hd, 4, 8, f) != 8 || std::fread(&fs, 8, 1, f) != 1) return 2;
    const int w = hd[0], h = hd[1], n = hd[2], format = hd[3], stride = hd[4], ofs = hd[5] & 15;
    int64_t span = 0;
    try {
        const FrameSettings s = propose_pixel_format(FrameSettings{}, format);
        frame_settings_rules(s, SET_YUV_DESCRIPTION, false);
        if (format == SLIDEO_PIXEL_BGR8) fail(SLIDEO_ERR_INVALID_ARG, "SLIDEO_PIXEL_BGR8 frames are not converted");
        span = pixel_format_validate(format, w, h, stride, n > 1 ? fs : -1);
    } catch (const Error& e) { std::fprintf(stderr, "%d %s\n", e.code, e.what()); return 3; }
    const size_t total = (size_t)(fs * (n - 1) + span);
    // malloc's blocks are 16-byte aligned: the source starts `ofs` bytes in and ends with the block
    uint8_t* exact = static_cast<uint8_t*>(std::malloc(ofs + total));
    if (!exact || (uintptr_t)exact % 16 != 0) return 2;
    uint8_t* src = exact + ofs;
    if (std::fread(src, 1, total, f) != total) return 2;
    std::fclose(f);
    const size_t ob = (size_t)w * h * 3 * n;
    uint8_t* dst = static_cast<uint8_t*>(std::malloc(ob));
    const PixArgs a = pixels_args(format, src, fs, stride, w, h, n, dst);
    const int form = pixel_format_form(format);
    if (form == PIX_PACKED3) run_grid<PIX_PACKED3>(a, n);
    else if (form == PIX_PACKED4) run_grid<PIX_PACKED4>(a, n);
    else run_grid<PIX_PLANAR>(a, n);
    f = std::fopen(outp, "wb");
    if (!f || std::fwrite(dst, 1, ob, f) != ob) return 2;
    std::fclose(f);
    std::free(dst);
    std::free(exact);
    std::printf("wide %d out4 %d\n", a.wide, a.out4);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc >= 4 && !std::strcmp(argv[1], "convert")) return convert(argv[2], argv[3]);
    if (argc >= 7 && !std::strcmp(argv[1], "validate")) {
        try {
            std::printf("0 %lld\n", (long long)pixel_format_validate(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]),
                                                                     std::atoll(argv[6])));
        } catch (const Error& e) { std::printf("%d %s\n", e.code, e.what()); }
        return 0;
    }
    if (argc >= 2 && !std::strcmp(argv[1], "set")) {
        FrameSettings s{};
        for (int i = 2; i < argc; ++i) {
            try {
                const FrameSettings next = propose_pixel_format(s, std::atoi(argv[i]));
                frame_settings_rules(next, SET_YUV_DESCRIPTION, false);
                s = next;
                std::printf("0 ok\n");
            } catch (const Error& e) { std::printf("%d %s\n", e.code, e.what()); }
        }
        std::printf("state %d\n", s.pixel_format);
        return 0;
    }
    if (argc >= 3 && !std::strcmp(argv[1], "info")) {
        int bpp = 0, planes = 0, b = 0, g = 0, r = 0;
        const int format = std::atoi(argv[2]);
        const bool ok = pixel_format_info(format, &bpp, &planes);
        if (ok) pixel_format_channels(format, &b, &g, &r);
        std::printf("%d %d %d %d %d %d\n", ok ? 1 : 0, bpp, planes, b, g, r);
        return 0;
    }
    std::fprintf(stderr, "usage: %s convert <case> <out> | validate format w h stride frame_stride | set <format> ... | info <format>\n", argv[0]);
    return 2;
}
