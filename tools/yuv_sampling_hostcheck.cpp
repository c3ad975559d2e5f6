// yuv_sampling_hostcheck — the per-thread body of csrc/yuv_sampling.hip.h (yuv_sampled_thread, compiled for the host) run lane by lane
// over the whole launch grid, and the host rules of csrc/frame_settings.h that go with "YUV sampling", for
// tests/test_yuv_sampling_abi.py, which compares the outcome with tests/yuv_sampling_ref.py.
//   g++ -O1 -g -std=c++17 [-fsanitize=address,undefined] -I include -I slideo_amd/csrc tools/yuv_sampling_hostcheck.cpp -o hostcheck
//   hostcheck convert <case> <out>
//       <case>: int32 {w, h, n, matrix, range, depth, sampling, y_stride, uv_stride, uv_step, src_offset, 0}, int64 {u_offset,
//       v_offset, frame_stride}, then the frames: (n - 1) * frame_stride + span bytes.  <out>: n images of h x w x 3.  The source
//       is copied to `src_offset` bytes past the 16-byte aligned base of an allocation that ends with the last frame byte, and the
//       destination is exact-size too: a load or store past either end is the sanitizer's to report, and so is a wide load at an
//       address that is not a multiple of its size.  Prints the wide-load flags the host chose.
//   hostcheck validate sampling w h y_stride uv_stride u_offset v_offset uv_step frame_stride bytes_per_sample
//       prints "<code> <message>" of yuv420_validate (code 0: "0 <span>")
//   hostcheck set <op> <value> ...      op: s <sampling> | d <matrix> <range> <depth>
//       walks the set calls in order over one FrameSettings as settings_commit does (proposal, then the rules between settings; a
//       refused call leaves the record as it was) and prints per call "<code> <message>", then "state matrix range depth sampling"
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "frame_settings.h"
#include "yuv_sampling.hip.h"

using namespace slideo;

namespace {

template <int SAMPLING, int DEPTH>
void run_grid(const YuvArgs& a, const YuvCoef& k, int n) {
    const int gx = ((a.w + 3) / 4 + YUV_TX - 1) / YUV_TX, gy = (a.h + YUV_TY - 1) / YUV_TY;
    for (int z = 0; z < n; ++z)
        for (int by = 0; by < gy; ++by)
            for (int bx = 0; bx < gx; ++bx)
                for (int ty = 0; ty < YUV_TY; ++ty)
                    for (int tx = 0; tx < YUV_TX; ++tx) yuv_sampled_thread<SAMPLING, DEPTH>(a, k, bx * YUV_TX + tx, by * YUV_TY + ty, z);
}

template <int SAMPLING>
void run_depth(int depth, const YuvArgs& a, const YuvCoef& k, int n) {
    if (depth == SLIDEO_YUV_DEPTH_8) run_grid<SAMPLING, YUV_D8>(a, k, n);
    else if (depth == SLIDEO_YUV_DEPTH_10_MSB) run_grid<SAMPLING, YUV_D10_MSB>(a, k, n);
    else run_grid<SAMPLING, YUV_D10_LSB>(a, k, n);
}

int convert(const char* in, const char* outp) {
    FILE* f = std::fopen(in, "rb");
    if (!f) return 2;
    int32_t hd[12];
    int64_t of[3];
    if (std::fread(hd, 4, 12, f) != 12 || std::fread(of, 8, 3, f) != 3) return 2;
    const int w = hd[0], h = hd[1], n = hd[2], matrix = hd[3], range = hd[4], depth = hd[5], sampling = hd[6], ofs = hd[10] & 15;
    slideo_yuv420_layout L{};
    L.y_stride = hd[7]; L.uv_stride = hd[8]; L.uv_step = hd[9]; L.u_offset = of[0]; L.v_offset = of[1];
    const int64_t fs = of[2];
    int64_t span = 0;
    try {
        FrameSettings s = propose_yuv_description(FrameSettings{}, matrix, range, depth);
        s = propose_yuv_sampling(s, sampling);
        frame_settings_rules(s, SET_YUV_DESCRIPTION, false);
        if (sampling == SLIDEO_YUV_SAMPLING_420) fail(SLIDEO_ERR_INVALID_ARG, "4:2:0 has its own kernels (tools/yuv_desc_hostcheck.cpp)");
        span = yuv420_validate(w, h, &L, n > 1 ? fs : -1, s.yuv.bytes_per_sample(), sampling);
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
    int32_t c[7];
    yuv_coefficients(matrix, range, c);
    const YuvCoef k{c[0], c[1], c[2], c[3], c[4], c[5]};
    const YuvArgs a = yuv_sampled_args(sampling, depth, src, fs, L, w, h, n, dst);
    if (sampling == SLIDEO_YUV_SAMPLING_422_PACKED) run_grid<YUV_S422P, YUV_D8>(a, k, n);
    else if (sampling == SLIDEO_YUV_SAMPLING_422) run_depth<YUV_S422>(depth, a, k, n);
    else run_depth<YUV_S444>(depth, a, k, n);
    f = std::fopen(outp, "wb");
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
    if (argc >= 12 && !std::strcmp(argv[1], "validate")) {
        slideo_yuv420_layout L{};
        const int sampling = std::atoi(argv[2]), w = std::atoi(argv[3]), h = std::atoi(argv[4]);
        L.y_stride = std::atoi(argv[5]); L.uv_stride = std::atoi(argv[6]); L.u_offset = std::atoll(argv[7]); L.v_offset = std::atoll(argv[8]);
        L.uv_step = std::atoi(argv[9]);
        try {
            std::printf("0 %lld\n", (long long)yuv420_validate(w, h, &L, std::atoll(argv[10]), std::atoi(argv[11]), sampling));
        } catch (const Error& e) { std::printf("%d %s\n", e.code, e.what()); }
        return 0;
    }
    if (argc >= 2 && !std::strcmp(argv[1], "set")) {
        FrameSettings s{};
        for (int i = 2; i < argc;) {
            const bool samp = !std::strcmp(argv[i], "s");
            const int at = i;
            i += samp ? 2 : 4;
            if ((!samp && std::strcmp(argv[at], "d")) || i > argc) return 2;
            try {
                const FrameSettings next = samp ? propose_yuv_sampling(s, std::atoi(argv[at + 1]))
                                                : propose_yuv_description(s, std::atoi(argv[at + 1]), std::atoi(argv[at + 2]), std::atoi(argv[at + 3]));
                frame_settings_rules(next, SET_YUV_DESCRIPTION, false);
                s = next;
                std::printf("0 ok\n");
            } catch (const Error& e) { std::printf("%d %s\n", e.code, e.what()); }
        }
        std::printf("state %d %d %d %d\n", s.yuv.matrix, s.yuv.range, s.yuv.depth, s.yuv.sampling);
        return 0;
    }
    std::fprintf(stderr, "usage: %s convert <case> <out> | validate sampling w h ... | set (s <sampling> | d <matrix> <range> <depth>) ...\n", argv[0]);
    return 2;
}
