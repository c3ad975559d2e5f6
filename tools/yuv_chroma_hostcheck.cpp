// yuv_chroma_hostcheck — the per-thread body of csrc/yuv_chroma.hip.h (yuv_chroma_thread, compiled for the host) run lane by lane
// over the whole launch grid, and the host rules of csrc/frame_settings.h that go with "YUV chroma filter", for
// tests/test_yuv_chroma_abi.py, which compares the outcome with tests/yuv_chroma_ref.py.  The cross-lane exchange of the kernel is
// one hook (yuv_chroma_exchange); here it computes the neighbour lane's dword directly.
//   g++ -O1 -g -std=c++17 [-fsanitize=address,undefined] -I include -I slideo_amd/csrc tools/yuv_chroma_hostcheck.cpp -o hostcheck
//   hostcheck convert <cases> <out>
//       <cases>: any number of records, each int32 {w, h, n, matrix, range, depth, sampling, y_stride, uv_stride, uv_step, filter,
//       data bytes}, int64 {u_offset, v_offset, frame_stride}, then `data bytes` of frames, of which the first (n - 1) *
//       frame_stride + span are the frames' (the rest is padding behind the last frame).  <out>: per record n images of h x w x 3.
//       Every record is converted with its source 0, 1, 2, 4 and 8 bytes past the 16-byte aligned base of an allocation that ends
//       with the last frame byte, into an exact-size destination: a load or store past either end is the sanitizer's to report, and
//       so is a wide load at an address that is not a multiple of its size.  The five images must agree (exit 4 if not); the first
//       is written.  Prints how often each load and store path was taken.
//   hostcheck set <op> <value> ...      op: c <filter> | s <sampling> | d <matrix> <range> <depth>
//       walks the set calls in order over one FrameSettings as settings_commit does (proposal, then the rules between settings; a
//       refused call leaves the record as it was) and prints per call "<code> <message>", then "state matrix range depth sampling
//       filter"
//   hostcheck weights <filter> <sampling>      prints "<code>" and the twelve integers of yuv_chroma_weights
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

struct Hits {
    long wide_y, bytes_y, packed8, packed4, wide_c8, wide_c4, wide_c2, bytes_c, neighbour, halo, clamp, out4, out_bytes;
};
static Hits g_hits;
#define YUV_CHROMA_HIT(path) (++g_hits.path)

#include "frame_settings.h"
#include "yuv_chroma.hip.h"

using namespace slideo;

namespace {

template <int SAMPLING, int DEPTH>
void run_grid(const YuvArgs& a, const YuvChromaW& cw, const YuvCoef& k, int n) {
    const int rows = SAMPLING == YUV_S420 ? a.h / 2 : a.h;
    const int gx = ((a.w + 3) / 4 + YUV_TX - 1) / YUV_TX, gy = (rows + YUV_TY - 1) / YUV_TY;
    for (int z = 0; z < n; ++z)
        for (int by = 0; by < gy; ++by)
            for (int bx = 0; bx < gx; ++bx)
                for (int ty = 0; ty < YUV_TY; ++ty)
                    for (int tx = 0; tx < YUV_TX; ++tx) yuv_chroma_thread<SAMPLING, DEPTH>(a, cw, k, bx * YUV_TX + tx, tx, by * YUV_TY + ty, z);
}

template <int SAMPLING>
void run_depth(int depth, const YuvArgs& a, const YuvChromaW& cw, const YuvCoef& k, int n) {
    if (depth == SLIDEO_YUV_DEPTH_8) run_grid<SAMPLING, YUV_D8>(a, cw, k, n);
    else if (depth == SLIDEO_YUV_DEPTH_10_MSB) run_grid<SAMPLING, YUV_D10_MSB>(a, cw, k, n);
    else run_grid<SAMPLING, YUV_D10_LSB>(a, cw, k, n);
}

int convert(const char* in, const char* outp) {
    FILE* f = std::fopen(in, "rb");
    FILE* fo = std::fopen(outp, "wb");
    if (!f || !fo) return 2;
    int32_t hd[12];
    int64_t of[3];
    long records = 0;
    while (std::fread(hd, 4, 12, f) == 12) {
        if (std::fread(of, 8, 3, f) != 3) return 2;
        const int w = hd[0], h = hd[1], n = hd[2], matrix = hd[3], range = hd[4], depth = hd[5], sampling = hd[6], filter = hd[10];
        slideo_yuv420_layout L{};
        L.y_stride = hd[7]; L.uv_stride = hd[8]; L.uv_step = hd[9]; L.u_offset = of[0]; L.v_offset = of[1];
        const int64_t fs = of[2];
        int64_t span = 0;
        int32_t w12[12];
        try {
            FrameSettings s = propose_yuv_description(FrameSettings{}, matrix, range, depth);
            s = propose_yuv_sampling(s, sampling);
            s = propose_yuv_chroma(s, filter);
            frame_settings_rules(s, SET_YUV_DESCRIPTION, false);
            if (!s.yuv.filtered()) fail(SLIDEO_ERR_INVALID_ARG, "filter %d under sampling %d launches another kernel", filter, sampling);
            span = yuv420_validate(w, h, &L, n > 1 ? fs : -1, s.yuv.bytes_per_sample(), sampling);
        } catch (const Error& e) { std::fprintf(stderr, "record %ld: %d %s\n", records, e.code, e.what()); return 3; }
        if (!yuv_chroma_weights(filter, sampling, w12)) return 3;
        const size_t total = (size_t)(fs * (n - 1) + span);
        if (hd[11] < 0 || (size_t)hd[11] < total) return 2;
        std::vector<uint8_t> frames((size_t)hd[11]);
        if (std::fread(frames.data(), 1, frames.size(), f) != frames.size()) return 2;
        int32_t c[7];
        yuv_coefficients(matrix, range, c);
        const YuvCoef k{c[0], c[1], c[2], c[3], c[4], c[5]};
        const size_t ob = (size_t)w * h * 3 * n;
        std::vector<uint8_t> first;
        static const int OFS[5] = {0, 1, 2, 4, 8};
        for (int o = 0; o < 5; ++o) {
            // malloc's blocks are 16-byte aligned: the source starts OFS[o] bytes in and ends with the block
            uint8_t* exact = static_cast<uint8_t*>(std::malloc(OFS[o] + total));
            uint8_t* dst = static_cast<uint8_t*>(std::malloc(ob));
            if (!exact || !dst || (uintptr_t)exact % 16 != 0) return 2;
            std::memcpy(exact + OFS[o], frames.data(), total);
            std::memset(dst, 0xA5, ob);
            YuvArgs a;
            YuvChromaW cw;
            if (!yuv_chroma_args(sampling, depth, w12, exact + OFS[o], fs, L, w, h, n, dst, &a, &cw)) return 3;
            if (sampling == SLIDEO_YUV_SAMPLING_422_PACKED) run_grid<YUV_S422P, YUV_D8>(a, cw, k, n);
            else if (sampling == SLIDEO_YUV_SAMPLING_422) run_depth<YUV_S422>(depth, a, cw, k, n);
            else run_depth<YUV_S420>(depth, a, cw, k, n);
            if (o == 0) first.assign(dst, dst + ob);
            else if (std::memcmp(first.data(), dst, ob) != 0) {
                std::fprintf(stderr, "record %ld: the image at source offset %d differs from the one at offset 0\n", records, OFS[o]);
                return 4;
            }
            std::free(dst);
            std::free(exact);
        }
        if (std::fwrite(first.data(), 1, ob, fo) != ob) return 2;
        ++records;
    }
    std::fclose(f);
    std::fclose(fo);
    const Hits& g = g_hits;
    std::printf("records %ld\nwide_y %ld\nbytes_y %ld\npacked8 %ld\npacked4 %ld\nwide_c8 %ld\nwide_c4 %ld\nwide_c2 %ld\nbytes_c %ld\nneighbour %ld\nhalo %ld\n"
                "clamp %ld\nout4 %ld\nout_bytes %ld\n", records, g.wide_y, g.bytes_y, g.packed8, g.packed4, g.wide_c8, g.wide_c4, g.wide_c2, g.bytes_c,
                g.neighbour, g.halo, g.clamp, g.out4, g.out_bytes);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc >= 4 && !std::strcmp(argv[1], "convert")) return convert(argv[2], argv[3]);
    if (argc >= 4 && !std::strcmp(argv[1], "weights")) {
        int32_t w12[12] = {};
        const bool ok = yuv_chroma_weights(std::atoi(argv[2]), std::atoi(argv[3]), w12);
        std::printf("%d", ok ? 0 : 1);
        for (int i = 0; i < 12; ++i) std::printf(" %d", w12[i]);
        std::printf("\n");
        return 0;
    }
    if (argc >= 2 && !std::strcmp(argv[1], "set")) {
        FrameSettings s{};
        for (int i = 2; i < argc;) {
            const char op = argv[i][0];
            const int at = i;
            i += op == 'd' ? 4 : 2;
            if ((op != 'c' && op != 's' && op != 'd') || argv[at][1] || i > argc) return 2;
            try {
                const FrameSettings next = op == 'c'   ? propose_yuv_chroma(s, std::atoi(argv[at + 1]))
                                           : op == 's' ? propose_yuv_sampling(s, std::atoi(argv[at + 1]))
                                                       : propose_yuv_description(s, std::atoi(argv[at + 1]), std::atoi(argv[at + 2]), std::atoi(argv[at + 3]));
                frame_settings_rules(next, SET_YUV_DESCRIPTION, false);
                s = next;
                std::printf("0 ok\n");
            } catch (const Error& e) { std::printf("%d %s\n", e.code, e.what()); }
        }
        std::printf("state %d %d %d %d %d\n", s.yuv.matrix, s.yuv.range, s.yuv.depth, s.yuv.sampling, s.yuv.chroma);
        return 0;
    }
    std::fprintf(stderr, "usage: %s convert <cases> <out> | weights <filter> <sampling> | set (c <filter> | s <sampling> | d <matrix> <range> <depth>) ...\n", argv[0]);
    return 2;
}
