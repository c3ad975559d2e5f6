// shading_hostcheck — the per-thread body of csrc/shading.hip.h (shading_thread, both instances, compiled for the host) run lane by
// lane over its launch grid, the plain per-pixel rule of csrc/frame_settings.h, and the per-frame body of shading_map_kernel
// (tone_frame, tone_votes, shading_map_samples, shading_map_flush) run block by block as the kernel runs it, for
// tests/test_shading_abi.py, which compares with tests/shading_ref.py.
//   g++ -O1 -g -std=c++17 -ffp-contract=off [-fsanitize=address,undefined] -I include -I slideo_amd/csrc tools/shading_hostcheck.cpp -o hostcheck
//   hostcheck session <unit> <out> <cell> [tile rows]
//                                   <unit>: tools/tone_hostcheck.cpp's unit file, byte for byte.  Per frame the contributor, every
//                                   thread index through the vote phase and the merge of their boxes, then per row tile zeroed bins,
//                                   every thread index through the sample phase and through the flush.  [tile rows]: the rows of a
//                                   row tile in place of tone_tile_rows.  <out>: cnt, sum_f, sum_p u64 [gh * gw] each, then
//                                   frames_counted.  Prints "frames <counted> hits <hits of the counted frames> tiles <most tiles
//                                   a frame took> adds <LDS adds issued> samples <samples counted>".  Every array lives in a heap
//                                   allocation of exactly its size.
//   hostcheck apply <case> <out>    <case>: int32 {w, h, n, src_stride, dst_stride, src_offset, dst_offset, in_place, cell, with_lut},
//                                   the levels table (768 bytes, read when with_lut), the (gh + 1) * (gw + 1) uint16 gains, n frames
//                                   of h * src_stride bytes.  <out>: the destination buffer — in place the source buffer itself
//                                   (dst_stride and dst_offset unused).  Prints the paths taken, whether an out-of-place source is
//                                   unchanged, and whether the per-pixel rule of frame_settings.h gave the same bytes.
// Every buffer is a heap allocation of its exact size — an image ends with the last pixel of the last row of the last frame and
// begins `offset` bytes past a 16-byte boundary; the gains end with the last node — so that a sanitized build sees any access
// outside it or at a misaligned address.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "slideo_amd.h"
#include "frame_settings.h"
#define SHADING_MAP
#include "shading.hip.h"

using namespace slideo;

static bool read_file(const char* path, std::vector<uint8_t>& out) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    out.resize((size_t)n);
    const bool ok = std::fread(out.data(), 1, out.size(), f) == out.size();
    std::fclose(f);
    return ok;
}

static bool write_file(const char* path, const void* p, size_t n) {
    FILE* f = std::fopen(path, "wb");
    if (!f) return false;
    const bool ok = std::fwrite(p, 1, n, f) == n;
    std::fclose(f);
    return ok;
}

static size_t span(int w, int h, int n, int stride) { return (size_t)h * stride * (n - 1) + (size_t)(h - 1) * stride + (size_t)w * 3; }

static int run_apply(const char* cin, const char* cout) {
    std::vector<uint8_t> file;
    if (!read_file(cin, file) || file.size() < 40 + 768) return 2;
    int32_t hd[10];
    std::memcpy(hd, file.data(), 40);
    const int w = hd[0], h = hd[1], n = hd[2], ss = hd[3], ds = hd[4], sofs = hd[5] & 15, dofs = hd[6] & 15, in_place = hd[7], cell = hd[8], with_lut = hd[9];
    if (w < 1 || h < 1 || n < 1 || ss < 3 * w || (!in_place && ds < 3 * w) || !shading_cell_ok(cell)) return 2;
    const uint8_t* lut = file.data() + 40;
    const int gw = (w + cell - 1) / cell, gh = (h + cell - 1) / cell;
    const size_t nodes = (size_t)(gw + 1) * (gh + 1), sfb = (size_t)h * ss, dfb = (size_t)h * ds, head = 40 + 768 + nodes * 2;
    if (file.size() != head + sfb * n) return 2;
    uint16_t* gains = static_cast<uint16_t*>(std::malloc(nodes * 2));
    if (!gains) return 2;
    std::memcpy(gains, file.data() + 40 + 768, nodes * 2);
    const size_t stot = span(w, h, n, ss), dtot = in_place ? stot : span(w, h, n, ds);
    // exact-size blocks: malloc returns 16-byte aligned memory; the image begins `offset` bytes into it and ends at its last byte
    uint8_t* sraw = static_cast<uint8_t*>(std::malloc(sofs + stot));
    uint8_t* draw = in_place ? nullptr : static_cast<uint8_t*>(std::malloc(dofs + dtot));
    if (!sraw || (!in_place && !draw)) return 2;
    uint8_t* src = sraw + sofs;
    std::memcpy(src, file.data() + head, stot);
    uint8_t* dst = in_place ? src : draw + dofs;
    if (!in_place) std::memset(dst, 0xAA, dtot);
    const ShadingArgs a = shading_args(gains, cell, with_lut ? lut : nullptr, src, (int64_t)sfb, ss, dst, in_place ? (int64_t)sfb : (int64_t)dfb,
                                       in_place ? ss : ds, w, h, n);
    const int gx = ((w + 3) / 4 + LVL_TX - 1) / LVL_TX, gy = (h + LVL_TY - 1) / LVL_TY;
    for (int z = 0; z < n; ++z)
        for (int by = 0; by < gy; ++by)
            for (int bx = 0; bx < gx; ++bx)
                for (int ty = 0; ty < LVL_TY; ++ty)
                    for (int tx = 0; tx < LVL_TX; ++tx) {
                        if (with_lut) shading_thread<true>(a, lut, bx * LVL_TX + tx, by * LVL_TY + ty, z);
                        else shading_thread<false>(a, nullptr, bx * LVL_TX + tx, by * LVL_TY + ty, z);
                    }
    const int unchanged = in_place ? -1 : std::memcmp(src, file.data() + head, stot) == 0;
    // the plain rule, pixel by pixel, on the case's own bytes
    int rule = 1;
    const uint8_t* in = file.data() + head;
    const int dstride = in_place ? ss : ds;
    for (int z = 0; z < n && rule; ++z)
        for (int y = 0; y < h && rule; ++y)
            for (int x = 0; x < w * 3; ++x) {
                uint8_t v = frame_shading_pixel(gains, gw, cell, x / 3, y, in[(size_t)z * sfb + (size_t)y * ss + x]);
                if (with_lut) v = lut[(x % 3) * 256 + v];
                if (dst[(size_t)z * (in_place ? sfb : dfb) + (size_t)y * dstride + x] != v) { rule = 0; break; }
            }
    if (!write_file(cout, dst, dtot)) return 2;
    std::printf("in4 %d out4 %d place %d lut %d src_unchanged %d rule %d\n", a.img.in4, a.img.out4, in_place ? 1 : 0, with_lut ? 1 : 0, unchanged, rule);
    std::free(sraw); std::free(draw); std::free(gains);
    return 0;
}

template <class T>
static std::unique_ptr<T[]> read_exact(FILE* f, size_t n) {
    std::unique_ptr<T[]> p(new T[n]);                // (n == 0: a valid zero-size allocation, never dereferenced)
    if (n && std::fread(p.get(), sizeof(T), n, f) != n) { std::fprintf(stderr, "short read\n"); std::exit(2); }
    return p;
}

static long g_adds = 0;

static int run_session(const char* cin, const char* cout, int cell, int tile_rows) {
    if (!shading_cell_ok(cell)) return 2;
    FILE* f = std::fopen(cin, "rb");
    if (!f) return 2;
    int32_t hd[16];
    double thr;
    if (std::fread(hd, 4, 16, f) != 16 || std::fread(&thr, 8, 1, f) != 1) return 2;
    const int model = hd[0], k = hd[1], aw = hd[2], ah = hd[3], n = hd[7], ntrain = hd[8], npages = hd[12];
    const size_t qtot = (size_t)hd[9];
    if (n < 0 || k < 1 || aw < 1 || ah < 1 || npages < 0) return 2;
    static_assert(sizeof(slideo_keypoint) == 24 && sizeof(EvVote) == 8 && sizeof(EvXY) == 8, "record sizes");
    auto qofs = read_exact<uint32_t>(f, (size_t)n + 1);
    auto kp = read_exact<slideo_keypoint>(f, qtot);
    auto page_xy = read_exact<EvXY>(f, (size_t)ntrain);
    auto votes = read_exact<EvVote>(f, qtot * (size_t)k);
    std::unique_ptr<FrameCands[]> fcs(new FrameCands[(size_t)n]);
    std::memset(static_cast<void*>(fcs.get()), 0, sizeof(FrameCands) * (size_t)n);
    for (int i = 0; i < n; ++i) {
        int32_t nc;
        if (std::fread(&nc, 4, 1, f) != 1 || nc < 0 || nc > MAXC) return 2;
        fcs[i].ncand = nc;
        for (int j = 0; j < nc; ++j) {
            int32_t rec[5];
            if (std::fread(rec, 4, 5, f) != 5 || std::fread(fcs[i].M[j], 8, 9, f) != 9) return 2;
            fcs[i].page[j] = rec[0]; fcs[i].count[j] = rec[1]; fcs[i].ofs[j] = rec[2]; fcs[i].inliers[j] = rec[3]; fcs[i].found[j] = rec[4];
        }
    }
    std::unique_ptr<PageInfo[]> pages(new PageInfo[(size_t)npages]);
    std::memset(static_cast<void*>(pages.get()), 0, sizeof(PageInfo) * (size_t)npages);
    size_t small_bytes = 0;
    for (int p = 0; p < npages; ++p) {
        int32_t rec[4];
        if (std::fread(rec, 4, 4, f) != 4 || rec[2] < 1 || rec[3] < 1) return 2;
        pages[p].w = rec[0]; pages[p].h = rec[1]; pages[p].sw = rec[2]; pages[p].sh = rec[3];
        pages[p].small_ofs = (int64_t)small_bytes;
        small_bytes += (size_t)rec[2] * rec[3] * 3;
    }
    auto smalls = read_exact<uint8_t>(f, small_bytes);
    const size_t frame_bytes = (size_t)aw * ah * 3;
    auto frames = read_exact<uint8_t>(f, frame_bytes * (size_t)n);
    std::fclose(f);

    const int gw = (aw + cell - 1) / cell, gh = (ah + cell - 1) / cell, cells = gw * gh;
    if (cells > SHM_MAX_CELLS) return 2;
    std::unique_ptr<unsigned long long[]> acc(new unsigned long long[3 * (size_t)cells + 1]());
    std::unique_ptr<uint32_t[]> flags(new uint32_t[1]{(uint32_t)hd[10]});
    std::unique_ptr<uint32_t[]> bins(new uint32_t[3 * (size_t)cells]);

    ShadingMapArgs a{};
    a.t.ev.fcs = fcs.get(); a.t.ev.qofs = qofs.get(); a.t.ev.kp = kp.get(); a.t.ev.page_xy = page_xy.get(); a.t.ev.votes = votes.get();
    a.t.ev.flags = flags.get(); a.t.ev.rerun_mask = (uint32_t)hd[11];
    a.t.ev.k = k; a.t.ev.model = model; a.t.ev.thr2 = thr * thr;
    a.t.pageinfo = pages.get(); a.t.page_small = smalls.get();
    a.t.frames = frames.get(); a.t.frame_stride = (int64_t)frame_bytes; a.t.stride = aw * 3; a.t.aw = aw; a.t.ah = ah;
    a.t.min_inliers = hd[4]; a.t.min_hits = hd[5]; a.t.flat = hd[6];
    a.shift = cell == 16 ? 4 : cell == 32 ? 5 : 6; a.gw = gw; a.cells = cells;
    a.acc = acc.get();

    long hits = 0, most_tiles = 0;
    for (int fr = 0; fr < n; ++fr) {                                   // one block per frame
        const ToneFrame e = tone_frame(a.t, fr);
        if (e.slot < 0) continue;
        if (e.page < 0 || e.page >= npages) return 3;
        ToneBox box = tone_box_empty();
        for (int tid = 0; tid < TONE_THREADS; ++tid) {
            const ToneBox m = tone_votes(a.t, e, tid, TONE_THREADS);
            if (!m.hits) continue;
            box.hits += m.hits;
            box.x0 = m.x0 < box.x0 ? m.x0 : box.x0; box.y0 = m.y0 < box.y0 ? m.y0 : box.y0;
            box.x1 = m.x1 > box.x1 ? m.x1 : box.x1; box.y1 = m.y1 > box.y1 ? m.y1 : box.y1;
        }
        if (box.hits < a.t.min_hits) continue;
        const PageInfo& pi = pages[e.page];
        const int rows = tile_rows > 0 ? tile_rows : tone_tile_rows(pi.sw);
        long tiles = 0;
        for (int j0 = 0; j0 < pi.sh; j0 += rows) {
            ++tiles;
            std::memset(bins.get(), 0, sizeof(uint32_t) * 3 * (size_t)cells);
            for (int tid = 0; tid < TONE_THREADS; ++tid)
                shading_map_samples(a, e, box, fr, j0, j0 + rows < pi.sh ? j0 + rows : pi.sh, tid, TONE_THREADS, bins.get(),
                                    [](uint32_t* p, uint32_t v) { *p += v; ++g_adds; });
            for (int tid = 0; tid < TONE_THREADS; ++tid)
                shading_map_flush(a, tid, TONE_THREADS, bins.get(), [](unsigned long long* p, unsigned long long v) { *p += v; });
        }
        acc[3 * (size_t)cells] += 1;
        hits += box.hits;
        most_tiles = tiles > most_tiles ? tiles : most_tiles;
    }
    if (!write_file(cout, acc.get(), (3 * (size_t)cells + 1) * 8)) return 2;
    unsigned long long samples = 0;
    for (int c = 0; c < cells; ++c) samples += acc[c];
    std::printf("frames %llu hits %ld tiles %ld adds %ld samples %llu\n", acc[3 * (size_t)cells], hits, most_tiles, g_adds, samples);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s apply <case> <out> | session <unit> <out> <cell> [tile rows]\n", argv[0]); return 2; }
    const std::string mode = argv[1];
    try {
        if (mode == "apply" && argc == 4) return run_apply(argv[2], argv[3]);
        if (mode == "session" && (argc == 5 || argc == 6)) return run_session(argv[2], argv[3], std::atoi(argv[4]), argc == 6 ? std::atoi(argv[5]) : 0);
    } catch (const Error& e) {
        std::printf("%d %s\n", e.code, e.what());
        return 0;
    }
    std::fprintf(stderr, "bad arguments\n");
    return 2;
}
