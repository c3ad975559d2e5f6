// tone_hostcheck — the per-frame body of csrc/tone.hip.h (tone_frame, tone_votes, tone_samples, tone_flush, compiled for the host) run
// block by block as tone_kernel runs it: per frame the contributor, every thread index through the vote phase and the merge of
// their boxes, then per row tile zeroed bins, every thread index through the sample phase and through the flush.  For
// tests/test_tone_abi.py, which compares the counts with tests/tone_ref.py.  Every array lives in a heap allocation of exactly its
// size — the keypoints, the page coordinates, the votes (qtot * k entries, a frame's at qofs[f] * k, as on the device), the
// FrameCands, the page records, the small images, the frames, the bins, the accumulators —, so a load or store past any end is the
// sanitizer's to report.
//   g++ -O1 -g -std=c++17 [-fsanitize=address,undefined] -I include -I slideo_amd/csrc tools/tone_hostcheck.cpp -o hostcheck
//   hostcheck <unit> <out> [tile rows]
//       <unit>: int32 {model, k, aw, ah, min_inliers, min_hits, flat, n, ntrain, qtot, flags word, rerun mask, npages, 0, 0, 0},
//       double thr, then qofs u32 [n + 1], keypoints [qtot] (24 bytes each), page_xy f32 [ntrain][2], votes u32 [qtot * k][2], per
//       frame int32 ncand and per candidate int32 {page, count, ofs, inliers, found}, double M[9]; per page int32 {w, h, sw, sh}; the
//       small images back to back; the n frames (ah rows of aw * 3 bytes) back to back.
//       [tile rows]: the rows of a row tile in place of tone_tile_rows (the tests walk small images in several tiles with it).
//       <out>: cnt u64 [3][256], sum u64 [3][256], frames_counted u64.  Prints "frames <counted> hits <hits of the counted frames>
//       tiles <most tiles a frame took>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "tone.hip.h"

using namespace slideo;

namespace {

template <class T>
std::unique_ptr<T[]> read_exact(FILE* f, size_t n) {
    std::unique_ptr<T[]> p(new T[n]);                // (n == 0: a valid zero-size allocation, never dereferenced)
    if (n && std::fread(p.get(), sizeof(T), n, f) != n) { std::fprintf(stderr, "short read\n"); std::exit(2); }
    return p;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3 && argc != 4) { std::fprintf(stderr, "usage: %s <unit> <out> [tile rows]\n", argv[0]); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hd[16];
    double thr;
    if (std::fread(hd, 4, 16, f) != 16 || std::fread(&thr, 8, 1, f) != 1) return 2;
    const int model = hd[0], k = hd[1], aw = hd[2], ah = hd[3], n = hd[7], ntrain = hd[8], npages = hd[12];
    const size_t qtot = (size_t)hd[9];
    if (n < 0 || k < 1 || aw < 1 || ah < 1 || npages < 0) return 2;
    const int tile_rows = argc == 4 ? std::atoi(argv[3]) : 0;
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

    std::unique_ptr<unsigned long long[]> acc(new unsigned long long[TONE_BINS + 1]());
    std::unique_ptr<uint32_t[]> flags(new uint32_t[1]{(uint32_t)hd[10]});
    std::unique_ptr<uint32_t[]> bins(new uint32_t[TONE_BINS]);

    ToneArgs a{};
    a.ev.fcs = fcs.get(); a.ev.qofs = qofs.get(); a.ev.kp = kp.get(); a.ev.page_xy = page_xy.get(); a.ev.votes = votes.get();
    a.ev.flags = flags.get(); a.ev.rerun_mask = (uint32_t)hd[11];
    a.ev.k = k; a.ev.model = model; a.ev.thr2 = thr * thr;
    a.pageinfo = pages.get(); a.page_small = smalls.get();
    a.frames = frames.get(); a.frame_stride = (int64_t)frame_bytes; a.stride = aw * 3; a.aw = aw; a.ah = ah;
    a.min_inliers = hd[4]; a.min_hits = hd[5]; a.flat = hd[6];
    a.acc = acc.get();

    long hits = 0, most_tiles = 0;
    for (int fr = 0; fr < n; ++fr) {                                   // one block per frame
        const ToneFrame e = tone_frame(a, fr);
        if (e.slot < 0) continue;
        if (e.page < 0 || e.page >= npages) return 3;
        ToneBox box = tone_box_empty();
        for (int tid = 0; tid < TONE_THREADS; ++tid) {
            const ToneBox m = tone_votes(a, e, tid, TONE_THREADS);
            if (!m.hits) continue;
            box.hits += m.hits;
            box.x0 = m.x0 < box.x0 ? m.x0 : box.x0; box.y0 = m.y0 < box.y0 ? m.y0 : box.y0;
            box.x1 = m.x1 > box.x1 ? m.x1 : box.x1; box.y1 = m.y1 > box.y1 ? m.y1 : box.y1;
        }
        if (box.hits < a.min_hits) continue;
        const PageInfo& pi = pages[e.page];
        const int rows = tile_rows > 0 ? tile_rows : tone_tile_rows(pi.sw);
        long tiles = 0;
        for (int j0 = 0; j0 < pi.sh; j0 += rows) {
            ++tiles;
            std::memset(bins.get(), 0, sizeof(uint32_t) * TONE_BINS);
            for (int tid = 0; tid < TONE_THREADS; ++tid)
                tone_samples(a, e, box, fr, j0, j0 + rows < pi.sh ? j0 + rows : pi.sh, tid, TONE_THREADS, bins.get(),
                             [](uint32_t* p, uint32_t v) { *p += v; });
            for (int tid = 0; tid < TONE_THREADS; ++tid)
                tone_flush(a, tid, TONE_THREADS, bins.get(), [](unsigned long long* p, unsigned long long v) { *p += v; });
        }
        acc[TONE_BINS] += 1;
        hits += box.hits;
        most_tiles = tiles > most_tiles ? tiles : most_tiles;
    }
    FILE* fo = std::fopen(argv[2], "wb");
    if (!fo) return 2;
    std::fwrite(acc.get(), 8, TONE_BINS + 1, fo);
    std::fclose(fo);
    std::printf("frames %llu hits %ld tiles %ld\n", acc[TONE_BINS], hits, most_tiles);
    return 0;
}
