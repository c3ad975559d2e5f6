// placement_hostcheck — the per-frame body of csrc/placement.hip.h (placement_frame, placement_nearest, placement_rows,
// placement_sums, compiled for the host) run block by block as placement_kernel runs it: per frame the contributor, then per window of
// PL_WIN keypoints the slots reset and every thread index through each of the three phases.  For tests/test_placement_abi.py, which
// compares the sums with tests/placement_ref.py.  Every array lives in a heap allocation of exactly its size — the keypoints, the
// page coordinates, the votes (qtot * k entries, a frame's at qofs[f] * k, as on the device), the FrameCands, the page records, the
// slots, the accumulators —, so a load or store past any end is the sanitizer's to report.
//   g++ -O1 -g -std=c++17 [-fsanitize=address,undefined] -I include -I slideo_amd/csrc tools/placement_hostcheck.cpp -o hostcheck
//   hostcheck <unit> <out>
//       <unit>: int32 {model, k, aw, ah, min_inliers, cell, 0, n, ntrain, qtot, flags word, rerun mask, npages, 0, 0, 0}, double reach,
//       then qofs u32 [n + 1], keypoints [qtot] (24 bytes each), page_xy f32 [ntrain][2], votes u32 [qtot * k][2], per frame int32
//       ncand and per candidate int32 {page, count, ofs, inliers, found}, double M[9]; per page int32 {w, h}.
//       <out>: n, sfx, sfy, su, sv u64 [gh][gw] each, frames_counted u64.  Prints "frames <counted> windows <most windows a frame took>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "placement.hip.h"

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
    if (argc != 3) { std::fprintf(stderr, "usage: %s <unit> <out>\n", argv[0]); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hd[16];
    double reach;
    if (std::fread(hd, 4, 16, f) != 16 || std::fread(&reach, 8, 1, f) != 1) return 2;
    const int model = hd[0], k = hd[1], aw = hd[2], ah = hd[3], cell = hd[5], n = hd[7], ntrain = hd[8], npages = hd[12];
    const size_t qtot = (size_t)hd[9];
    if (n < 0 || k < 1 || aw < 1 || ah < 1 || npages < 0 || !evidence_cell_ok(cell)) return 2;
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
            if (rec[0] < 0 || rec[0] >= npages) return 3;
            fcs[i].page[j] = rec[0]; fcs[i].count[j] = rec[1]; fcs[i].ofs[j] = rec[2]; fcs[i].inliers[j] = rec[3]; fcs[i].found[j] = rec[4];
        }
    }
    std::unique_ptr<PageInfo[]> pages(new PageInfo[(size_t)npages]);
    std::memset(static_cast<void*>(pages.get()), 0, sizeof(PageInfo) * (size_t)npages);
    for (int p = 0; p < npages; ++p) {
        int32_t rec[2];
        if (std::fread(rec, 4, 2, f) != 2) return 2;
        pages[p].w = rec[0]; pages[p].h = rec[1];
    }
    std::fclose(f);

    const int gw = (aw + cell - 1) / cell, gh = (ah + cell - 1) / cell;
    const size_t nc = (size_t)gw * gh;
    std::unique_ptr<unsigned long long[]> acc(new unsigned long long[5 * nc + 1]());
    std::unique_ptr<uint32_t[]> flags(new uint32_t[1]{(uint32_t)hd[10]});
    std::unique_ptr<unsigned long long[]> d2min(new unsigned long long[PL_WIN]);
    std::unique_ptr<uint32_t[]> tmin(new uint32_t[PL_WIN]);

    PlacementArgs a{};
    a.ev.fcs = fcs.get(); a.ev.qofs = qofs.get(); a.ev.kp = kp.get(); a.ev.page_xy = page_xy.get(); a.ev.votes = votes.get();
    a.ev.flags = flags.get(); a.ev.rerun_mask = (uint32_t)hd[11];
    a.ev.k = k; a.ev.model = model;
    a.pageinfo = pages.get();
    a.reach2 = reach * reach;
    a.aw = aw; a.ah = ah; a.cell = cell; a.gw = gw; a.gh = gh; a.min_inliers = hd[4];
    a.acc = acc.get();

    long most_windows = 0;
    for (int fr = 0; fr < n; ++fr) {                                   // one block per frame
        const PlacementFrame e = placement_frame(a, fr);
        if (e.slot < 0) continue;
        acc[5 * nc] += 1;
        if (e.n == 0 || e.count <= 0) continue;
        long windows = 0;
        for (uint32_t base = 0; base < e.n; base += PL_WIN) {
            ++windows;
            for (int i = 0; i < PL_WIN; ++i) { d2min[i] = PL_NONE64; tmin[i] = PL_NONE32; }
            for (int tid = 0; tid < PL_THREADS; ++tid)
                placement_nearest(a, e, base, tid, PL_THREADS, d2min.get(), [](unsigned long long* p, unsigned long long v) { if (v < *p) *p = v; });
            for (int tid = 0; tid < PL_THREADS; ++tid)
                placement_rows(a, e, base, tid, PL_THREADS, d2min.get(), tmin.get(), [](uint32_t* p, uint32_t v) { if (v < *p) *p = v; });
            for (int tid = 0; tid < PL_THREADS; ++tid)
                placement_sums(a, e, base, tid, PL_THREADS, d2min.get(), tmin.get(), [](unsigned long long* p, unsigned long long v) { *p += v; });
        }
        most_windows = windows > most_windows ? windows : most_windows;
    }
    FILE* fo = std::fopen(argv[2], "wb");
    if (!fo) return 2;
    std::fwrite(acc.get(), 8, 5 * nc + 1, fo);
    std::fclose(fo);
    std::printf("frames %llu windows %ld\n", acc[5 * nc], most_windows);
    return 0;
}
