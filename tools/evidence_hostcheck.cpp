// evidence_hostcheck — the per-frame body of csrc/evidence.hip.h (evidence_frame, evidence_votes, evidence_count, compiled for the
// host) run block by block as evidence_kernel runs it: per frame, per window of EV_BITS keypoints, a zeroed bitset, every thread
// index through the vote phase, then every thread index through the count phase.  For tests/test_evidence_abi.py, which compares
// the counts with tests/evidence_ref.py.  Every array lives in a heap allocation of exactly its size — the keypoints, the page
// coordinates, the votes (qtot * k entries, a frame's at qofs[f] * k, as on the device), the FrameCands, the bitset, the counts —, so
// a load or store past any end is the sanitizer's to report.
//   g++ -O1 -g -std=c++17 [-fsanitize=address,undefined] -I include -I slideo_amd/csrc tools/evidence_hostcheck.cpp -o hostcheck
//   hostcheck <unit> <out>
//       <unit>: int32 {model, k, cell, aw, ah, min_inliers, n, ntrain, qtot, flags word, rerun mask, 0}, double thr, then
//       qofs u32 [n + 1], verdicts int32 [n][4], keypoints [qtot] (24 bytes each), page_xy f32 [ntrain][2], votes u32 [qtot * k][2],
//       then per frame int32 ncand and per candidate int32 {page, count, ofs}, double M[9].
//       <out>: seen u32 [gh][gw], then hit.  Prints "windows <most windows a frame took> votes <votes tested> bits <bits set>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "evidence.hip.h"

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
    int32_t hd[12];
    double thr;
    if (std::fread(hd, 4, 12, f) != 12 || std::fread(&thr, 8, 1, f) != 1) return 2;
    const int model = hd[0], k = hd[1], cell = hd[2], aw = hd[3], ah = hd[4], min_inliers = hd[5], n = hd[6], ntrain = hd[7];
    const size_t qtot = (size_t)hd[8];
    const uint32_t flags_word = (uint32_t)hd[9], rerun_mask = (uint32_t)hd[10];
    if (!evidence_cell_ok(cell) || n < 0 || k < 1 || aw < 1 || ah < 1) return 2;
    static_assert(sizeof(slideo_keypoint) == 24 && sizeof(slideo_verdict) == 16 && sizeof(EvVote) == 8 && sizeof(EvXY) == 8, "record sizes");
    auto qofs = read_exact<uint32_t>(f, (size_t)n + 1);
    auto verdicts = read_exact<slideo_verdict>(f, (size_t)n);
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
            int32_t rec[3];
            if (std::fread(rec, 4, 3, f) != 3 || std::fread(fcs[i].M[j], 8, 9, f) != 9) return 2;
            fcs[i].page[j] = rec[0]; fcs[i].count[j] = rec[1]; fcs[i].ofs[j] = rec[2];
        }
    }
    std::fclose(f);

    const int gw = (aw + cell - 1) / cell, gh = (ah + cell - 1) / cell;
    const size_t nc = (size_t)gw * gh;
    std::unique_ptr<uint32_t[]> seen(new uint32_t[nc]()), hit(new uint32_t[nc]());
    std::unique_ptr<uint32_t[]> flags(new uint32_t[1]{flags_word});
    std::unique_ptr<uint32_t[]> bits(new uint32_t[EV_WORDS]);

    EvidenceArgs a{};
    a.verdicts = verdicts.get(); a.fcs = fcs.get(); a.qofs = qofs.get(); a.kp = kp.get(); a.page_xy = page_xy.get(); a.votes = votes.get();
    a.flags = flags.get(); a.rerun_mask = rerun_mask;
    a.k = k; a.model = model; a.min_inliers = min_inliers; a.thr2 = thr * thr;
    a.aw = aw; a.ah = ah; a.cell = cell; a.gw = gw; a.gh = gh;
    a.seen = seen.get(); a.hit = hit.get();

    long most_windows = 0, tested = 0, set = 0;
    for (int fr = 0; fr < n; ++fr) {                                   // one block per frame
        const EvidenceFrame e = evidence_frame(a, fr);
        if (e.n == 0) continue;
        long windows = 0;
        for (uint32_t base = 0; base < e.n; base += EV_BITS) {
            ++windows;
            std::memset(bits.get(), 0, sizeof(uint32_t) * EV_WORDS);
            for (int tid = 0; tid < EV_THREADS; ++tid)
                evidence_votes(a, e, base, tid, EV_THREADS, bits.get(), [&](uint32_t* p, uint32_t v) { *p |= v; });
            for (int w = 0; w < EV_WORDS; ++w) set += __builtin_popcount(bits[w]);
            for (int tid = 0; tid < EV_THREADS; ++tid)
                evidence_count(a, e, base, tid, EV_THREADS, bits.get(), [](uint32_t* p) { *p += 1u; });
        }
        tested += e.count;
        most_windows = windows > most_windows ? windows : most_windows;
    }
    FILE* fo = std::fopen(argv[2], "wb");
    if (!fo) return 2;
    std::fwrite(seen.get(), 4, nc, fo);
    std::fwrite(hit.get(), 4, nc, fo);
    std::fclose(fo);
    std::printf("windows %ld votes %ld bits %ld\n", most_windows, tested, set);
    return 0;
}
