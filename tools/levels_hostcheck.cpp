// levels_hostcheck — the per-thread bodies of csrc/levels.hip.h (levels_thread, levels_hist_thread, compiled for the host) run lane
// by lane over their launch grids, and the plain rules of csrc/frame_settings.h (the stretch table, the points), for
// tests/test_levels_abi.py, which compares with tests/levels_ref.py.  The LDS adds and the global atomics are plain sums here; a
// block's bins are a u32 [768] array of its own, flushed into the u64 histogram as the kernel flushes them.
//   g++ -O1 -g -std=c++17 [-fsanitize=address,undefined] -I include -I slideo_amd/csrc tools/levels_hostcheck.cpp -o hostcheck
//   hostcheck apply <case> <out>    <case>: int32 {w, h, n, src_stride, dst_stride, src_offset, dst_offset, in_place}, the table (768
//                                   bytes), n frames of h * src_stride bytes.  <out>: the destination buffer — in place the source
//                                   buffer itself (dst_stride and dst_offset unused).  Prints the paths taken and whether an
//                                   out-of-place source is unchanged.
//   hostcheck hist <case> <out>     <case>: int32 {aw, ah, n, stride, src_offset, split[4]} — the n frames are observed in launches
//                                   of split[0], split[1], ... frames (zeros end the list; what is left goes into a last launch) —,
//                                   n frames of ah * stride bytes.  <out>: u64 [3][256].
//   hostcheck lut lo0 lo1 lo2 hi0 hi1 hi2 <out>     the stretch table (768 bytes), or "1 <message>" for a refusal
//   hostcheck lutsweep <out>        every (lo, hi) with 0 <= lo < hi <= 255, in order of lo then hi: channel 0's 256 bytes each
//   hostcheck points low_ppm high_ppm <hist: 768 u64>   "lo0 lo1 lo2 hi0 hi1 hi2", or "<code> <message>"
// Every image buffer is a heap allocation of its exact size — it ends with the last pixel of the last row of the last frame, and
// begins `offset` bytes past a 16-byte boundary — so that a sanitized build sees any access outside it or at a misaligned address.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "slideo_amd.h"
#include "frame_settings.h"
#include "levels.hip.h"

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
    if (!read_file(cin, file) || file.size() < 32 + 768) return 2;
    int32_t hd[8];
    std::memcpy(hd, file.data(), 32);
    const int w = hd[0], h = hd[1], n = hd[2], ss = hd[3], ds = hd[4], sofs = hd[5] & 15, dofs = hd[6] & 15, in_place = hd[7];
    if (w < 1 || h < 1 || n < 1 || ss < 3 * w || (!in_place && ds < 3 * w)) return 2;
    const uint8_t* lut = file.data() + 32;
    const size_t sfb = (size_t)h * ss, dfb = (size_t)h * ds;
    if (file.size() != 32 + 768 + sfb * n) return 2;
    const size_t stot = span(w, h, n, ss), dtot = in_place ? stot : span(w, h, n, ds);
    // exact-size blocks: malloc returns 16-byte aligned memory; the image begins `offset` bytes into it and ends at its last byte
    uint8_t* sraw = static_cast<uint8_t*>(std::malloc(sofs + stot));
    uint8_t* draw = in_place ? nullptr : static_cast<uint8_t*>(std::malloc(dofs + dtot));
    if (!sraw || (!in_place && !draw)) return 2;
    uint8_t* src = sraw + sofs;
    std::memcpy(src, file.data() + 32 + 768, stot);
    uint8_t* dst = in_place ? src : draw + dofs;
    if (!in_place) std::memset(dst, 0xAA, dtot);
    const LevelsArgs a = levels_args(lut, src, (int64_t)sfb, ss, dst, in_place ? (int64_t)sfb : (int64_t)dfb, in_place ? ss : ds, w, h, n);
    const int gx = ((w + 3) / 4 + LVL_TX - 1) / LVL_TX, gy = (h + LVL_TY - 1) / LVL_TY;
    for (int z = 0; z < n; ++z)
        for (int by = 0; by < gy; ++by)
            for (int bx = 0; bx < gx; ++bx)
                for (int ty = 0; ty < LVL_TY; ++ty)
                    for (int tx = 0; tx < LVL_TX; ++tx) levels_thread(a, lut, bx * LVL_TX + tx, by * LVL_TY + ty, z);
    const int unchanged = in_place ? -1 : std::memcmp(src, file.data() + 32 + 768, stot) == 0;
    if (!write_file(cout, dst, dtot)) return 2;
    std::printf("in4 %d out4 %d place %d src_unchanged %d\n", a.in4, a.out4, in_place ? 1 : 0, unchanged);
    std::free(sraw); std::free(draw);
    return 0;
}

static int run_hist(const char* cin, const char* cout) {
    std::vector<uint8_t> file;
    if (!read_file(cin, file) || file.size() < 36) return 2;
    int32_t hd[9];
    std::memcpy(hd, file.data(), 36);
    const int aw = hd[0], ah = hd[1], n = hd[2], stride = hd[3], ofs = hd[4] & 15;
    if (aw < 1 || ah < 1 || n < 1 || stride < 3 * aw) return 2;
    const size_t fb = (size_t)ah * stride, total = span(aw, ah, n, stride);
    if (file.size() != 36 + fb * n) return 2;
    uint8_t* raw = static_cast<uint8_t*>(std::malloc(ofs + total));
    if (!raw) return 2;
    uint8_t* src = raw + ofs;
    std::memcpy(src, file.data() + 36, total);
    std::vector<unsigned long long> hist(768, 0);
    const int gx = ((aw + 3) / 4 + LVL_TX - 1) / LVL_TX, gy = levels_hist_grid_y(ah);
    int in4 = 1, launches = 0, tiles = 0;
    for (int i = 0, k = 0; i < n; ++k) {
        int nb = k < 4 && hd[5 + k] > 0 ? hd[5 + k] : n - i;
        if (nb > n - i) nb = n - i;
        const LevelsHistArgs a = levels_hist_args(src + (size_t)i * fb, (int64_t)fb, stride, aw, ah, nb, hist.data());
        in4 &= a.in4; ++launches;
        for (int by = 0; by < gy; ++by)
            for (int bx = 0; bx < gx; ++bx) {
                uint32_t bins[768];
                std::memset(bins, 0, sizeof bins);
                int mine = 0;
                for (int ty = 0; ty < LVL_TY; ++ty)
                    for (int tx = 0; tx < LVL_TX; ++tx) {
                        int t = 0;
                        for (int y = by * LVL_TY + ty; y < ah; y += gy * LVL_TY, ++t) levels_hist_thread(a, bins, bx * LVL_TX + tx, y);
                        if (t > mine) mine = t;
                    }
                if (mine > tiles) tiles = mine;
                for (int b = 0; b < 768; ++b) if (bins[b]) hist[b] += bins[b];
            }
        i += nb;
    }
    if (!write_file(cout, hist.data(), 768 * 8)) return 2;
    std::printf("in4 %d launches %d grid_y %d tiles %d\n", in4, launches, gy, tiles);
    std::free(raw);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s apply|hist|lut|lutsweep|points ...\n", argv[0]); return 2; }
    const std::string mode = argv[1];
    try {
        if (mode == "apply" && argc == 4) return run_apply(argv[2], argv[3]);
        if (mode == "hist" && argc == 4) return run_hist(argv[2], argv[3]);
        if (mode == "lut" && argc == 9) {
            int32_t lo[3], hi[3];
            for (int c = 0; c < 3; ++c) { lo[c] = std::atoi(argv[2 + c]); hi[c] = std::atoi(argv[5 + c]); }
            uint8_t lut[768];
            frame_levels_lut(lo, hi, lut);
            if (!write_file(argv[8], lut, 768)) return 2;
            std::printf("0 ok identity %d\n", frame_levels_identity(lut) ? 1 : 0);
            return 0;
        }
        if (mode == "lutsweep" && argc == 3) {
            std::vector<uint8_t> out;
            uint8_t lut[768];
            for (int lo = 0; lo < 255; ++lo)
                for (int hi = lo + 1; hi <= 255; ++hi) {
                    const int32_t l[3] = {lo, 0, 0}, h[3] = {hi, 255, 255};
                    frame_levels_lut(l, h, lut);
                    out.insert(out.end(), lut, lut + 256);
                }
            if (!write_file(argv[2], out.data(), out.size())) return 2;
            std::printf("%zu\n", out.size() / 256);
            return 0;
        }
        if (mode == "points" && argc == 5) {
            std::vector<uint8_t> file;
            if (!read_file(argv[4], file) || file.size() != 768 * 8) return 2;
            uint64_t hist[768];
            std::memcpy(hist, file.data(), sizeof hist);
            int32_t lo[3], hi[3];
            levels_points(hist, std::atoi(argv[2]), std::atoi(argv[3]), lo, hi);
            std::printf("%d %d %d %d %d %d\n", lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]);
            return 0;
        }
    } catch (const Error& e) {
        std::printf("%d %s\n", e.code, e.what());
        return 0;
    }
    std::fprintf(stderr, "bad arguments\n");
    return 2;
}
