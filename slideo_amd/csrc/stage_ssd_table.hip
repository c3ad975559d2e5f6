// stage_ssd_table.hip — the SSD-table engine under the direct page look-up (stage_direct.hip) and the gate reference ANCHOR
// (stage_gate_anchor.hip): the centred operand, the table of dot products, and what the two taps share (kernels: ssd_table.hip.h).
#include "runtime.hpp"
#include "ssd_table.hip.h"

using namespace slideo;

namespace slideo {

int64_t ssd_kp(int64_t L) { return cdiv64(L, SSD_KGRAN) * SSD_KGRAN; }
int ssd_rows_pad(int rows) { return cdiv(rows, SSD_TILE) * SSD_TILE; }

void ssd_operand_build(const uint8_t* src, int64_t stride, const long long* ofs, int n, int rows_pad, int64_t L, int64_t kp, uint4* out,
                       long long* norm, hipStream_t st, const uint8_t* weights) {
    // 32-row tiles x K slices: about 2048 waves, a wave at least one group of four K steps; the norms are added to
    const int tiles = rows_pad / 32;
    const int ky = (int)std::max<int64_t>(1, std::min<int64_t>(cdiv64(512, tiles), cdiv64(kp / SSD_KGRAN, SSD_BLOCK / 64)));
    HIP_CHECK(hipMemsetAsync(norm, 0, (size_t)n * 8, st));
    const auto kernel = !weights ? direct_centre_kernel<false, true> : out ? direct_centre_kernel<true, true> : direct_centre_kernel<true, false>;
    kernel<<<dim3(tiles, ky), SSD_BLOCK, 0, st>>>(src, stride, ofs, n, L, kp, weights, out, reinterpret_cast<unsigned long long*>(norm));
    check_launch("direct_centre_kernel");
}

namespace {

// K chunks of the grid over n x np rows: enough blocks for every CU to hold a few waves, chunks of whole granules and at most
// SSD_KCHUNK_MAX
int64_t ssd_kchunk(int n, int np, int64_t kp) {
    const int64_t tiles = (int64_t)cdiv(n, SSD_TILE) * cdiv(np, SSD_TILE);
    const int64_t want = std::max<int64_t>(1, cdiv64(1024, tiles));    // waves wanted / tiles
    int64_t chunk = cdiv64(cdiv64(kp, want), SSD_KGRAN) * SSD_KGRAN;
    chunk = std::max<int64_t>(chunk, 8 * SSD_KGRAN);
    return std::min<int64_t>(chunk, SSD_KCHUNK_MAX);
}

}  // namespace

void ssd_table_dots(const uint4* a, int n, const uint4* b, int np, int64_t kp, unsigned long long* dot, hipStream_t st) {
    if (!b) np = n;
    HIP_CHECK(hipMemsetAsync(dot, 0, (size_t)n * np * 8, st));
    const int64_t kchunk = ssd_kchunk(n, np, kp);
    const int64_t nz = cdiv64(kp, kchunk);
    if (kchunk > SSD_KCHUNK_MAX || kchunk % SSD_KGRAN || nz > 65535) fail(SLIDEO_ERR_HIP, "internal: K chunk %lld of %lld", (long long)kchunk, (long long)kp);
    const dim3 grid(cdiv(n, 2 * SSD_TILE), cdiv(np, 2 * SSD_TILE), (unsigned)nz);
    if (b) {
        page_ssd_kernel<<<grid, SSD_BLOCK, 0, st>>>(a, n, b, np, kp, kchunk, dot);
        check_launch("page_ssd_kernel");
    } else {
        frame_gram_kernel<<<grid, SSD_BLOCK, 0, st>>>(a, n, kp, kchunk, dot);
        check_launch("frame_gram_kernel");
    }
}

const uint8_t* tap_valid_weights(const slideo_matcher* m, const char* tap, bool use_valid, int sw, int sh) {
    if (!use_valid) return nullptr;
    const GateMap& g = m->fs.gate_map;
    if (!g.on) fail(SLIDEO_ERR_STATE, "%s: no validity map is in force (a frame mask under SLIDEO_MASK_GATE)", tap);
    if (sw != g.sw || sh != g.sh) fail(SLIDEO_ERR_INVALID_ARG, "%s: %dx%d small images, the validity map is %dx%d", tap, sw, sh, g.sw, g.sh);
    return m->d_gate_w.as<uint8_t>();
}

}  // namespace slideo
