// stage_content.hip — the frame content box of include/slideo_amd.h "Frame content box": the content accumulator's entry points,
// the launch the observe driver (stage_activity.hip) calls on a staged block, and the read-out (kernels: content.hip.h).
#include "runtime.hpp"
#include "content.hip.h"

#include <vector>

using namespace slideo;

namespace slideo {

void content_launch(slideo_matcher* m, const DevFrames& f, int n, hipStream_t st) {
    const slideo_matcher::Content& K = m->content;
    const ContentArgs a = content_args(f.p, f.frame_stride, f.stride, f.w, f.h, n, K.level, m->d_cnt_lit.as<uint32_t>());
    const dim3 grid((unsigned)cdiv64((f.w + 3) / 4, CNT_TX), (unsigned)cdiv64(f.h, CNT_TY));
    content_kernel<<<grid, dim3(CNT_TX, CNT_TY), 0, st>>>(a);
    check_launch("content_kernel");
}

}  // namespace slideo

extern "C" {

int32_t slideo_matcher_content_begin(slideo_matcher* m, int32_t level) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (level < 0 || level > CNT_MAX_LEVEL) fail(SLIDEO_ERR_INVALID_ARG, "content_begin: level %d outside 0..%d", level, CNT_MAX_LEVEL);
    require_idle(m);
    m->content = slideo_matcher::Content{};
    m->content.on = true; m->content.level = level;
    API_CATCH(m)
}

int32_t slideo_matcher_content_end(slideo_matcher* m) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    require_idle(m);
    HIP_CHECK(hipSetDevice(m->device));
    m->content = slideo_matcher::Content{};
    m->d_cnt_lit.release(); m->d_cnt_fill.release();
    if (!m->activity.on && !m->levels.on) m->d_act_stage.release();      // (shared by the sessions: released when the last of them ends)
    API_CATCH(m)
}

int32_t slideo_matcher_content_info(slideo_matcher* m, int32_t* aw, int32_t* ah, int32_t* frames, int32_t* level) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (!aw || !ah || !frames || !level) fail(SLIDEO_ERR_INVALID_ARG, "null aw/ah/frames/level");
    const slideo_matcher::Content& K = m->content;
    if (!K.on) fail(SLIDEO_ERR_STATE, "no content accumulator: slideo_matcher_content_begin first");
    *aw = K.aw; *ah = K.ah; *frames = (int32_t)K.frames; *level = K.level;
    API_CATCH(m)
}

int32_t slideo_matcher_content_counts(slideo_matcher* m, uint32_t* out, int64_t capacity_elems, int32_t* aw, int32_t* ah, int32_t* frames) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (!aw || !ah || !frames) fail(SLIDEO_ERR_INVALID_ARG, "null aw/ah/frames");
    require_idle(m);
    const slideo_matcher::Content& K = m->content;
    if (!K.on || K.aw == 0) fail(SLIDEO_ERR_STATE, "the content accumulator has observed no frame");
    *aw = K.aw; *ah = K.ah; *frames = (int32_t)K.frames;
    if (!out) return SLIDEO_OK;
    const int64_t px = (int64_t)K.aw * K.ah;
    if (px > capacity_elems) fail(SLIDEO_ERR_CAPACITY, "the counts need %lld elements", (long long)px);
    HIP_CHECK(hipSetDevice(m->device));
    HIP_CHECK(hipMemcpyAsync(out, m->d_cnt_lit.p, (size_t)px * 4, hipMemcpyDeviceToHost, m->stream));
    HIP_CHECK(hipStreamSynchronize(m->stream));
    API_CATCH(m)
}

int32_t slideo_matcher_content_box(slideo_matcher* m, int32_t min_share_ppm, int32_t min_fill_ppm, int32_t* box, int64_t* n_content,
                                   uint32_t* fill_out, int64_t fill_capacity_elems) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (!box || !n_content) fail(SLIDEO_ERR_INVALID_ARG, "null box/n_content");
    if (min_share_ppm < 0 || min_share_ppm > CNT_MAX_PPM) fail(SLIDEO_ERR_INVALID_ARG, "content_box: min_share_ppm %d outside 0..%d", min_share_ppm, CNT_MAX_PPM);
    if (min_fill_ppm < 0 || min_fill_ppm > CNT_MAX_PPM) fail(SLIDEO_ERR_INVALID_ARG, "content_box: min_fill_ppm %d outside 0..%d", min_fill_ppm, CNT_MAX_PPM);
    require_idle(m);
    const slideo_matcher::Content& K = m->content;
    if (!K.on || K.frames == 0) fail(SLIDEO_ERR_STATE, "the content accumulator has observed no frame");
    const int aw = K.aw, ah = K.ah;
    const size_t nfill = (size_t)ah + aw;
    if (fill_out && (int64_t)nfill > fill_capacity_elems) fail(SLIDEO_ERR_CAPACITY, "the fills need %lld elements", (long long)nfill);
    HIP_CHECK(hipSetDevice(m->device));
    hipStream_t st = m->stream;
    // {n_content (u64) | row fills | column fills}
    m->d_cnt_fill.reserve(8 + nfill * 4);
    ContentFillArgs a{};
    a.lit = m->d_cnt_lit.as<uint32_t>();
    a.aw = aw; a.ah = ah;
    a.ppm = (uint64_t)min_share_ppm; a.frames = (uint64_t)K.frames;
    a.n_content = m->d_cnt_fill.as<unsigned long long>();
    a.row_fill = m->d_cnt_fill.as<uint32_t>() + 2; a.col_fill = a.row_fill + ah;
    HIP_CHECK(hipMemsetAsync(m->d_cnt_fill.p, 0, 8 + nfill * 4, st));
    const dim3 grid((unsigned)cdiv64(aw, CNT_FILL_TX), (unsigned)cdiv64(ah, CNT_FILL_ROWS));
    content_fill_kernel<<<grid, dim3(CNT_FILL_TX), 0, st>>>(a);
    check_launch("content_fill_kernel");
    std::vector<uint32_t> got(2 + nfill);
    HIP_CHECK(hipMemcpyAsync(got.data(), m->d_cnt_fill.p, 8 + nfill * 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    const uint64_t total = (uint64_t)got[0] | ((uint64_t)got[1] << 32);
    const uint32_t* rows = got.data() + 2;
    const uint32_t* cols = rows + ah;
    uint64_t rsum = 0, csum = 0;
    for (int y = 0; y < ah; ++y) rsum += rows[y];
    for (int x = 0; x < aw; ++x) csum += cols[x];
    if (rsum != total || csum != total || total > (uint64_t)aw * ah)
        fail(SLIDEO_ERR_HIP, "internal: %llu content pixels, %llu in the rows, %llu in the columns", (unsigned long long)total,
             (unsigned long long)rsum, (unsigned long long)csum);
    // the first and the last content row and column, from the fills (include/slideo_amd.h: strict, in u64)
    int x0 = -1, x1 = 0, y0 = -1, y1 = 0;
    for (int y = 0; y < ah; ++y)
        if ((uint64_t)rows[y] * 1000000ull > (uint64_t)min_fill_ppm * (uint64_t)aw) { if (y0 < 0) y0 = y; y1 = y + 1; }
    for (int x = 0; x < aw; ++x)
        if ((uint64_t)cols[x] * 1000000ull > (uint64_t)min_fill_ppm * (uint64_t)ah) { if (x0 < 0) x0 = x; x1 = x + 1; }
    if (x0 < 0 || y0 < 0) x0 = y0 = x1 = y1 = 0;
    box[0] = x0; box[1] = y0; box[2] = x1; box[3] = y1;
    *n_content = (int64_t)total;
    if (fill_out) std::copy(rows, rows + nfill, fill_out);
    API_CATCH(m)
}

}  // extern "C"
