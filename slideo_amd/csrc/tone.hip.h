// tone.hip.h — the match tone table (include/slideo_amd.h "Match tone table"): per channel, what page tone a frame tone stands for,
// counted over the pixels of the contributing candidate's small image that the matched hits enclose.
//
//   tone_kernel   grid: the unit's frames, block TONE_THREADS; launched by unit_verify behind verdict_kernel (and evidence_kernel) on
//                 the unit's stream, only while a session is open.  Per frame:
//                   the contributor   the candidate slot with a model and the most inliers (tone_frame; block-uniform);
//                   phase 1           its run of votes tested in f64 (evidence_passes, by inclusion); a thread keeps its hits' count
//                                     and integer box in registers and merges them into five LDS words ONCE, at its end (add, min,
//                                     max; results unused);
//                   phase 2           work items of TONE_SEG consecutive pixels of one small-image row.  A thread maps each pixel's
//                                     centre through M in f64, gathers the frame's 3 bytes, and keeps per channel the bin, a run
//                                     length and a run sum: the LDS adds (u32 [2][3][256], results unused) are issued only when the
//                                     bin changes and at the item's end.  On a slide almost every sample of an item falls into one
//                                     bin: 6 adds per item, not 6 per pixel, so the same-address serialisation of a white page
//                                     costs one add per item and channel;
//                   flush             the block's NONZERO bins go to the global u64 arrays with 64-bit atomics whose result is not
//                                     read; one thread adds 1 to frames_counted.
//                 The small image is walked in row tiles of at most TONE_TILE_PX pixels, flushed one by one: a block's u32 sum bin
//                 holds at most 255 * TONE_TILE_PX (static_assert below).  A usual small image (about 120 000 pixels) is one tile.
//                 Integer adds commute: the units in flight share the accumulators and no order enters.  The unit's flags word is
//                 read first (evidence_kernel's rule): a unit that is run again leaves without counting.
// The per-frame body is host + device functions which a thread of the block (or, on the host, every thread index in turn:
// tools/tone_hostcheck.cpp) calls with its index; the kernel puts its barriers between them.
// tone_lut: the pure host function of the header, integers only.
#pragma once
#include <stdint.h>

#include "evidence.hip.h"

namespace slideo {

constexpr int TONE_THREADS = 256;
constexpr int TONE_SEG = 32;                         // consecutive pixels of a row per work item
constexpr int TONE_TILE_PX = 1 << 22;                // pixels of a row tile at most: a block's u32 bins are flushed after each
constexpr int TONE_BINS = 2 * 3 * 256;               // {cnt [3][256] | sum [3][256]}
constexpr int64_t TONE_MAX_FRAMES = (int64_t)1 << 31;   // frames through a session
constexpr int TONE_BOX_LIM = 1 << 30;                // a hit's box coordinates are clamped here (pages are at most MAX_DIM wide: no effect)
static_assert((uint64_t)255 * TONE_TILE_PX < ((uint64_t)1 << 32) && TONE_TILE_PX < (1 << 24), "a block's sum bins are u32");

struct ToneArgs {
    EvidenceArgs ev;                     // fcs, qofs, kp, page_xy, votes, flags, rerun_mask, k, model, thr2 (the others unused)
    const PageInfo* pageinfo;
    const uint8_t* page_small;           // the pages' small images, a page's at pageinfo[p].small_ofs
    const uint8_t* frames;               // the unit's analysed images, BGR8
    int64_t frame_stride;
    int32_t stride, aw, ah;
    int32_t min_inliers, min_hits, flat;
    unsigned long long* acc;             // {cnt [3][256] | sum [3][256] | frames_counted}
};

// the contributor of a frame: its page, transform and run of votes.  slot < 0: none
struct ToneFrame {
    int32_t slot, page, count;
    uint32_t q0, n;
    const double* M;
    const EvVote* votes;
};

// a thread's (then the block's) hits: their number and the box of their page points, {floor min x, floor min y, ceil max x, ceil max y}
struct ToneBox { int32_t hits, x0, y0, x1, y1; };
EV_HD ToneBox tone_box_empty() { return ToneBox{0, TONE_BOX_LIM, TONE_BOX_LIM, -TONE_BOX_LIM, -TONE_BOX_LIM}; }

// whether slot j holds a model: its transform, as slideo_last_frame_candidates returns it, is not all zero
EV_HD bool tone_slot_found(const FrameCands& fc, int j, int model) {
    const int nm = model == 1 ? 9 : 6;
    bool any = model != 1 && fc.found[j] != 0;
    for (int i = 0; i < nm; ++i) any |= fc.M[j][i] != 0.0;
    return any;
}

EV_HD ToneFrame tone_frame(const ToneArgs& a, int f) {
    ToneFrame e{};
    e.slot = -1;
    if (a.ev.flags && (a.ev.flags[0] & a.ev.rerun_mask)) return e;
    const FrameCands& fc = a.ev.fcs[f];
    const int nc = fc.ncand < MAXC ? fc.ncand : MAXC;
    int best = -1;
    for (int j = 0; j < nc; ++j) {
        if (fc.inliers[j] < a.min_inliers || !tone_slot_found(fc, j, a.ev.model)) continue;
        if (best < 0 || fc.inliers[j] > fc.inliers[best]) best = j;
    }
    if (best < 0) return e;
    e.slot = best; e.page = fc.page[best]; e.count = fc.count[best];
    e.q0 = a.ev.qofs[f]; e.n = a.ev.qofs[f + 1] - e.q0;
    e.M = fc.M[best];
    e.votes = a.ev.votes + (size_t)e.q0 * a.ev.k + fc.ofs[best];
    return e;
}

EV_HD int32_t tone_clamp(double v) {
    return v < -(double)TONE_BOX_LIM ? -TONE_BOX_LIM : v > (double)TONE_BOX_LIM ? TONE_BOX_LIM : (int32_t)v;
}

// phase 1: thread tid of nt tests its share of the contributor's votes -> its hits and their box
EV_HD ToneBox tone_votes(const ToneArgs& a, const ToneFrame& e, int tid, int nt) {
    ToneBox b = tone_box_empty();
    for (int i = tid; i < e.count; i += nt) {
        const EvVote v = e.votes[i];
        if (v.x >= e.n) continue;
        const slideo_keypoint q = a.ev.kp[e.q0 + v.x];
        const EvXY p = a.ev.page_xy[v.y];
        if (!evidence_passes(a.ev, e.M, p.x, p.y, q.x, q.y)) continue;
        const int32_t fx = tone_clamp(__builtin_floor((double)p.x)), fy = tone_clamp(__builtin_floor((double)p.y));
        const int32_t cx = tone_clamp(__builtin_ceil((double)p.x)), cy = tone_clamp(__builtin_ceil((double)p.y));
        ++b.hits;
        b.x0 = fx < b.x0 ? fx : b.x0; b.y0 = fy < b.y0 ? fy : b.y0;
        b.x1 = cx > b.x1 ? cx : b.x1; b.y1 = cy > b.y1 ? cy : b.y1;
    }
    return b;
}

// the page coordinate of small pixel i's centre along an axis of `full` page pixels and `small` small pixels
EV_HD double tone_centre(int i, int full, int small) { return (((double)i + 0.5) * (double)full) / (double)small - 0.5; }

// whether the four edge-clamped neighbours of small pixel (i, j) differ from it by at most `flat` in every channel
EV_HD bool tone_flat(const uint8_t* small, int sw, int sh, int i, int j, int flat) {
    if (flat >= 255) return true;
    const uint8_t* c = small + ((size_t)j * sw + i) * 3;
    const int il = i > 0 ? i - 1 : 0, ir = i + 1 < sw ? i + 1 : sw - 1, ju = j > 0 ? j - 1 : 0, jd = j + 1 < sh ? j + 1 : sh - 1;
    const uint8_t* nb[4] = {small + ((size_t)j * sw + il) * 3, small + ((size_t)j * sw + ir) * 3, small + ((size_t)ju * sw + i) * 3,
                            small + ((size_t)jd * sw + i) * 3};
    bool ok = true;
    for (int k = 0; k < 4; ++k)
        for (int ch = 0; ch < 3; ++ch) {
            const int d = (int)nb[k][ch] - (int)c[ch];
            ok &= (d < 0 ? -d : d) <= flat;
        }
    return ok;
}

// phase 2 of the row tile [j0, j1): thread tid of nt walks its work items; bins: TONE_BINS words, zero before the tile
template <class Add>
EV_HD void tone_samples(const ToneArgs& a, const ToneFrame& e, const ToneBox& box, int f, int j0, int j1, int tid, int nt, uint32_t* bins,
                        Add&& add) {
    const PageInfo pi = a.pageinfo[e.page];
    const uint8_t* small = a.page_small + pi.small_ofs;
    const uint8_t* frame = a.frames + (int64_t)f * a.frame_stride;
    const int sw = pi.sw, sh = pi.sh;
    const int nseg = (sw + TONE_SEG - 1) / TONE_SEG;
    const int items = (j1 - j0) * nseg;                    // (at most TONE_TILE_PX / sw rows of ceil(sw / TONE_SEG) items: an int)
    const double* M = e.M;
    for (int it = tid; it < items; it += nt) {
        const int j = j0 + it / nseg, i0 = (it % nseg) * TONE_SEG;
        const double y = tone_centre(j, pi.h, sh);
        if (!((double)box.y0 <= y && y <= (double)box.y1)) continue;
        const int i1 = i0 + TONE_SEG < sw ? i0 + TONE_SEG : sw;
        uint32_t bin[3] = {0, 0, 0}, run[3] = {0, 0, 0}, rsum[3] = {0, 0, 0};
        for (int i = i0; i < i1; ++i) {
            const double x = tone_centre(i, pi.w, sw);
            if (!((double)box.x0 <= x && x <= (double)box.x1)) continue;
            double X = M[0] * x + M[1] * y + M[2], Y = M[3] * x + M[4] * y + M[5];
            if (a.ev.model == 1) {
                const double w = M[6] * x + M[7] * y + M[8];
                if (w == 0.0) continue;
                X /= w; Y /= w;
            }
            const double Xr = __builtin_floor(X + 0.5), Yr = __builtin_floor(Y + 0.5);
            if (!(Xr >= 0.0 && Xr < (double)a.aw && Yr >= 0.0 && Yr < (double)a.ah)) continue;      // (a NaN fails here)
            if (!tone_flat(small, sw, sh, i, j, a.flat)) continue;
            const uint8_t* fp = frame + (int64_t)(int)Yr * a.stride + (int64_t)(int)Xr * 3;
            const uint8_t* pp = small + ((size_t)j * sw + i) * 3;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (int ch = 0; ch < 3; ++ch) {
                const uint32_t fv = fp[ch], pv = pp[ch];
                if (run[ch] && fv != bin[ch]) {
                    add(bins + ch * 256 + bin[ch], run[ch]);
                    add(bins + 768 + ch * 256 + bin[ch], rsum[ch]);
                    run[ch] = 0; rsum[ch] = 0;
                }
                bin[ch] = fv; ++run[ch]; rsum[ch] += pv;
            }
        }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int ch = 0; ch < 3; ++ch)
            if (run[ch]) { add(bins + ch * 256 + bin[ch], run[ch]); add(bins + 768 + ch * 256 + bin[ch], rsum[ch]); }
    }
}

// the tile's nonzero bins to the accumulators: thread tid of nt
template <class Add64>
EV_HD void tone_flush(const ToneArgs& a, int tid, int nt, const uint32_t* bins, Add64&& add64) {
    for (int b = tid; b < TONE_BINS; b += nt) {
        const uint32_t v = bins[b];
        if (v) add64(a.acc + b, (unsigned long long)v);
    }
}

// rows of a tile of a small image sw wide (sw <= TONE_TILE_PX)
EV_HD int tone_tile_rows(int sw) { const int r = TONE_TILE_PX / (sw > 0 ? sw : 1); return r > 0 ? r : 1; }

#if defined(__HIPCC__)
__global__ __launch_bounds__(TONE_THREADS) void tone_kernel(ToneArgs a) {
    __shared__ uint32_t bins[TONE_BINS];
    __shared__ int32_t s_box[5];
    const int f = blockIdx.x, tid = threadIdx.x;
    const ToneFrame e = tone_frame(a, f);                  // (block-uniform: every thread reads the same words)
    if (e.slot < 0) return;
    if (tid == 0) { const ToneBox z = tone_box_empty(); s_box[0] = 0; s_box[1] = z.x0; s_box[2] = z.y0; s_box[3] = z.x1; s_box[4] = z.y1; }
    __syncthreads();
    const ToneBox mine = tone_votes(a, e, tid, TONE_THREADS);
    if (mine.hits) {                                       // (results unused: LDS atomics without a return value, once per thread)
        atomicAdd(&s_box[0], mine.hits);
        atomicMin(&s_box[1], mine.x0); atomicMin(&s_box[2], mine.y0);
        atomicMax(&s_box[3], mine.x1); atomicMax(&s_box[4], mine.y1);
    }
    __syncthreads();
    const ToneBox box{s_box[0], s_box[1], s_box[2], s_box[3], s_box[4]};
    if (box.hits < a.min_hits) return;                     // (block-uniform)
    const PageInfo pi = a.pageinfo[e.page];
    const int rows = tone_tile_rows(pi.sw);
    for (int j0 = 0; j0 < pi.sh; j0 += rows) {
        for (int b = tid; b < TONE_BINS; b += TONE_THREADS) bins[b] = 0;
        __syncthreads();
        tone_samples(a, e, box, f, j0, j0 + rows < pi.sh ? j0 + rows : pi.sh, tid, TONE_THREADS, bins,
                     [](uint32_t* p, uint32_t v) { atomicAdd(p, v); });
        __syncthreads();
        tone_flush(a, tid, TONE_THREADS, bins, [](unsigned long long* p, unsigned long long v) { atomicAdd(p, v); });
        __syncthreads();
    }
    if (tid == 0) atomicAdd(a.acc + TONE_BINS, 1ull);
}
#endif

// ---- the pure host function ----------------------------------------------------------------------------------------------------
// lut_out [3][256] from cnt, sum [3][256]; false: a channel without an anchor (nothing is written)
inline bool tone_lut(const uint64_t* cnt, const uint64_t* sum, uint64_t min_count, uint8_t* lut_out) {
    uint8_t out[768];
    for (int c = 0; c < 3; ++c) {
        const uint64_t* n = cnt + c * 256;
        const uint64_t* s = sum + c * 256;
        int anchor[256], na = 0;
        uint64_t m[256];
        uint64_t top = 0;
        for (int v = 0; v < 256; ++v) {
            if (n[v] < min_count) continue;
            const uint64_t mean = (2 * s[v] + n[v]) / (2 * n[v]);
            top = mean > top ? mean : top;
            anchor[na++] = v; m[v] = top;
        }
        if (na == 0) return false;
        uint8_t* o = out + c * 256;
        for (int x = 0; x <= anchor[0]; ++x) o[x] = (uint8_t)m[anchor[0]];
        for (int k = 0; k + 1 < na; ++k) {
            const uint64_t p = (uint64_t)anchor[k], q = (uint64_t)anchor[k + 1];
            for (uint64_t x = p + 1; x < q; ++x) o[x] = (uint8_t)((2 * (m[p] * (q - x) + m[q] * (x - p)) + (q - p)) / (2 * (q - p)));
            o[q] = (uint8_t)m[q];
        }
        for (int x = anchor[na - 1]; x < 256; ++x) o[x] = (uint8_t)m[anchor[na - 1]];
    }
    for (int i = 0; i < 768; ++i) lut_out[i] = out[i];
    return true;
}

}  // namespace slideo
