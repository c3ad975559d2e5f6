// stage_orb.hip — drivers of the ORB stage (kernels: orb.hip.h) and of the front doors in front of it: YUV frames (one argument
// record and one dispatch over the kernel families of yuv420.hip.h, yuv_sampling.hip.h, yuv_chroma.hip.h, yuv_transfer.hip.h), frames of
// another pixel format (pixel_format.hip.h), the frame levels' table (levels.hip.h), the working-size reduce (reduce.hip.h) and the
// frame region's rectify (frame_region.hip.h) with the frame lens fused into it (frame_lens.hip.h); the frame mask's pyramid and
// candidate filter (frame_mask.hip.h); the gather of a device frame list's planes (frame_list.hip.h).
#include <type_traits>

#include "runtime.hpp"
#include "orb.hip.h"
#include "yuv420.hip.h"
#include "yuv_sampling.hip.h"
#include "yuv_chroma.hip.h"
#include "yuv_transfer.hip.h"
#include "pixel_format.hip.h"
#include "frame_list.hip.h"
#define LEVELS_APPLY_KERNEL      // (levels_hist_kernel is stage_activity.hip's)
#include "levels.hip.h"
#define SHADING_APPLY_KERNEL
#include "shading.hip.h"
#include "reduce.hip.h"
#include "frame_region.hip.h"
#include "frame_lens.hip.h"
#include "frame_mask.hip.h"

using namespace slideo;

namespace slideo {

static GrayCoef gray_coef(const slideo_matcher* m) {
    return m->cfg.ocv.gray == 1 ? GrayCoef{1868u, 9617u, 4899u, 14u} : GrayCoef{3735u, 19235u, 9798u, 15u};
}

// device tables of the ORB kernels (umax, Gaussian taps, BRIEF pattern, intensity-centroid weights) and their launch attributes
void orb_stage_init(slideo_matcher* m) {
    const slideo_config* cfg = &m->cfg;
    OrbTables t{};
    umax_table(cfg->patch_size / 2, t.umax);
    if (cfg->ocv.blur == 2) gauss7_q8_rounded(t.gk); else gauss7_fixed(t.gk);
    gauss7_f32(t.gkf);
    brief_pattern(cfg->patch_size, t.pattern, cfg->ocv.rng_mul);
    m->d_tables.reserve(sizeof(OrbTables));
    HIP_CHECK(hipMemcpy(m->d_tables.p, &t, sizeof(t), hipMemcpyHostToDevice));
    std::vector<uint32_t> ict;
    ic_weight_table(cfg->patch_size / 2, t.umax, ict, m->ic_shift);
    m->ic_entries = (int)(ict.size() / 2);
    m->d_ictab.reserve(ict.size() * 4);
    HIP_CHECK(hipMemcpy(m->d_ictab.p, ict.data(), ict.size() * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&describe_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  describe_window(cfg->patch_size / 2).dwords * 16));
}

// per frame size: the resize tap table and the FAST tile table
void orb_geom_init(slideo_matcher* m, GeomEntry& e, const std::vector<uint32_t>& lin_tab) {
    std::vector<uint32_t> tab = lin_tab;
    if (tab.empty()) tab.push_back(0);
    e.lin_tab.reserve(tab.size() * 4);
    HIP_CHECK(hipMemcpyAsync(e.lin_tab.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, m->stream));
    std::vector<int4> ft((size_t)std::max(e.g.fast_tiles, 1));
    for (int t = 0; t < e.g.fast_tiles; ++t) ft[t] = fast_tile_entry(e.g, t);
    e.fast_tiles.reserve(ft.size() * sizeof(int4));
    HIP_CHECK(hipMemcpyAsync(e.fast_tiles.p, ft.data(), ft.size() * sizeof(int4), hipMemcpyHostToDevice, m->stream));
    HIP_CHECK(hipStreamSynchronize(m->stream));              // the host vectors die here
}

void orb_launch_gray(const slideo_matcher* m, const uint8_t* frames_dev, int64_t frame_stride, int stride, uint8_t* gray, int64_t gframe, int w, int h,
                     int pitch, int n, hipStream_t st) {
    const int aligned4 = ((uintptr_t)frames_dev % 4 == 0) && (stride % 4 == 0) && (frame_stride % 4 == 0);
    gray_kernel<<<dim3(cdiv(cdiv(w, 4), 256), h, n), 256, 0, st>>>(frames_dev, frame_stride, stride, gray, gframe, w, h, pitch, aligned4, gray_coef(m));
    check_launch("gray_kernel");
}

// ---- the YUV door: one argument record (yuv420.hip.h YuvArgs, filled by yuv_args and each family's two lines on it), one dispatch -------
static YuvCoef yuv_coef(const YuvDesc& desc) {
    int32_t c[7];
    yuv_coefficients(desc.matrix, desc.range, c);
    return YuvCoef{c[0], c[1], c[2], c[3], c[4], c[5]};
}

// the runtime depth, and (sampling, depth), as template constants: f(integral_constant<int, YUV_D*>) and f(integral_constant<int,
// YUV_S*>, integral_constant<int, YUV_D*>).  A family launches the instances it has; for a pair it has none for, which the rules in
// front of it never let through, it calls yuv_no_kernel
template <class F>
static void yuv_dispatch_depth(int depth, F&& f) {
    if (depth == SLIDEO_YUV_DEPTH_8) f(std::integral_constant<int, YUV_D8>{});
    else if (depth == SLIDEO_YUV_DEPTH_10_MSB) f(std::integral_constant<int, YUV_D10_MSB>{});
    else f(std::integral_constant<int, YUV_D10_LSB>{});
}
template <class F>
static void yuv_dispatch(int sampling, int depth, F&& f) {
    auto at_depth = [&](auto s) { yuv_dispatch_depth(depth, [&](auto d) { f(s, d); }); };
    if (sampling == SLIDEO_YUV_SAMPLING_422_PACKED) {
        if (depth != SLIDEO_YUV_DEPTH_8) fail(SLIDEO_ERR_UNSUPPORTED, "internal: packed 4:2:2 under a 10-bit depth");
        f(std::integral_constant<int, YUV_S422P>{}, std::integral_constant<int, YUV_D8>{});
    } else if (sampling == SLIDEO_YUV_SAMPLING_420) at_depth(std::integral_constant<int, YUV_S420>{});
    else if (sampling == SLIDEO_YUV_SAMPLING_422) at_depth(std::integral_constant<int, YUV_S422>{});
    else at_depth(std::integral_constant<int, YUV_S444>{});
}

[[noreturn]] static void yuv_no_kernel(const char* family, int sampling, int depth) {
    fail(SLIDEO_ERR_HIP, "internal: no %s kernel for sampling %d under depth %d", family, sampling, depth);
}

// n decoded YUV frames (validated layout, frame stride src_fs) -> BGR8 at dst (stride 3w, frame stride 3wh).  One kernel family per
// call, in this order: a transfer other than SDR (10-bit frames; tab: the matcher's device copy of LIN and OUT; the description's
// matrix is not consulted), a chroma filter other than NEAREST where the sampling has chroma to interpolate, a sampling other than
// 4:2:0, else the 4:2:0 description kernel — the default description (BT.601, limited, 8) included, whose coefficients are
// cvtColor(COLOR_YUV2BGR_*)'s.  A thread owns four columns of one row, or of the two luma rows of a chroma row (rows2)
void launch_yuv420_to_bgr(const YuvDesc& desc, const uint8_t* src, int64_t src_fs, const slideo_yuv420_layout& L, int w, int h, int n, uint8_t* dst,
                          hipStream_t st, const uint32_t* transfer_tab) {
    const int s = desc.sampling, d = desc.depth;
    const bool rows2 = s == SLIDEO_YUV_SAMPLING_420;
    const dim3 block(YUV_TX, YUV_TY);
    if (desc.transfer != SLIDEO_YUV_TRANSFER_SDR) {
        const uint4* tab = reinterpret_cast<const uint4*>(transfer_tab);
        if (!tab || d == SLIDEO_YUV_DEPTH_8 || s == SLIDEO_YUV_SAMPLING_422_PACKED || desc.filtered())
            fail(SLIDEO_ERR_HIP, "internal: no transfer kernel for transfer %d under depth %d, sampling %d, chroma filter %d", desc.transfer, d, s, desc.chroma);
        const YuvArgs a = yuv_transfer_args(s, src, src_fs, L, w, h, n, dst);
        int32_t c[7];
        YuvTransferCoef k{};
        yuv_transfer_coefficients(desc.range, c);
        k.cy = c[0]; k.cub = c[1]; k.cug = c[2]; k.cvg = c[3]; k.cvr = c[4]; k.yofs = c[5];
        yuv_transfer_gamut(k.g);
        const dim3 grid(cdiv(cdiv(w, 4), YUV_TX), cdiv(rows2 ? h / 2 : h, YUV_TY * YUV_TRK_ROWS), n);
        yuv_dispatch(s, d, [&](auto S, auto D) {
            if constexpr (S() != YUV_S422P && D() != YUV_D8) yuv_transfer_to_bgr_kernel<S(), D()><<<grid, block, 0, st>>>(a, k, tab);
            else yuv_no_kernel("transfer", s, d);
        });
        check_launch("yuv_transfer_to_bgr_kernel");
    } else if (desc.filtered()) {
        int32_t w12[12];
        YuvArgs a;
        YuvChromaW wt;
        if (!yuv_chroma_weights(desc.chroma, s, w12) || !yuv_chroma_args(s, d, w12, src, src_fs, L, w, h, n, dst, &a, &wt))
            fail(SLIDEO_ERR_HIP, "internal: no chroma filter kernel for filter %d under sampling %d", desc.chroma, s);
        const YuvCoef k = yuv_coef(desc);
        const dim3 grid(cdiv(cdiv(w, 4), YUV_TX), cdiv(rows2 ? h / 2 : h, YUV_TY), n);
        yuv_dispatch(s, d, [&](auto S, auto D) {
            if constexpr (S() != YUV_S444) yuv_chroma_to_bgr_kernel<S(), D()><<<grid, block, 0, st>>>(a, wt, k);
            else yuv_no_kernel("chroma filter", s, d);
        });
        check_launch("yuv_chroma_to_bgr_kernel");
    } else if (!rows2) {
        const YuvArgs a = yuv_sampled_args(s, d, src, src_fs, L, w, h, n, dst);
        const YuvCoef k = yuv_coef(desc);
        const dim3 grid(cdiv(cdiv(w, 4), YUV_TX), cdiv(h, YUV_TY), n);
        yuv_dispatch(s, d, [&](auto S, auto D) {
            if constexpr (S() != YUV_S420) yuv_sampled_to_bgr_kernel<S(), D()><<<grid, block, 0, st>>>(a, k);
            else yuv_no_kernel("sampling", s, d);
        });
        check_launch("yuv_sampled_to_bgr_kernel");
    } else {
        const YuvArgs a = yuv_desc_args(d, src, src_fs, L, w, h, n, dst);
        const YuvCoef k = yuv_coef(desc);
        const dim3 grid(cdiv(cdiv(w, 4), YUV_TX), cdiv(h / 2, YUV_TY), n);
        yuv_dispatch_depth(d, [&](auto D) { yuv420_to_bgr_desc_kernel<D()><<<grid, block, 0, st>>>(a, k); });
        check_launch("yuv420_to_bgr_desc_kernel");
    }
}

// n frames under a pixel format other than SLIDEO_PIXEL_BGR8 (a layout pixel_format_validate accepted: rows `stride`, frames src_fs
// apart) -> BGR8 at dst (stride 3w, frame stride 3wh)
void launch_pixels_to_bgr(int format, const uint8_t* src, int64_t src_fs, int stride, int w, int h, int n, uint8_t* dst, hipStream_t st) {
    if (format == SLIDEO_PIXEL_BGR8) fail(SLIDEO_ERR_HIP, "internal: SLIDEO_PIXEL_BGR8 frames are not converted");
    const PixArgs a = pixels_args(format, src, src_fs, stride, w, h, n, dst);
    const dim3 grid(cdiv(cdiv(w, 4), YUV_TX), cdiv(h, YUV_TY), n), block(YUV_TX, YUV_TY);
    const int form = pixel_format_form(format);
    if (form == PIX_PACKED3) pixels_to_bgr_kernel<PIX_PACKED3><<<grid, block, 0, st>>>(a);
    else if (form == PIX_PACKED4) pixels_to_bgr_kernel<PIX_PACKED4><<<grid, block, 0, st>>>(a);
    else pixels_to_bgr_kernel<PIX_PLANAR><<<grid, block, 0, st>>>(a);
    check_launch("pixels_to_bgr_kernel");
}

// n frames of a device frame list (tab_dev: their 3n plane addresses, device memory) -> the plan's staged layout at dst, frames
// P.frame_bytes apart: what a host list's copies leave there
void launch_frame_gather(const FrameListPlan& P, const uint8_t* const* tab_dev, int n, uint8_t* dst, hipStream_t st) {
    const GatherArgs a = frame_gather_args(P, tab_dev, dst);
    const dim3 grid(frame_gather_chunks(a), a.n_planes, n), block(GATHER_TX, GATHER_TY);
    frame_gather_kernel<<<grid, block, 0, st>>>(a);
    check_launch("frame_gather_kernel");
}

// n BGR8 images through the matcher's levels table; src == dst (and equal strides): in place
void launch_levels(slideo_matcher* m, const uint8_t* src, int64_t src_fs, int src_stride, uint8_t* dst, int64_t dst_fs, int dst_stride, int w, int h,
                   int n, hipStream_t st) {
    if (!m->fs.levels.set || !m->d_levels.p) fail(SLIDEO_ERR_HIP, "internal: no frame levels table to apply");
    const LevelsArgs a = levels_args(m->d_levels.as<uint8_t>(), src, src_fs, src_stride, dst, dst_fs, dst_stride, w, h, n);
    const dim3 grid(cdiv(cdiv(w, 4), LVL_TX), cdiv(h, LVL_TY), n), block(LVL_TX, LVL_TY);
    levels_kernel<<<grid, block, 0, st>>>(a);
    check_launch("levels_kernel");
}

// n BGR8 images through the matcher's gain field, and through its levels table in the same pass when `levels`
void launch_shading(slideo_matcher* m, bool levels, const uint8_t* src, int64_t src_fs, int src_stride, uint8_t* dst, int64_t dst_fs, int dst_stride,
                    int w, int h, int n, hipStream_t st) {
    const FrameShading& F = m->fs.shading;
    if (!F.set || !m->d_shading.p) fail(SLIDEO_ERR_HIP, "internal: no frame shading field to apply");
    if (levels && (!m->fs.levels.set || !m->d_levels.p)) fail(SLIDEO_ERR_HIP, "internal: no frame levels table to apply");
    if (w != F.aw || h != F.ah) fail(SLIDEO_ERR_INVALID_ARG, "analysed size %dx%d is not the frame shading's %dx%d", w, h, F.aw, F.ah);
    const ShadingArgs a = shading_args(m->d_shading.as<uint16_t>(), F.cell, levels ? m->d_levels.as<uint8_t>() : nullptr, src, src_fs, src_stride, dst,
                                       dst_fs, dst_stride, w, h, n);
    const dim3 grid(cdiv(cdiv(w, 4), LVL_TX), cdiv(h, LVL_TY), n), block(LVL_TX, LVL_TY);
    if (levels) shading_kernel<true><<<grid, block, 0, st>>>(a);
    else shading_kernel<false><<<grid, block, 0, st>>>(a);
    check_launch("shading_kernel");
}

// the reduce class (w, h) -> (dw, dh): ResizeAreaFast when both factors are integers (the test of resize.cpp, in double), else the
// tap tables under the matcher's ocv.area, uploaded once
static ReduceEntry& reduce_for(slideo_matcher* m, int w, int h, int dw, int dh) {
    for (auto& r : m->reduces) if (r->ag.sw == w && r->ag.sh == h && r->ag.dw == dw && r->ag.dh == dh) return *r;
    auto e = std::make_unique<ReduceEntry>();
    std::vector<AreaTap> taps;
    std::vector<int32_t> idx;
    if (!build_area_geom_to(w, h, dw, dh, e->ag, taps, idx, m->cfg.ocv.area))
        fail(SLIDEO_ERR_INVALID_ARG, "reduce %dx%d -> %dx%d is not a shrink", w, h, dw, dh);
    e->d_taps.reserve(std::max<size_t>(taps.size() * sizeof(AreaTap), 16));
    e->d_idx.reserve(std::max<size_t>(idx.size() * 4, 16));
    HIP_CHECK(hipMemcpyAsync(e->d_taps.p, taps.data(), taps.size() * sizeof(AreaTap), hipMemcpyHostToDevice, m->stream));
    HIP_CHECK(hipMemcpyAsync(e->d_idx.p, idx.data(), idx.size() * 4, hipMemcpyHostToDevice, m->stream));
    HIP_CHECK(hipStreamSynchronize(m->stream));              // the host vectors die here
    m->reduces.push_back(std::move(e));
    return *m->reduces.back();
}

// n BGR8 frames of w x h (rows `stride`, frames src_fs apart) -> resize(INTER_AREA) to dw x dh at dst (stride 3dw, frame stride 3dw dh)
void launch_reduce(slideo_matcher* m, const uint8_t* src, int64_t src_fs, int stride, int w, int h, int dw, int dh, int n, uint8_t* dst,
                   hipStream_t st) {
    const ReduceEntry& e = reduce_for(m, w, h, dw, dh);
    ReduceArgs a{};
    a.src = src; a.src_frame_stride = src_fs; a.src_stride = stride;
    a.dst = dst; a.sw = w; a.sh = h; a.dw = dw; a.dh = dh;
    a.ix = e.ag.iscale_x; a.iy = e.ag.iscale_y; a.inv_area = e.ag.fast_scale;
    a.out4 = (uintptr_t)dst % 4 == 0 && dw % 4 == 0;
    const dim3 grid(cdiv(cdiv(dw, 4), RED_TX), cdiv(dh, RED_TY), n), block(RED_TX, RED_TY);
    if (e.ag.fast) {
        // whole factors: w == ix dw and h == iy dh.  2x2 from 8-byte aligned rows through the dword kernel
        const bool aligned = a.ix == 2 && a.iy == 2 && a.out4 && (uintptr_t)src % 8 == 0 && stride % 8 == 0 && src_fs % 8 == 0;
        if (aligned) reduce2x2_kernel<<<grid, block, 0, st>>>(a);
        else reduce_int_kernel<<<grid, block, 0, st>>>(a);
    } else {
        reduce_area_kernel<<<grid, block, 0, st>>>(a, e.ag, e.d_taps.as<AreaTap>(), e.d_idx.as<int32_t>());
    }
    check_launch("reduce kernel");
}

void frame_region_classify(FrameRegion& R) { R.kind = rect_classify(R.M, R.tx, R.ty); }

// n BGR8 frames of R.src_w x R.src_h (rows `stride`, frames src_fs apart) -> their rectified images at dst (stride 3 out_w).
// L (a lens that is set): the ONE launch undistorts as well — lens_kernel, with the region's map in front where R is set, else at
// the lens's source size
void launch_rectify(const FrameRegion& R, const FrameLens* L, const uint8_t* src, int64_t src_fs, int stride, int n, uint8_t* dst, hipStream_t st) {
    if (L) {
        const int dw = R.set ? R.out_w : L->src_w, dh = R.set ? R.out_h : L->src_h;
        const LensArgs a = lens_args(R.set ? R.M : nullptr, L->cx, L->cy, L->q, L->k1, L->k2, src, src_fs, stride, L->src_w, L->src_h, dst, dw, dh);
        const dim3 grid(cdiv(cdiv(dw, 4), RECT_TX), cdiv(dh, RECT_TY), n), block(RECT_TX, RECT_TY);
        if (R.set) lens_kernel<true><<<grid, block, 0, st>>>(a);
        else lens_kernel<false><<<grid, block, 0, st>>>(a);
        check_launch("lens_kernel");
        return;
    }
    const RectifyArgs a = rect_args(R.M, R.kind, R.tx, R.ty, src, src_fs, stride, R.src_w, R.src_h, dst, R.out_w, R.out_h);
    const dim3 grid(cdiv(cdiv(R.out_w, 4), RECT_TX), cdiv(R.out_h, RECT_TY), n), block(RECT_TX, RECT_TY);
    if (R.kind == RECT_TRANSLATE) rectify_kernel<RECT_TRANSLATE><<<grid, block, 0, st>>>(a);
    else if (R.kind == RECT_AFFINE) rectify_kernel<RECT_AFFINE><<<grid, block, 0, st>>>(a);
    else rectify_kernel<RECT_PROJECTIVE><<<grid, block, 0, st>>>(a);
    check_launch("rectify_kernel");
}

void frame_lens_point(double cx, double cy, double q, double k1, double k2, double u, double v, double* xd, double* yd) {
    lens_point(cx, cy, q, k1, k2, u, v, *xd, *yd);
}

void orb_launch_scan(const uint32_t* counts, int n, uint32_t* qofs, uint32_t* info, hipStream_t st) {
    scan_kernel<<<1, 1024, 0, st>>>(counts, n, qofs, info);
    check_launch("scan_kernel");
}

// ---- ORB over `n` equally sized frames already on the device, in three steps -------------
// stage 1: gray, pyramid, FAST+NMS, blur, retainBest thresholds, per-frame offsets; copies {Qtot, max, flags} to pinned memory
static void launch_blur(slideo_matcher* m, Slot& S, const PyrGeom& g, int n, const uint8_t* strip_mask) {
    hipStream_t st = S.st;
    if (m->cfg.ocv.blur == 0)
        blur_f32_kernel<true><<<dim3(g.blur_tiles, n), 256, 0, st>>>(g, S.d_pyr.as<uint8_t>(), S.d_blur.as<uint8_t>(), m->d_tables.as<OrbTables>(), strip_mask);
    else if (m->cfg.ocv.blur == 1)
        blur_f32_kernel<false><<<dim3(g.blur_tiles, n), 256, 0, st>>>(g, S.d_pyr.as<uint8_t>(), S.d_blur.as<uint8_t>(), m->d_tables.as<OrbTables>(), strip_mask);
    else
        blur_kernel<<<dim3(g.blur_tiles, n), 256, 0, st>>>(g, S.d_pyr.as<uint8_t>(), S.d_blur.as<uint8_t>(), m->d_tables.as<OrbTables>());
    check_launch("blur kernel");
}

// SLIDEO_RESIZE_GENERIC=1: every pyramid level through resize_kernel (the form for any shrink factor) instead of resize_quad_kernel
static bool resize_generic_forced() { return env_long("SLIDEO_RESIZE_GENERIC", 0) != 0; }      // (read per unit: the tests switch it)

// `with_blur`: also materialise the WHOLE blurred pyramid (only the pyramid tap wants it)
// the f32 blur of ocv.blur 0 / 1 cannot be evaluated per BRIEF sample in integer arithmetic: those variants always
// materialise the blurred pyramid (blur_f32_kernel) and describe from it (describe_blurred_kernel)
void orb_stage1(slideo_matcher* m, Slot& S, const DevFrames& f, int n, bool with_blur, uint32_t kp_cap, const uint8_t* mask_pyr) {
    hipStream_t st = S.st;
    const int w = f.w, h = f.h;
    const bool full_blur = with_blur;
    with_blur = with_blur || blur_is_f32(m);
    GeomEntry& ge = geom_for(m, w, h);
    const PyrGeom& g = ge.g;
    const int L = g.nlevels;
    S.d_pyr.reserve((size_t)g.frame_bytes * n + 256);      // + slack: describe_kernel stages whole dwords past a window's last byte
    if (with_blur) S.d_blur.reserve((size_t)g.frame_bytes * n);
    S.d_cand.reserve(std::max<size_t>((size_t)g.cand_per_frame * n * 4, 16));
    const size_t n_cc = (size_t)n * L;
    S.d_hist.reserve(n_cc * 256 * 4);
    S.d_candcount.reserve(n_cc * 2 * 4);
    S.d_flags.reserve(16);
    uint32_t* hist = S.d_hist.as<uint32_t>();
    uint32_t* cand_count = S.d_candcount.as<uint32_t>();
    uint32_t* flags = S.d_flags.as<uint32_t>();
    HIP_CHECK(hipMemsetAsync(hist, 0, n_cc * 256 * 4, st));
    HIP_CHECK(hipMemsetAsync(cand_count, 0, n_cc * 2 * 4, st));
    HIP_CHECK(hipMemsetAsync(flags, 0, 16, st));
    S.d_thr.reserve(n_cc * 4); S.d_lvlofs.reserve(n_cc * 4); S.d_kpcount.reserve((size_t)n * 4);
    S.d_qofs.reserve((size_t)(n + 1) * 4); S.d_info.reserve(64);
    S.h_info.reserve(64);

    const int aligned4 = ((uintptr_t)f.p % 4 == 0) && (f.stride % 4 == 0) && (f.frame_stride % 4 == 0);
    {
        dim3 grid(cdiv(cdiv(w, 4), 256), h, n);
        gray_kernel<<<grid, 256, 0, st>>>(f.p, f.frame_stride, f.stride, S.d_pyr.as<uint8_t>(), g.frame_bytes, w, h,
                                          g.lv[0].pitch, aligned4, gray_coef(m));
        check_launch("gray_kernel");
    }
    for (int l = 1; l < L; ++l) {
        if (g.lv[l].w <= 0 || g.lv[l].h <= 0) continue;
        // flat thread index t -> (row, 4-pixel group) = (t / nxq, t % nxq); magic = ceil(2^32 / nxq) divides
        // exactly while nxq^2 * h < 2^32, which MAX_DIM guarantees
        const int nxq = cdiv(g.lv[l].w, 4);
        const uint32_t magic = nxq > 1 ? (uint32_t)(((1ull << 32) + (uint64_t)nxq - 1) / (uint64_t)nxq) : 0u;
        dim3 grid(cdiv(nxq * cdiv(g.lv[l].h, RESIZE_ROWS), 256), 1, n);
        if (g.lv[l].rq_ok && !resize_generic_forced())
            resize_quad_kernel<<<grid, 256, 0, st>>>(S.d_pyr.as<uint8_t>(), g.frame_bytes, g.lv[l - 1], g.lv[l], ge.lin_tab.as<uint32_t>(),
                                                     nxq, magic);
        else
            resize_kernel<<<grid, 256, 0, st>>>(S.d_pyr.as<uint8_t>(), g.frame_bytes, g.lv[l - 1], g.lv[l], ge.lin_tab.as<uint32_t>(),
                                                nxq, magic);
        check_launch("resize kernel");
    }
    if (g.fast_tiles > 0) {
        fast_kernel<<<dim3(cdiv(g.fast_tiles, FAST_TPB), n), 256, 0, st>>>(g, S.d_pyr.as<uint8_t>(), S.d_cand.as<uint32_t>(), cand_count, hist, ge.fast_tiles.as<int4>());
        check_launch("fast_kernel");
        // frame mask: the candidates the mask forbids leave the lists before retainBest counts them
        if (mask_pyr) {
            mask_filter_kernel<<<dim3(L, n), MASK_BLOCK, 0, st>>>(g, mask_pyr, S.d_cand.as<uint32_t>(), cand_count, hist);
            check_launch("mask_filter_kernel");
        }
    }
    // the whole blurred pyramid only for the pyramid tap; on the frame path the f32 variants blur in stage 2, and only the strips
    // the kept keypoints sample (blur_mark_kernel)
    if (full_blur && g.blur_tiles > 0) launch_blur(m, S, g, n, nullptr);
    threshold_kernel<<<n, 64 * L, 0, st>>>(g, hist, cand_count, S.d_thr.as<uint32_t>(), S.d_lvlofs.as<uint32_t>(),
                                           S.d_kpcount.as<uint32_t>(), flags, kp_cap);
    check_launch("threshold_kernel");
    scan_kernel<<<1, 1024, 0, st>>>(S.d_kpcount.as<uint32_t>(), n, S.d_qofs.as<uint32_t>(), S.d_info.as<uint32_t>());
    check_launch("scan_kernel");
    HIP_CHECK(hipMemcpyAsync(S.h_info.p, S.d_info.p, 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(S.h_info.as<uint32_t>() + 2, flags, 4, hipMemcpyDeviceToHost, st));
    S.orb.nframes = n;
    S.orb.full_blur = full_blur;
}

// the one mid-pipeline host sync: 12 bytes that size everything downstream
void orb_wait_info(slideo_matcher* m, Slot& S) {
    HIP_CHECK(hipStreamSynchronize(S.st));
    const uint32_t qtot = S.h_info.as<uint32_t>()[0], maxc = S.h_info.as<uint32_t>()[1], fl = S.h_info.as<uint32_t>()[2];
    if (fl & 1u) fail(SLIDEO_ERR_HIP, "internal: FAST candidate list overflow");
    S.orb.qtot = qtot; S.orb.max_count = maxc;
}

// stage 2: compact the kept candidates, canonical sort, IC angle + rotated BRIEF
// by_capacity: qtot / maxc are CAPACITIES (n * kp_cap, kp_cap) and the real counts stay on the device
void orb_stage2(slideo_matcher* m, Slot& S, int w, int h, bool by_capacity) {
    hipStream_t st = S.st;
    const PyrGeom& g = geom_for(m, w, h).g;
    const int L = g.nlevels, n = S.orb.nframes;
    const uint32_t qtot = S.orb.qtot, maxc = S.orb.max_count;
    const uint32_t qtot_arg = by_capacity ? 0xFFFFFFFFu : qtot;
    S.d_items.reserve(std::max<size_t>((size_t)qtot * 8, 16));
    S.d_kp.reserve(std::max<size_t>((size_t)qtot * sizeof(slideo_keypoint), 16));
    S.d_desc.reserve(std::max<size_t>((size_t)qtot * 32, 32));
    if (qtot == 0) return;
    uint32_t* cand_count = S.d_candcount.as<uint32_t>();
    uint32_t* cursor = cand_count + (size_t)n * L;
    compact_kernel<<<dim3(L, n), 256, 0, st>>>(g, S.d_cand.as<uint32_t>(), cand_count, S.d_thr.as<uint32_t>(),
                                               S.d_lvlofs.as<uint32_t>(), S.d_qofs.as<uint32_t>(), cursor, S.d_items.as<uint64_t>());
    check_launch("compact_kernel");
    int np2 = 2;
    while ((uint32_t)np2 < maxc && np2 < KP_SORT_LDS) np2 <<= 1;
    sort_kernel<<<n, 1024, (size_t)np2 * 8, st>>>(S.d_qofs.as<uint32_t>(), S.d_items.as<uint64_t>(), np2);
    check_launch("sort_kernel");
    if (maxc > (uint32_t)np2) {                       // only reachable through the exact-size path (kp_cap_for <= KP_SORT_LDS)
        sort_global_kernel<<<n, 1024, 0, st>>>(S.d_qofs.as<uint32_t>(), S.d_items.as<uint64_t>(), (uint32_t)np2);
        check_launch("sort_global_kernel");
    }
    if (blur_is_f32(m)) {
        if (!S.orb.full_blur && g.blur_tiles > 0) {
            const size_t mask_bytes = (size_t)n * g.blur_tiles * 4;
            S.d_blurmask.reserve(mask_bytes);
            HIP_CHECK(hipMemsetAsync(S.d_blurmask.p, 0, mask_bytes, st));
            blur_mark_kernel<<<cdiv((int)qtot, 256), 256, 0, st>>>(g, S.d_qofs.as<uint32_t>(), n, S.d_items.as<uint64_t>(), qtot_arg, S.d_blurmask.as<uint8_t>());
            check_launch("blur_mark_kernel");
            launch_blur(m, S, g, n, S.d_blurmask.as<uint8_t>());
        }
        describe_blurred_kernel<<<cdiv((int)qtot, 4), 256, 0, st>>>(g, S.d_pyr.as<uint8_t>(), S.d_blur.as<uint8_t>(), m->d_tables.as<OrbTables>(),
                                                                    S.d_qofs.as<uint32_t>(), n, S.d_items.as<uint64_t>(), qtot_arg,
                                                                    m->d_ictab.as<uint2>(), m->ic_shift, m->ic_entries,
                                                                    S.d_kp.as<slideo_keypoint>(), S.d_desc.as<uint8_t>(), m->cfg.ocv.atan);
        check_launch("describe_blurred_kernel");
        return;
    }
    const DescWin dw = describe_window(g.half_patch);
    describe_kernel<<<cdiv((int)qtot, 4), 256, (size_t)dw.dwords * 16, st>>>(g, S.d_pyr.as<uint8_t>(), m->d_tables.as<OrbTables>(),
                                                                             S.d_qofs.as<uint32_t>(), n, S.d_items.as<uint64_t>(), qtot_arg, dw,
                                                                             m->d_ictab.as<uint2>(), m->ic_shift, m->ic_entries,
                                                                             S.d_kp.as<slideo_keypoint>(), S.d_desc.as<uint8_t>(), m->cfg.ocv.atan);
    check_launch("describe_kernel");
}

// synchronous ORB (page ingest, taps).  Leaves: d_qofs[n+1], d_kp[qtot], d_desc[qtot*32]; S.orb filled.
void run_orb(slideo_matcher* m, Slot& S, const DevFrames& f, int n, bool keep_host_qofs, bool with_blur, const uint8_t* mask_pyr) {
    orb_stage1(m, S, f, n, with_blur, 0xFFFFFFFFu, mask_pyr);
    orb_wait_info(m, S);
    orb_stage2(m, S, f.w, f.h);
    if (keep_host_qofs) {
        S.orb.qofs.resize(n + 1);
        HIP_CHECK(hipMemcpyAsync(S.orb.qofs.data(), S.d_qofs.p, (size_t)(n + 1) * 4, hipMemcpyDeviceToHost, S.st));
        HIP_CHECK(hipStreamSynchronize(S.st));
    }
}

// ---- frame mask (include/slideo_amd.h "Frame mask") ---------------------------------------------------------------------------
// The mask pyramid: level 0 the mask as given, level l the image pyramid's own resize (resize_kernel, the w x h geometry's tap
// tables) of level l - 1 followed by threshold(254, THRESH_TOZERO) — one frame in the pyramid's level layout, so that a FAST
// candidate's (y, x) indexes its level directly.  Made once per mask, here, into `out`; the matcher is idle.
void frame_mask_build(slideo_matcher* m, const uint8_t* mask, int w, int h, int stride, DevBuf& out) {
    GeomEntry& ge = geom_for(m, w, h);
    const PyrGeom& g = ge.g;
    hipStream_t st = m->stream;
    out.reserve((size_t)g.frame_bytes + 256);
    uint8_t* pyr = out.as<uint8_t>();
    HIP_CHECK(hipMemsetAsync(pyr, 0, (size_t)g.frame_bytes + 256, st));
    HIP_CHECK(hipMemcpy2DAsync(pyr + g.lv[0].ofs, g.lv[0].pitch, mask, stride, w, h, hipMemcpyHostToDevice, st));
    for (int l = 1; l < g.nlevels; ++l) {
        if (g.lv[l].w <= 0 || g.lv[l].h <= 0) continue;
        const int nxq = cdiv(g.lv[l].w, 4);               // (the launch arithmetic of orb_stage1's pyramid loop)
        const uint32_t magic = nxq > 1 ? (uint32_t)(((1ull << 32) + (uint64_t)nxq - 1) / (uint64_t)nxq) : 0u;
        resize_kernel<<<dim3(cdiv(nxq * cdiv(g.lv[l].h, RESIZE_ROWS), 256), 1, 1), 256, 0, st>>>(pyr, g.frame_bytes, g.lv[l - 1], g.lv[l],
                                                                                                 ge.lin_tab.as<uint32_t>(), nxq, magic);
        check_launch("resize_kernel (frame mask)");
        mask_threshold_kernel<<<cdiv(g.lv[l].w * g.lv[l].h, MASK_BLOCK), MASK_BLOCK, 0, st>>>(pyr, g.lv[l]);
        check_launch("mask_threshold_kernel");
    }
    HIP_CHECK(hipStreamSynchronize(st));                  // (the caller's mask bytes are copied: they may go)
}

const uint8_t* frame_mask_for(const slideo_matcher* m, int w, int h) {
    const FrameMask& k = m->fs.mask;
    if (!k.set) return nullptr;
    if (w != k.w || h != k.h)
        fail(SLIDEO_ERR_INVALID_ARG, "frame mask: the frames are analysed at %dx%d, the mask is %dx%d (slideo_matcher_set_frame_mask)", w, h, k.w, k.h);
    if (!(m->fs.mask_scope & SLIDEO_MASK_DETECT)) return nullptr;    // (a GATE-only mask: the size rule above, no filter)
    return m->d_mask_pyr.as<uint8_t>();
}

}  // namespace slideo
