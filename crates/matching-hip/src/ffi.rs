//! Hand-written declarations of include/slideo_amd.h (ABI 7) — what bindgen would emit for the entry points this crate
//! uses.  Field order and types mirror the C structs exactly; tests/test_capi_load.py pins the C side's layout
//! (sizeof(slideo_config) == 168) and `assert_abi()` below pins the version at run time.
#![allow(non_camel_case_types)]
use std::os::raw::{c_char, c_void};

pub const SLIDEO_ABI_VERSION: u32 = 7;
pub const SLIDEO_MASK_DETECT: u32 = 1;
pub const SLIDEO_MASK_GATE: u32 = 2;
pub const SLIDEO_DIRECT_WHOLE: u32 = 0;
pub const SLIDEO_DIRECT_VALID: u32 = 1;
pub const SLIDEO_GATE_PREVIOUS: u32 = 0;
pub const SLIDEO_GATE_ANCHOR: u32 = 1;
pub const SLIDEO_GROUP_GATE_HALO: u32 = 0;
pub const SLIDEO_GROUP_GATE_CHAIN: u32 = 1;
pub const SLIDEO_GATE_MEMORY_MAX: i32 = 64;
pub const SLIDEO_GATE_REF_RESET: i64 = -1;
pub const SLIDEO_GATE_REF_DEFERRED: i64 = -2;
pub const SLIDEO_YUV_MATRIX_BT601: i32 = 0;
pub const SLIDEO_YUV_MATRIX_BT709: i32 = 1;
pub const SLIDEO_YUV_RANGE_LIMITED: i32 = 0;
pub const SLIDEO_YUV_RANGE_FULL: i32 = 1;
pub const SLIDEO_YUV_DEPTH_8: i32 = 0;
pub const SLIDEO_YUV_DEPTH_10_MSB: i32 = 1;
pub const SLIDEO_YUV_DEPTH_10_LSB: i32 = 2;
pub const SLIDEO_YUV_SAMPLING_420: i32 = 0;
pub const SLIDEO_YUV_SAMPLING_422: i32 = 1;
pub const SLIDEO_YUV_SAMPLING_444: i32 = 2;
pub const SLIDEO_YUV_SAMPLING_422_PACKED: i32 = 3;
pub const SLIDEO_YUV_CHROMA_NEAREST: i32 = 0;
pub const SLIDEO_YUV_CHROMA_BILINEAR_LEFT: i32 = 1;
pub const SLIDEO_YUV_CHROMA_BILINEAR_CENTER: i32 = 2;
pub const SLIDEO_YUV_CHROMA_BILINEAR_TOPLEFT: i32 = 3;
pub const SLIDEO_YUV_TRANSFER_SDR: i32 = 0;
pub const SLIDEO_YUV_TRANSFER_HLG: i32 = 1;
pub const SLIDEO_YUV_TRANSFER_PQ: i32 = 2;
pub const SLIDEO_PIXEL_BGR8: i32 = 0;
pub const SLIDEO_PIXEL_RGB8: i32 = 1;
pub const SLIDEO_PIXEL_BGRA8: i32 = 2;
pub const SLIDEO_PIXEL_RGBA8: i32 = 3;
pub const SLIDEO_PIXEL_ARGB8: i32 = 4;
pub const SLIDEO_PIXEL_ABGR8: i32 = 5;
pub const SLIDEO_PIXEL_PLANAR_RGB8: i32 = 6;
pub const SLIDEO_PIXEL_PLANAR_BGR8: i32 = 7;
pub const SLIDEO_PIXEL_PLANAR_GBR8: i32 = 8;

/// slideo_ocv_variants: which restatement of each OpenCV primitive runs.  slideo_config_default fills it; the
/// application never touches it.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct slideo_ocv_variants {
    pub gray: i32,
    pub blur: i32,
    pub resize: i32,
    pub atan: i32,
    pub warp: i32,
    pub area: i32,
    pub lm: i32,
    pub rng_mul: u32,
    pub hdlt: i32,
}

/// slideo_config: every literal the reference hard-codes on the hot path; defaults = those literals.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct slideo_config {
    pub nfeatures: i32,
    pub scale_factor: f32,
    pub nlevels: i32,
    pub edge_threshold: i32,
    pub patch_size: i32,
    pub fast_threshold: i32,
    pub knn_k: i32,
    pub vote_tolerance: f32,
    pub max_candidate_pages: i32,
    pub ransac_threshold: f64,
    pub ransac_max_iters: i32,
    pub ransac_confidence: f64,
    pub refine_iters: i32,
    pub max_rated: i32,
    pub min_rating: f64,
    pub min_rating_ratio: f64,
    pub min_similarity: f32,
    pub small_area: i32,
    pub changed_similarity: f32,
    /// 0.0 = the reference's tolerance vote (default); > 0: ratio test instead (extension)
    pub ratio_test: f32,
    /// 0 = the reference's estimateAffinePartial2D (default); 1 = 8-DOF homography (extension)
    pub verify_model: i32,
    /// 0 = exact brute-force k-NN (default); 1 = the LSH candidate rule of the reference's FLANN index
    pub matcher: i32,
    pub lsh_tables: i32,
    pub lsh_key_bits: i32,
    pub lsh_multi_probe: i32,
    /// 0 = the reference's verdict (best similarity, mo/lib.rs:370-389; default); 1 = rating order, similarity only accepts
    pub verdict_rule: i32,
    pub ocv: slideo_ocv_variants,
}

#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct slideo_verdict {
    /// -1 = None
    pub page_idx: i32,
    pub similarity: f32,
    pub inliers: i32,
    pub n_keypoints: i32,
}

/// slideo_sift_config: cv::SIFT::create's parameters (the north-star's optional extractor, slideo_matcher_use_sift)
#[repr(C)]
#[derive(Clone, Copy)]
pub struct slideo_sift_config {
    pub nfeatures: i32,
    pub n_octave_layers: i32,
    pub contrast_threshold: f64,
    pub edge_threshold: f64,
    pub sigma: f64,
}

/// The N-device group (include/slideo_amd.h, "N-device group"): one matcher per GPU behind one handle.  This crate binds the
/// group form of every call; a group over one device is the single matcher.
#[repr(C)]
pub struct slideo_group {
    _private: [u8; 0],
}

/// One matcher on one device (the single-device handle; this crate drives the group, the YUV twins take either).
#[repr(C)]
pub struct slideo_matcher {
    _private: [u8; 0],
}

/// slideo_yuv420_layout (include/slideo_amd.h, "YUV 4:2:0 frames"): where the planes of one decoded frame sit, so that a VCN or
/// FFmpeg FrameSource hands its NV12 / I420 surface to the *_yuv420 calls as it is (pitched; chroma at pitch * aligned_height).
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct slideo_yuv420_layout {
    /// bytes between luma rows, >= width
    pub y_stride: i32,
    /// bytes between chroma rows
    pub uv_stride: i32,
    /// byte offset of the first U sample from the frame's base; the Y plane starts at the base
    pub u_offset: i64,
    /// byte offset of the first V sample
    pub v_offset: i64,
    /// 2 = interleaved (NV12 / NV21), 1 = planar (I420 / YV12)
    pub uv_step: i32,
    pub _pad: i32,
}

pub const SLIDEO_YUV420_NV12: i32 = 0;
pub const SLIDEO_YUV420_NV21: i32 = 1;
pub const SLIDEO_YUV420_I420: i32 = 2;
pub const SLIDEO_YUV420_YV12: i32 = 3;
pub const SLIDEO_YUV422_I422: i32 = 16;
pub const SLIDEO_YUV422_YV16: i32 = 17;
pub const SLIDEO_YUV422_NV16: i32 = 18;
pub const SLIDEO_YUV422_NV61: i32 = 19;
pub const SLIDEO_YUV422_YUY2: i32 = 20;
pub const SLIDEO_YUV422_UYVY: i32 = 21;
pub const SLIDEO_YUV422_YVYU: i32 = 22;
pub const SLIDEO_YUV422_VYUY: i32 = 23;
pub const SLIDEO_YUV444_I444: i32 = 24;
pub const SLIDEO_YUV444_YV24: i32 = 25;
pub const SLIDEO_YUV444_NV24: i32 = 26;
pub const SLIDEO_YUV444_NV42: i32 = 27;

extern "C" {
    pub fn slideo_abi_version() -> u32;
    pub fn slideo_config_default(cfg: *mut slideo_config);
    /// members of a group (n_devices 0 at create = every gfx950 device of the node)
    pub fn slideo_group_device_count(g: *const slideo_group) -> i32;
    pub fn slideo_group_create(
        cfg: *const slideo_config,
        n_devices: i32,
        devices: *const i32,
        out: *mut *mut slideo_group,
    ) -> i32;
    pub fn slideo_group_destroy(g: *mut slideo_group);
    pub fn slideo_group_last_error(g: *const slideo_group) -> *const c_char;
    pub fn slideo_group_add_pages_bgr8(
        g: *mut slideo_group,
        n_pages: i32,
        data: *const *const u8,
        width: *const i32,
        height: *const i32,
        stride_bytes: *const i32,
    ) -> i32;
    pub fn slideo_group_finalize_pages(g: *mut slideo_group) -> i32;
    pub fn slideo_group_match_frames_bgr8(
        g: *mut slideo_group,
        n_frames: i32,
        frames: *const u8,
        width: i32,
        height: i32,
        stride_bytes: i32,
        frame_stride_bytes: i64,
        verdicts_out: *mut slideo_verdict,
    ) -> i32;
    pub fn slideo_sift_config_default(cfg: *mut slideo_sift_config);
    /// optional: SIFT + L2 search in front of the verify stages (before the first page); ratio 0 = the path's tolerance vote
    pub fn slideo_group_use_sift(g: *mut slideo_group, cfg: *const slideo_sift_config, ratio: f32) -> i32;
    pub fn slideo_group_match_kept_frames(
        g: *mut slideo_group,
        n_sel: i32,
        sel: *const i32,
        verdicts_out: *mut slideo_verdict,
    ) -> i32;
    pub fn slideo_group_changed_mask_bgr8(
        g: *mut slideo_group,
        n_frames: i32,
        frames: *const u8,
        width: i32,
        height: i32,
        stride_bytes: i32,
        frame_stride_bytes: i64,
        prev_small: *const u8,
        last_small_out: *mut u8,
        changed_out: *mut u8,
        similarity_out: *mut f32,
    ) -> i32;
    // ---- decoded YUV 4:2:0 frames: the twins of the frame calls (same results as the BGR call on cvtColor's BGR image)
    pub fn slideo_yuv420_layout_packed(format: i32, width: i32, height: i32, out: *mut slideo_yuv420_layout) -> i32;
    pub fn slideo_yuv420_layout_packed16(format: i32, width: i32, height: i32, out: *mut slideo_yuv420_layout) -> i32;
    pub fn slideo_group_match_frames_yuv420(
        g: *mut slideo_group,
        n_frames: i32,
        frames: *const u8,
        width: i32,
        height: i32,
        layout: *const slideo_yuv420_layout,
        frame_stride_bytes: i64,
        verdicts_out: *mut slideo_verdict,
    ) -> i32;
    pub fn slideo_group_changed_mask_yuv420(
        g: *mut slideo_group,
        n_frames: i32,
        frames: *const u8,
        width: i32,
        height: i32,
        layout: *const slideo_yuv420_layout,
        frame_stride_bytes: i64,
        prev_small: *const u8,
        last_small_out: *mut u8,
        changed_out: *mut u8,
        similarity_out: *mut f32,
    ) -> i32;
    pub fn slideo_match_frames_yuv420(
        m: *mut slideo_matcher,
        n_frames: i32,
        frames: *const u8,
        width: i32,
        height: i32,
        layout: *const slideo_yuv420_layout,
        frame_stride_bytes: i64,
        verdicts_out: *mut slideo_verdict,
    ) -> i32;
    pub fn slideo_match_frames_yuv420_dev(
        m: *mut slideo_matcher,
        n_frames: i32,
        frames_dev: *const u8,
        width: i32,
        height: i32,
        layout: *const slideo_yuv420_layout,
        frame_stride_bytes: i64,
        verdicts_out: *mut slideo_verdict,
        hip_stream: *mut c_void,
    ) -> i32;
    pub fn slideo_match_frames_submit_yuv420_dev(
        m: *mut slideo_matcher,
        n_frames: i32,
        frames_dev: *const u8,
        width: i32,
        height: i32,
        layout: *const slideo_yuv420_layout,
        frame_stride_bytes: i64,
        hip_stream: *mut c_void,
        ticket_out: *mut i64,
    ) -> i32;
    pub fn slideo_changed_mask_yuv420(
        m: *mut slideo_matcher,
        n_frames: i32,
        frames: *const u8,
        width: i32,
        height: i32,
        layout: *const slideo_yuv420_layout,
        frame_stride_bytes: i64,
        prev_small: *const u8,
        last_small_out: *mut u8,
        changed_out: *mut u8,
        similarity_out: *mut f32,
    ) -> i32;
    pub fn slideo_yuv420_to_bgr8(
        m: *mut slideo_matcher,
        frame: *const u8,
        width: i32,
        height: i32,
        layout: *const slideo_yuv420_layout,
        bgr_out: *mut u8,
        out_capacity: i64,
    ) -> i32;
    // ---- changed-frame gate: MarkSimilarIter inside the unit pipeline (slideo_amd.h "Changed-frame gate").  A group of any member
    // count carries one gate state (slideo_group_gate_*, slideo_group_match_changed_frames_*): results equal a single matcher's.
    pub fn slideo_group_member(g: *mut slideo_group, i: i32) -> *mut slideo_matcher;
    pub fn slideo_changed_ssd_threshold(changed_similarity: f32, small_w: i32, small_h: i32) -> i64;
    pub fn slideo_matcher_gate_reset(m: *mut slideo_matcher, prev_small: *const u8, small_w: i32, small_h: i32) -> i32;
    pub fn slideo_matcher_gate_last_small(
        m: *mut slideo_matcher,
        out: *mut u8,
        out_capacity: i64,
        sw: *mut i32,
        sh: *mut i32,
    ) -> i32;
    pub fn slideo_match_changed_frames_bgr8(
        m: *mut slideo_matcher,
        n_frames: i32,
        frames: *const u8,
        width: i32,
        height: i32,
        stride_bytes: i32,
        frame_stride_bytes: i64,
        changed_out: *mut u8,
        similarity_out: *mut f32,
        verdicts_out: *mut slideo_verdict,
    ) -> i32;
    pub fn slideo_match_changed_frames_yuv420(
        m: *mut slideo_matcher,
        n_frames: i32,
        frames: *const u8,
        width: i32,
        height: i32,
        layout: *const slideo_yuv420_layout,
        frame_stride_bytes: i64,
        changed_out: *mut u8,
        similarity_out: *mut f32,
        verdicts_out: *mut slideo_verdict,
    ) -> i32;
    pub fn slideo_match_changed_frames_bgr8_dev(
        m: *mut slideo_matcher,
        n_frames: i32,
        frames_dev: *const u8,
        width: i32,
        height: i32,
        stride_bytes: i32,
        frame_stride_bytes: i64,
        changed_out: *mut u8,
        similarity_out: *mut f32,
        verdicts_out: *mut slideo_verdict,
        hip_stream: *mut c_void,
    ) -> i32;
    pub fn slideo_match_changed_frames_yuv420_dev(
        m: *mut slideo_matcher,
        n_frames: i32,
        frames_dev: *const u8,
        width: i32,
        height: i32,
        layout: *const slideo_yuv420_layout,
        frame_stride_bytes: i64,
        changed_out: *mut u8,
        similarity_out: *mut f32,
        verdicts_out: *mut slideo_verdict,
        hip_stream: *mut c_void,
    ) -> i32;
    pub fn slideo_match_changed_frames_submit_dev(
        m: *mut slideo_matcher,
        n_frames: i32,
        frames_dev: *const u8,
        width: i32,
        height: i32,
        stride_bytes: i32,
        frame_stride_bytes: i64,
        hip_stream: *mut c_void,
        ticket_out: *mut i64,
    ) -> i32;
    pub fn slideo_match_changed_frames_submit_yuv420_dev(
        m: *mut slideo_matcher,
        n_frames: i32,
        frames_dev: *const u8,
        width: i32,
        height: i32,
        layout: *const slideo_yuv420_layout,
        frame_stride_bytes: i64,
        hip_stream: *mut c_void,
        ticket_out: *mut i64,
    ) -> i32;
    pub fn slideo_match_changed_frames_collect(
        m: *mut slideo_matcher,
        ticket: i64,
        changed_out: *mut u8,
        similarity_out: *mut f32,
        verdicts_out: *mut slideo_verdict,
    ) -> i32;
    pub fn slideo_matcher_gate_reset_from_frame_bgr8(
        m: *mut slideo_matcher,
        frame: *const u8,
        width: i32,
        height: i32,
        stride_bytes: i32,
    ) -> i32;
    pub fn slideo_matcher_gate_reset_from_frame_yuv420(
        m: *mut slideo_matcher,
        frame: *const u8,
        width: i32,
        height: i32,
        layout: *const slideo_yuv420_layout,
    ) -> i32;
    pub fn slideo_matcher_gate_reset_from_frame_bgr8_dev(
        m: *mut slideo_matcher,
        frame_dev: *const u8,
        width: i32,
        height: i32,
        stride_bytes: i32,
        hip_stream: *mut c_void,
    ) -> i32;
    pub fn slideo_matcher_gate_reset_from_frame_yuv420_dev(
        m: *mut slideo_matcher,
        frame_dev: *const u8,
        width: i32,
        height: i32,
        layout: *const slideo_yuv420_layout,
        hip_stream: *mut c_void,
    ) -> i32;
    pub fn slideo_group_gate_reset(g: *mut slideo_group, prev_small: *const u8, small_w: i32, small_h: i32) -> i32;
    pub fn slideo_group_gate_last_small(
        g: *mut slideo_group,
        out: *mut u8,
        out_capacity: i64,
        sw: *mut i32,
        sh: *mut i32,
    ) -> i32;
    pub fn slideo_group_match_changed_frames_bgr8(
        g: *mut slideo_group,
        n_frames: i32,
        frames: *const u8,
        width: i32,
        height: i32,
        stride_bytes: i32,
        frame_stride_bytes: i64,
        changed_out: *mut u8,
        similarity_out: *mut f32,
        verdicts_out: *mut slideo_verdict,
    ) -> i32;
    pub fn slideo_group_match_changed_frames_yuv420(
        g: *mut slideo_group,
        n_frames: i32,
        frames: *const u8,
        width: i32,
        height: i32,
        layout: *const slideo_yuv420_layout,
        frame_stride_bytes: i64,
        changed_out: *mut u8,
        similarity_out: *mut f32,
        verdicts_out: *mut slideo_verdict,
    ) -> i32;
    // frame mask (include/slideo_amd.h "Frame mask"): mask null clears it
    pub fn slideo_matcher_set_frame_mask(
        m: *mut slideo_matcher,
        mask: *const u8,
        width: i32,
        height: i32,
        stride_bytes: i32,
    ) -> i32;
    pub fn slideo_matcher_frame_mask_info(
        m: *const slideo_matcher,
        width: *mut i32,
        height: *mut i32,
        is_set: *mut i32,
    ) -> i32;
    pub fn slideo_group_set_frame_mask(
        g: *mut slideo_group,
        mask: *const u8,
        width: i32,
        height: i32,
        stride_bytes: i32,
    ) -> i32;
    pub fn slideo_frame_mask_level(
        m: *mut slideo_matcher,
        level: i32,
        out: *mut u8,
        out_capacity: i64,
        lw: *mut i32,
        lh: *mut i32,
    ) -> i32;
    // frame mask scope (include/slideo_amd.h "Frame mask scope"): SLIDEO_MASK_DETECT | SLIDEO_MASK_GATE
    pub fn slideo_matcher_set_frame_mask_scope(m: *mut slideo_matcher, scope: u32) -> i32;
    pub fn slideo_matcher_frame_mask_scope(m: *const slideo_matcher, scope: *mut u32) -> i32;
    pub fn slideo_group_set_frame_mask_scope(g: *mut slideo_group, scope: u32) -> i32;
    pub fn slideo_changed_ssd_threshold_n(changed_similarity: f32, n_pixels: i64) -> i64;
    pub fn slideo_frame_mask_small(
        m: *mut slideo_matcher,
        out: *mut u8,
        out_capacity: i64,
        sw: *mut i32,
        sh: *mut i32,
        n_valid: *mut i64,
    ) -> i32;
    // direct page look-up (include/slideo_amd.h "Direct page look-up")
    pub fn slideo_matcher_set_direct_similarity(m: *mut slideo_matcher, t: f32) -> i32;
    pub fn slideo_matcher_direct_similarity(m: *const slideo_matcher, t: *mut f32) -> i32;
    pub fn slideo_group_set_direct_similarity(g: *mut slideo_group, t: f32) -> i32;
    pub fn slideo_direct_ssd_threshold(t: f32, n_pixels: i64) -> i64;
    pub fn slideo_page_small_ssd(
        m: *mut slideo_matcher,
        small: *const u8,
        n: i32,
        sw: i32,
        sh: i32,
        ssd_out: *mut u64,
    ) -> i32;
    // direct look-up scope (include/slideo_amd.h "Direct look-up scope"): SLIDEO_DIRECT_WHOLE / SLIDEO_DIRECT_VALID
    pub fn slideo_matcher_set_direct_scope(m: *mut slideo_matcher, scope: u32) -> i32;
    pub fn slideo_matcher_direct_scope(m: *const slideo_matcher, scope: *mut u32) -> i32;
    pub fn slideo_group_set_direct_scope(g: *mut slideo_group, scope: u32) -> i32;
    pub fn slideo_page_small_ssd_valid(
        m: *mut slideo_matcher,
        small: *const u8,
        n: i32,
        sw: i32,
        sh: i32,
        ssd_out: *mut u64,
    ) -> i32;
    // gate reference (include/slideo_amd.h "Gate reference"): SLIDEO_GATE_PREVIOUS / SLIDEO_GATE_ANCHOR
    pub fn slideo_matcher_set_gate_reference(m: *mut slideo_matcher, reference: u32) -> i32;
    pub fn slideo_matcher_gate_reference(m: *const slideo_matcher, reference: *mut u32) -> i32;
    pub fn slideo_group_set_gate_reference(g: *mut slideo_group, reference: u32) -> i32;
    // gate settle (include/slideo_amd.h "Gate settle"): under SLIDEO_GATE_ANCHOR, (settle_similarity, max_defer); 0: off
    pub fn slideo_matcher_set_gate_settle(m: *mut slideo_matcher, settle_similarity: f32, max_defer: i32) -> i32;
    pub fn slideo_matcher_gate_settle(m: *const slideo_matcher, settle_similarity: *mut f32, max_defer: *mut i32) -> i32;
    pub fn slideo_group_set_gate_settle(g: *mut slideo_group, settle_similarity: f32, max_defer: i32) -> i32;
    // gate state record (include/slideo_amd.h "Gate state record"): the whole gate state — anchor, previous image, deferral count — as bytes
    pub fn slideo_matcher_gate_state_bytes(m: *mut slideo_matcher, bytes: *mut i64) -> i32;
    pub fn slideo_matcher_gate_state_export(m: *mut slideo_matcher, out: *mut u8, capacity: i64, bytes: *mut i64) -> i32;
    pub fn slideo_matcher_gate_state_import(m: *mut slideo_matcher, rec: *const u8, bytes: i64) -> i32;
    // group gate order (include/slideo_amd.h "Group gate order"): SLIDEO_GROUP_GATE_HALO / SLIDEO_GROUP_GATE_CHAIN
    pub fn slideo_group_set_gate_order(g: *mut slideo_group, order: u32) -> i32;
    pub fn slideo_group_gate_order(g: *const slideo_group, order: *mut u32) -> i32;
    pub fn slideo_group_gate_state_export(g: *mut slideo_group, out: *mut u8, capacity: i64, bytes: *mut i64) -> i32;
    pub fn slideo_group_gate_state_import(g: *mut slideo_group, rec: *const u8, bytes: i64) -> i32;
    pub fn slideo_group_gate_chain_waited(g: *const slideo_group, member: i32, seconds: *mut f64) -> i32;
    // gate memory (include/slideo_amd.h "Gate memory"): under SLIDEO_GATE_ANCHOR, the last `capacity` matched frames; 0: off
    pub fn slideo_matcher_set_gate_memory(m: *mut slideo_matcher, capacity: i32) -> i32;
    pub fn slideo_matcher_gate_memory(m: *const slideo_matcher, capacity: *mut i32) -> i32;
    pub fn slideo_group_set_gate_memory(g: *mut slideo_group, capacity: i32) -> i32;
    pub fn slideo_matcher_last_gate_refs(m: *mut slideo_matcher, refs_out: *mut i64, capacity: i64, n: *mut i64) -> i32;
    pub fn slideo_group_last_gate_refs(g: *mut slideo_group, refs_out: *mut i64, capacity: i64, n: *mut i64) -> i32;
    pub fn slideo_small_gram_ssd(
        m: *mut slideo_matcher,
        small: *const u8,
        n: i32,
        sw: i32,
        sh: i32,
        use_valid: i32,
        ssd_out: *mut u64,
    ) -> i32;
    // YUV colour description (include/slideo_amd.h "YUV colour description"): SLIDEO_YUV_MATRIX_* / _RANGE_* / _DEPTH_*
    pub fn slideo_matcher_set_yuv_description(m: *mut slideo_matcher, matrix: i32, range: i32, depth: i32) -> i32;
    pub fn slideo_matcher_yuv_description(
        m: *const slideo_matcher,
        matrix: *mut i32,
        range: *mut i32,
        depth: *mut i32,
    ) -> i32;
    pub fn slideo_group_set_yuv_description(g: *mut slideo_group, matrix: i32, range: i32, depth: i32) -> i32;
    pub fn slideo_yuv_coefficients(matrix: i32, range: i32, out7: *mut i32) -> i32;
    // YUV sampling (include/slideo_amd.h "YUV sampling"): SLIDEO_YUV_SAMPLING_*; the layouts of SLIDEO_YUV422_* / SLIDEO_YUV444_*
    pub fn slideo_matcher_set_yuv_sampling(m: *mut slideo_matcher, sampling: i32) -> i32;
    pub fn slideo_matcher_yuv_sampling(m: *const slideo_matcher, sampling: *mut i32) -> i32;
    pub fn slideo_group_set_yuv_sampling(g: *mut slideo_group, sampling: i32) -> i32;
    pub fn slideo_yuv_layout_packed(format: i32, width: i32, height: i32, bytes_per_sample: i32, out: *mut slideo_yuv420_layout) -> i32;
    // YUV chroma filter (include/slideo_amd.h "YUV chroma filter"): SLIDEO_YUV_CHROMA_*; out12 = wh[2][3], wv[2][3]
    pub fn slideo_matcher_set_yuv_chroma(m: *mut slideo_matcher, filter: i32) -> i32;
    pub fn slideo_matcher_yuv_chroma(m: *const slideo_matcher, filter: *mut i32) -> i32;
    pub fn slideo_group_set_yuv_chroma(g: *mut slideo_group, filter: i32) -> i32;
    pub fn slideo_yuv_chroma_weights(filter: i32, sampling: i32, out12: *mut i32) -> i32;
    // YUV transfer (include/slideo_amd.h "YUV transfer"): SLIDEO_YUV_TRANSFER_*; white_nits 0 = 203; coef7, gamut9, lin1024, out4096
    pub fn slideo_matcher_set_yuv_transfer(m: *mut slideo_matcher, transfer: i32, white_nits: f32) -> i32;
    pub fn slideo_matcher_yuv_transfer(m: *const slideo_matcher, transfer: *mut i32, white_nits: *mut f32) -> i32;
    pub fn slideo_group_set_yuv_transfer(g: *mut slideo_group, transfer: i32, white_nits: f32) -> i32;
    pub fn slideo_yuv_transfer_tables(transfer: i32, range: i32, white_nits: f32, coef7: *mut i32, gamut9: *mut i32, lin1024: *mut u16, out4096: *mut u8) -> i32;
    // frame pixel format (include/slideo_amd.h "Frame pixel format"): SLIDEO_PIXEL_*; how every *_bgr8 frame call reads its frames
    pub fn slideo_matcher_set_pixel_format(m: *mut slideo_matcher, format: i32) -> i32;
    pub fn slideo_matcher_pixel_format(m: *const slideo_matcher, format: *mut i32) -> i32;
    pub fn slideo_group_set_pixel_format(g: *mut slideo_group, format: i32) -> i32;
    pub fn slideo_pixel_format_info(format: i32, bytes_per_pixel: *mut i32, planes: *mut i32) -> i32;
    pub fn slideo_pixels_to_bgr8(
        m: *mut slideo_matcher, frame: *const u8, width: i32, height: i32, stride_bytes: i32, bgr_out: *mut u8, out_capacity: i64,
    ) -> i32;
    // frame levels (include/slideo_amd.h "Frame levels"): a per-channel tone table uint8 [3][256] in front of the pipeline, and its learner
    pub fn slideo_matcher_set_frame_levels(m: *mut slideo_matcher, lut768: *const u8) -> i32;
    pub fn slideo_matcher_frame_levels(m: *const slideo_matcher, lut768_out: *mut u8, set_out: *mut i32) -> i32;
    pub fn slideo_group_set_frame_levels(g: *mut slideo_group, lut768: *const u8) -> i32;
    pub fn slideo_frame_levels_lut(lo: *const i32, hi: *const i32, lut768_out: *mut u8) -> i32;
    pub fn slideo_levels_bgr8(
        m: *mut slideo_matcher, bgr: *const u8, width: i32, height: i32, stride_bytes: i32, bgr_out: *mut u8, out_capacity: i64,
    ) -> i32;
    pub fn slideo_matcher_levels_begin(m: *mut slideo_matcher) -> i32;
    pub fn slideo_matcher_levels_end(m: *mut slideo_matcher) -> i32;
    pub fn slideo_matcher_levels_info(m: *mut slideo_matcher, frames: *mut i64, pixels: *mut i64) -> i32;
    pub fn slideo_matcher_levels_histogram(m: *mut slideo_matcher, hist768: *mut u64) -> i32;
    pub fn slideo_matcher_levels_points(m: *mut slideo_matcher, low_ppm: i32, high_ppm: i32, lo: *mut i32, hi: *mut i32) -> i32;
    // frame shading (include/slideo_amd.h "Frame shading"): a bilinear Q8.8 gain field uint16 [gh + 1][gw + 1] in front of the levels
    pub fn slideo_matcher_set_frame_shading(m: *mut slideo_matcher, aw: i32, ah: i32, cell: i32, gains: *const u16) -> i32;
    pub fn slideo_matcher_frame_shading(
        m: *const slideo_matcher, gains_out: *mut u16, capacity_elems: i64, aw: *mut i32, ah: *mut i32, cell: *mut i32, set_out: *mut i32,
    ) -> i32;
    pub fn slideo_group_set_frame_shading(g: *mut slideo_group, aw: i32, ah: i32, cell: i32, gains: *const u16) -> i32;
    pub fn slideo_shading_bgr8(
        m: *mut slideo_matcher, bgr: *const u8, width: i32, height: i32, stride_bytes: i32, bgr_out: *mut u8, out_capacity: i64,
    ) -> i32;
    pub fn slideo_shading_field(
        cnt: *const u64, sum_f: *const u64, sum_p: *const u64, gw: i32, gh: i32, cell: i32, min_count: i64, min_gain_q8: i32, max_gain_q8: i32,
        smooth: i32, gains_out: *mut u16, cells_used_out: *mut i32,
    ) -> i32;
    // match shading map (include/slideo_amd.h "Match shading map"): per-cell sums of matched pixel pairs, u64 [gh][gw] each
    pub fn slideo_matcher_shading_begin(m: *mut slideo_matcher, cell: i32, min_inliers: i32, min_hits: i32, flat: i32) -> i32;
    pub fn slideo_matcher_shading_end(m: *mut slideo_matcher) -> i32;
    pub fn slideo_matcher_shading_info(
        m: *mut slideo_matcher, cell: *mut i32, min_inliers: *mut i32, min_hits: *mut i32, flat: *mut i32, aw: *mut i32, ah: *mut i32, gw: *mut i32,
        gh: *mut i32, frames_through: *mut i64,
    ) -> i32;
    pub fn slideo_matcher_shading_sums(
        m: *mut slideo_matcher, cnt_out: *mut u64, sum_f_out: *mut u64, sum_p_out: *mut u64, capacity_elems: i64, gw: *mut i32, gh: *mut i32,
        frames_through: *mut i64, frames_counted: *mut i64,
    ) -> i32;
    pub fn slideo_group_shading_begin(g: *mut slideo_group, cell: i32, min_inliers: i32, min_hits: i32, flat: i32) -> i32;
    pub fn slideo_group_shading_end(g: *mut slideo_group) -> i32;
    pub fn slideo_group_shading_info(
        g: *mut slideo_group, cell: *mut i32, min_inliers: *mut i32, min_hits: *mut i32, flat: *mut i32, aw: *mut i32, ah: *mut i32, gw: *mut i32,
        gh: *mut i32, frames_through: *mut i64,
    ) -> i32;
    pub fn slideo_group_shading_sums(
        g: *mut slideo_group, cnt_out: *mut u64, sum_f_out: *mut u64, sum_p_out: *mut u64, capacity_elems: i64, gw: *mut i32, gh: *mut i32,
        frames_through: *mut i64, frames_counted: *mut i64,
    ) -> i32;
    // frame region (include/slideo_amd.h "Frame region"): frames stand for a rectified quadrilateral of themselves
    pub fn slideo_matcher_set_frame_region(
        m: *mut slideo_matcher,
        src_w: i32,
        src_h: i32,
        m9: *const f64,
        out_w: i32,
        out_h: i32,
    ) -> i32;
    pub fn slideo_matcher_frame_region(
        m: *const slideo_matcher,
        src_w: *mut i32,
        src_h: *mut i32,
        m9_out: *mut f64,
        out_w: *mut i32,
        out_h: *mut i32,
        is_set: *mut i32,
    ) -> i32;
    pub fn slideo_group_set_frame_region(
        g: *mut slideo_group,
        src_w: i32,
        src_h: i32,
        m9: *const f64,
        out_w: i32,
        out_h: i32,
    ) -> i32;
    pub fn slideo_frame_region_from_quad(quad: *const f64, out_w: i32, out_h: i32, m9_out: *mut f64) -> i32;
    pub fn slideo_rectify_bgr8(
        m: *mut slideo_matcher,
        bgr: *const u8,
        width: i32,
        height: i32,
        stride_bytes: i32,
        out: *mut u8,
        out_capacity: i64,
    ) -> i32;
    // frame lens (include/slideo_amd.h "Frame lens"): radial undistortion in the launch that rectifies
    pub fn slideo_matcher_set_frame_lens(m: *mut slideo_matcher, src_w: i32, src_h: i32, cx: f64, cy: f64, f: f64, k1: f64, k2: f64) -> i32;
    pub fn slideo_matcher_frame_lens(
        m: *const slideo_matcher,
        src_w: *mut i32,
        src_h: *mut i32,
        cx: *mut f64,
        cy: *mut f64,
        f: *mut f64,
        k1: *mut f64,
        k2: *mut f64,
        is_set: *mut i32,
    ) -> i32;
    pub fn slideo_group_set_frame_lens(g: *mut slideo_group, src_w: i32, src_h: i32, cx: f64, cy: f64, f: f64, k1: f64, k2: f64) -> i32;
    pub fn slideo_frame_lens_point(cx: f64, cy: f64, f: f64, k1: f64, k2: f64, u: f64, v: f64, xd: *mut f64, yd: *mut f64) -> i32;
    pub fn slideo_undistort_bgr8(
        m: *mut slideo_matcher,
        bgr: *const u8,
        width: i32,
        height: i32,
        stride_bytes: i32,
        out: *mut u8,
        out_capacity: i64,
    ) -> i32;
    // match evidence map (include/slideo_amd.h "Match evidence map"): where the keypoints of matched frames fall and which of them the
    // winning page's transform explains; the mask and the box made of the counts
    pub fn slideo_matcher_evidence_begin(m: *mut slideo_matcher, cell: i32, min_inliers: i32) -> i32;
    pub fn slideo_matcher_evidence_end(m: *mut slideo_matcher) -> i32;
    pub fn slideo_matcher_evidence_info(
        m: *mut slideo_matcher,
        cell: *mut i32,
        min_inliers: *mut i32,
        aw: *mut i32,
        ah: *mut i32,
        gw: *mut i32,
        gh: *mut i32,
        frames_through: *mut i64,
        frames_counted: *mut i64,
    ) -> i32;
    pub fn slideo_matcher_evidence_counts(
        m: *mut slideo_matcher,
        seen_out: *mut u32,
        hit_out: *mut u32,
        capacity_elems: i64,
        gw: *mut i32,
        gh: *mut i32,
        frames_through: *mut i64,
        frames_counted: *mut i64,
    ) -> i32;
    pub fn slideo_group_evidence_begin(g: *mut slideo_group, cell: i32, min_inliers: i32) -> i32;
    pub fn slideo_group_evidence_end(g: *mut slideo_group) -> i32;
    pub fn slideo_group_evidence_info(
        g: *mut slideo_group,
        cell: *mut i32,
        min_inliers: *mut i32,
        aw: *mut i32,
        ah: *mut i32,
        gw: *mut i32,
        gh: *mut i32,
        frames_through: *mut i64,
        frames_counted: *mut i64,
    ) -> i32;
    pub fn slideo_group_evidence_counts(
        g: *mut slideo_group,
        seen_out: *mut u32,
        hit_out: *mut u32,
        capacity_elems: i64,
        gw: *mut i32,
        gh: *mut i32,
        frames_through: *mut i64,
        frames_counted: *mut i64,
    ) -> i32;
    pub fn slideo_evidence_mask(
        seen: *const u32,
        hit: *const u32,
        gw: i32,
        gh: i32,
        cell: i32,
        aw: i32,
        ah: i32,
        min_seen: i64,
        min_hit_ppm: i32,
        grow: i32,
        mask_out: *mut u8,
        stride_bytes: i64,
    ) -> i32;
    pub fn slideo_evidence_box(
        seen: *const u32,
        hit: *const u32,
        gw: i32,
        gh: i32,
        cell: i32,
        aw: i32,
        ah: i32,
        min_hits: i64,
        min_hit_ppm: i32,
        box_out4: *mut i32,
    ) -> i32;
    pub fn slideo_matcher_rng_stream_len(m: *const slideo_matcher, len: *mut i64) -> i32;
    // match tone table (include/slideo_amd.h "Match tone table"): per channel and frame value, the page values of the small-image
    // pixels that the contributing candidate's hits enclose; the levels table made of the counts
    pub fn slideo_matcher_tone_begin(m: *mut slideo_matcher, min_inliers: i32, min_hits: i32, flat: i32) -> i32;
    pub fn slideo_matcher_tone_end(m: *mut slideo_matcher) -> i32;
    pub fn slideo_matcher_tone_info(
        m: *mut slideo_matcher,
        min_inliers: *mut i32,
        min_hits: *mut i32,
        flat: *mut i32,
        frames_through: *mut i64,
    ) -> i32;
    pub fn slideo_matcher_tone_counts(
        m: *mut slideo_matcher,
        cnt_out: *mut u64,
        sum_out: *mut u64,
        frames_through: *mut i64,
        frames_counted: *mut i64,
    ) -> i32;
    pub fn slideo_group_tone_begin(g: *mut slideo_group, min_inliers: i32, min_hits: i32, flat: i32) -> i32;
    pub fn slideo_group_tone_end(g: *mut slideo_group) -> i32;
    pub fn slideo_group_tone_info(
        g: *mut slideo_group,
        min_inliers: *mut i32,
        min_hits: *mut i32,
        flat: *mut i32,
        frames_through: *mut i64,
    ) -> i32;
    pub fn slideo_group_tone_counts(
        g: *mut slideo_group,
        cnt_out: *mut u64,
        sum_out: *mut u64,
        frames_through: *mut i64,
        frames_counted: *mut i64,
    ) -> i32;
    pub fn slideo_tone_lut(cnt: *const u64, sum: *const u64, min_count: i64, lut_out: *mut u8) -> i32;
    // match placement map (include/slideo_amd.h "Match placement map"): per cell, the frame positions of the keypoints the contributing
    // candidate explains and the unit-slide positions of their page points, summed; the keystoned quad fitted to the cells
    pub fn slideo_matcher_placement_begin(m: *mut slideo_matcher, cell: i32, min_inliers: i32, reach: f64) -> i32;
    pub fn slideo_matcher_placement_end(m: *mut slideo_matcher) -> i32;
    pub fn slideo_matcher_placement_info(
        m: *mut slideo_matcher,
        cell: *mut i32,
        min_inliers: *mut i32,
        reach: *mut f64,
        aw: *mut i32,
        ah: *mut i32,
        gw: *mut i32,
        gh: *mut i32,
        frames_through: *mut i64,
    ) -> i32;
    pub fn slideo_matcher_placement_sums(
        m: *mut slideo_matcher,
        n_out: *mut u64,
        sfx_out: *mut u64,
        sfy_out: *mut u64,
        su_out: *mut u64,
        sv_out: *mut u64,
        capacity_elems: i64,
        gw: *mut i32,
        gh: *mut i32,
        frames_through: *mut i64,
        frames_counted: *mut i64,
    ) -> i32;
    pub fn slideo_group_placement_begin(g: *mut slideo_group, cell: i32, min_inliers: i32, reach: f64) -> i32;
    pub fn slideo_group_placement_end(g: *mut slideo_group) -> i32;
    pub fn slideo_group_placement_info(
        g: *mut slideo_group,
        cell: *mut i32,
        min_inliers: *mut i32,
        reach: *mut f64,
        aw: *mut i32,
        ah: *mut i32,
        gw: *mut i32,
        gh: *mut i32,
        frames_through: *mut i64,
    ) -> i32;
    pub fn slideo_group_placement_sums(
        g: *mut slideo_group,
        n_out: *mut u64,
        sfx_out: *mut u64,
        sfy_out: *mut u64,
        su_out: *mut u64,
        sv_out: *mut u64,
        capacity_elems: i64,
        gw: *mut i32,
        gh: *mut i32,
        frames_through: *mut i64,
        frames_counted: *mut i64,
    ) -> i32;
    pub fn slideo_placement_quad(
        n: *const u64,
        sfx: *const u64,
        sfy: *const u64,
        su: *const u64,
        sv: *const u64,
        gw: i32,
        gh: i32,
        cell: i32,
        aw: i32,
        ah: i32,
        min_count: i64,
        trim_px: f64,
        rounds: i32,
        quad_out8: *mut f64,
        h_out9: *mut f64,
        cells_used: *mut i32,
        rms_px: *mut f64,
    ) -> i32;
    // placement lens (include/slideo_amd.h "Placement lens"): the frame lens and the quad fitted jointly to the same sums
    pub fn slideo_placement_lens(
        n: *const u64,
        sfx: *const u64,
        sfy: *const u64,
        su: *const u64,
        sv: *const u64,
        gw: i32,
        gh: i32,
        cell: i32,
        aw: i32,
        ah: i32,
        min_count: i64,
        cx: f64,
        cy: f64,
        f: f64,
        order: i32,
        trim_px: f64,
        rounds: i32,
        iters: i32,
        k_out2: *mut f64,
        quad_out8: *mut f64,
        h_out9: *mut f64,
        cells_used: *mut i32,
        rms_px: *mut f64,
    ) -> i32;
    // frame activity map (include/slideo_amd.h "Frame activity map"): per-pixel counts of moved pairs, and the mask read out of them
    pub fn slideo_matcher_activity_begin(m: *mut slideo_matcher, delta: i32) -> i32;
    pub fn slideo_matcher_activity_end(m: *mut slideo_matcher) -> i32;
    pub fn slideo_matcher_observe_frames_bgr8(
        m: *mut slideo_matcher,
        n_frames: i32,
        frames: *const u8,
        width: i32,
        height: i32,
        stride_bytes: i32,
        frame_stride_bytes: i64,
    ) -> i32;
    pub fn slideo_matcher_observe_frames_yuv420(
        m: *mut slideo_matcher,
        n_frames: i32,
        frames: *const u8,
        width: i32,
        height: i32,
        layout: *const slideo_yuv420_layout,
        frame_stride_bytes: i64,
    ) -> i32;
    pub fn slideo_matcher_observe_frames_bgr8_dev(
        m: *mut slideo_matcher,
        n_frames: i32,
        frames_dev: *const u8,
        width: i32,
        height: i32,
        stride_bytes: i32,
        frame_stride_bytes: i64,
        hip_stream: *mut c_void,
    ) -> i32;
    pub fn slideo_matcher_observe_frames_yuv420_dev(
        m: *mut slideo_matcher,
        n_frames: i32,
        frames_dev: *const u8,
        width: i32,
        height: i32,
        layout: *const slideo_yuv420_layout,
        frame_stride_bytes: i64,
        hip_stream: *mut c_void,
    ) -> i32;
    pub fn slideo_matcher_activity_info(
        m: *mut slideo_matcher,
        aw: *mut i32,
        ah: *mut i32,
        pairs: *mut i32,
        delta: *mut i32,
    ) -> i32;
    pub fn slideo_matcher_activity_counts(
        m: *mut slideo_matcher,
        out: *mut u32,
        capacity_elems: i64,
        aw: *mut i32,
        ah: *mut i32,
        pairs: *mut i32,
    ) -> i32;
    pub fn slideo_matcher_activity_mask(
        m: *mut slideo_matcher,
        max_share_ppm: i32,
        grow: i32,
        out: *mut u8,
        capacity: i64,
        aw: *mut i32,
        ah: *mut i32,
        n_active: *mut i64,
        n_masked: *mut i64,
    ) -> i32;
    // frame content box (include/slideo_amd.h "Frame content box"): per-pixel counts of lit frames, and the box read out of them;
    // the slideo_matcher_observe_frames_* calls above feed it
    pub fn slideo_matcher_content_begin(m: *mut slideo_matcher, level: i32) -> i32;
    pub fn slideo_matcher_content_end(m: *mut slideo_matcher) -> i32;
    pub fn slideo_matcher_content_info(
        m: *mut slideo_matcher,
        aw: *mut i32,
        ah: *mut i32,
        frames: *mut i32,
        level: *mut i32,
    ) -> i32;
    pub fn slideo_matcher_content_counts(
        m: *mut slideo_matcher,
        out: *mut u32,
        capacity_elems: i64,
        aw: *mut i32,
        ah: *mut i32,
        frames: *mut i32,
    ) -> i32;
    pub fn slideo_matcher_content_box(
        m: *mut slideo_matcher,
        min_share_ppm: i32,
        min_fill_ppm: i32,
        box_out: *mut i32,
        n_content: *mut i64,
        fill_out: *mut u32,
        fill_capacity_elems: i64,
    ) -> i32;
}

/// slideo_frame_list (include/slideo_amd.h, "Frame lists"): a batch described by per-frame plane pointers instead of base + stride,
/// so that frames decoded into separate buffers are matched without a copy into one batch.  `planes` is a host array of
/// `n_frames * 3` addresses; `stride[k]` the bytes between rows of the plane at `planes[3 * i + k]`.
pub const SLIDEO_FRAME_LIST_BGR: i32 = 0;
pub const SLIDEO_FRAME_LIST_YUV: i32 = 1;
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct slideo_frame_list {
    pub door: i32,
    pub on_device: i32,
    pub n_frames: i32,
    pub width: i32,
    pub height: i32,
    pub uv_step: i32,
    pub stride: [i64; 3],
    pub planes: *const *const c_void,
}

extern "C" {
    pub fn slideo_match_frames_list(
        m: *mut slideo_matcher,
        list: *const slideo_frame_list,
        verdicts_out: *mut slideo_verdict,
        hip_stream: *mut c_void,
    ) -> i32;
    pub fn slideo_match_frames_submit_list(
        m: *mut slideo_matcher,
        list: *const slideo_frame_list,
        hip_stream: *mut c_void,
        ticket_out: *mut i64,
    ) -> i32;
    pub fn slideo_match_changed_frames_list(
        m: *mut slideo_matcher,
        list: *const slideo_frame_list,
        changed_out: *mut u8,
        similarity_out: *mut f32,
        verdicts_out: *mut slideo_verdict,
        hip_stream: *mut c_void,
    ) -> i32;
    pub fn slideo_match_changed_frames_submit_list(
        m: *mut slideo_matcher,
        list: *const slideo_frame_list,
        hip_stream: *mut c_void,
        ticket_out: *mut i64,
    ) -> i32;
    pub fn slideo_changed_mask_list(
        m: *mut slideo_matcher,
        list: *const slideo_frame_list,
        prev_small: *const u8,
        last_small_out: *mut u8,
        changed_out: *mut u8,
        similarity_out: *mut f32,
    ) -> i32;
    pub fn slideo_matcher_observe_frames_list(m: *mut slideo_matcher, list: *const slideo_frame_list, hip_stream: *mut c_void) -> i32;
    pub fn slideo_matcher_gate_reset_from_frame_list(m: *mut slideo_matcher, list: *const slideo_frame_list, hip_stream: *mut c_void) -> i32;
    pub fn slideo_group_match_frames_list(g: *mut slideo_group, list: *const slideo_frame_list, verdicts_out: *mut slideo_verdict) -> i32;
    pub fn slideo_group_match_changed_frames_list(
        g: *mut slideo_group,
        list: *const slideo_frame_list,
        changed_out: *mut u8,
        similarity_out: *mut f32,
        verdicts_out: *mut slideo_verdict,
    ) -> i32;
    pub fn slideo_group_changed_mask_list(
        g: *mut slideo_group,
        list: *const slideo_frame_list,
        prev_small: *const u8,
        last_small_out: *mut u8,
        changed_out: *mut u8,
        similarity_out: *mut f32,
    ) -> i32;
    pub fn slideo_frame_list_to_bgr8(m: *mut slideo_matcher, list: *const slideo_frame_list, bgr_out: *mut u8, out_capacity: i64) -> i32;
}

/// The struct layouts above are only valid for one ABI version of the library.
pub fn assert_abi() {
    let v = unsafe { slideo_abi_version() };
    assert_eq!(
        v, SLIDEO_ABI_VERSION,
        "libslideo_amd.so has ABI {} but this crate was written for ABI {}",
        v, SLIDEO_ABI_VERSION
    );
    assert_eq!(std::mem::size_of::<slideo_config>(), 168);
    assert_eq!(std::mem::size_of::<slideo_verdict>(), 16);
    assert_eq!(std::mem::size_of::<slideo_yuv420_layout>(), 32);
    assert_eq!(std::mem::size_of::<slideo_frame_list>(), 56);
}
