//! matching-hip — hediet/slideo's `matching` trait surface (crates/matching/src/lib.rs:7-40) over the MI355X-native
//! matcher libslideo_amd.so.  A drop-in for crates/matching-opencv: same traits, same progress protocol, same
//! panics-instead-of-Results, same post-processing of the per-frame results.
//!
//!   OpenCVImageVideoMatcher::default()          -> HipImageVideoMatcher::default()
//!   create_video_matcher    (mo/lib.rs:37-64)   -> slideo_group_create (one matcher per GPU of the node) + add_pages_bgr8 +
//!                                                  finalize_pages: pages analysed across the devices, DB replicated
//!   match_images_with_video (mo/lib.rs:140-158) -> opens the video to size the progress bar, as the reference does
//!   process                 (mo/lib.rs:168-246) -> sampled frames in batches, each batch sharded over the devices:
//!                                                  slideo_group_match_changed_frames_bgr8 (MarkSimilarIter and the
//!                                                  match of the changed frames in one gated call); without the gate:
//!                                                  slideo_group_changed_mask_bgr8 (MarkSimilarIter,
//!                                                  mo/video_capture.rs:86-98), then slideo_group_match_kept_frames on
//!                                                  the changed ones (the mask's upload, on the device that holds it)
//!                                                  (match_images_with_frame, mo/lib.rs:249-413); sentinel, sort,
//!                                                  consecutive-duplicate removal as mo/lib.rs:185-189,229-244
//! (mo/ = crates/matching-opencv/src/)
//!
//! UNCOMPILED in the repository this crate ships in (no Rust toolchain there).
mod decode;
mod ffi;

use matching::{
    ImageVideoMatcher, MatchableImage, Matching, ProgressReporter, VideoMatcher, VideoMatcherTask,
};
use std::{
    ffi::CStr,
    path::{Path, PathBuf},
    sync::{Arc, Mutex},
    time::Duration,
};

/// Sampled frames handed to the library per call AND DEVICE.  The changed-frame mask needs consecutive samples in one call
/// (or the previous small image carried over, which is what happens at batch seams); 64 x 1080p = 400 MB of host memory
/// per device of the group.
const FRAMES_PER_CALL_PER_DEVICE: usize = 64;
/// The changed-frame gate inside the unit pipeline (slideo_group_match_changed_frames_bgr8); false: the stop-and-go pair
/// slideo_group_changed_mask_bgr8 + slideo_group_match_kept_frames, for comparisons.
const CHANGED_GATE: bool = true;

struct RawHandle(*mut ffi::slideo_group);
// The pointer itself may move between threads; USE is serialised by the Mutex below — include/slideo_amd.h: "a matcher
// is NOT re-entrant: calls on one handle must come from one thread at a time".
unsafe impl Send for RawHandle {}

struct Handle {
    raw: Mutex<RawHandle>,
}

impl Drop for Handle {
    fn drop(&mut self) {
        let g = self.raw.lock().unwrap_or_else(|e| e.into_inner());
        unsafe { ffi::slideo_group_destroy(g.0) }
    }
}

/// The reference has no `Result` anywhere on this surface: it panics (mo/lib.rs:95-104, unwrap() throughout).
fn check(h: *mut ffi::slideo_group, rc: i32) {
    if rc != 0 {
        let msg = unsafe { CStr::from_ptr(ffi::slideo_group_last_error(h)) }
            .to_string_lossy()
            .into_owned();
        panic!("slideo_amd error {}: {}", rc, msg);
    }
}

pub struct HipImageVideoMatcher {
    /// HIP device ordinals, one matcher each (slideo_group_create).  Empty (default) = every gfx950 device of the node:
    /// the reference fans out over the whole machine too (the global rayon pool, mo/lib.rs:45,174).
    pub devices: Vec<i32>,
    /// Some(ratio): the north-star's SIFT + L2 front end (slideo_group_use_sift) instead of the reference's ORB + Hamming;
    /// Some(0.0) keeps the path's own 5 % tolerance vote on the L2 distances (the robust choice on decks whose pages
    /// share a template), Some(r > 0) is Lowe's ratio test.  None (default) = the reference's extractor and matcher.
    pub sift_ratio: Option<f32>,
    /// Some((mask, width, height)): the frame mask (slideo_group_set_frame_mask), width x height bytes, nonzero = detect
    /// here; the frames' analysed size must be the mask's.  None (default) = no mask, as the reference.
    pub frame_mask: Option<(Vec<u8>, i32, i32)>,
    /// Which stages the frame mask applies to (slideo_group_set_frame_mask_scope): ffi::SLIDEO_MASK_DETECT (default),
    /// ffi::SLIDEO_MASK_GATE, or both.  With SLIDEO_MASK_GATE the changed-frame gate ignores the masked regions too.
    pub frame_mask_scope: u32,
    /// The direct page look-up (slideo_group_set_direct_similarity): t in (0, 1]; a changed frame whose small image is at
    /// least that similar to a page's is resolved to that page without ORB, search or verify (full-screen slide frames of a
    /// screen recording; the reference never decides without keypoints).  Not together with SLIDEO_MASK_GATE.  0.0 (default) = off.
    pub direct_similarity: f32,
    /// What the direct page look-up compares (slideo_group_set_direct_scope): ffi::SLIDEO_DIRECT_WHOLE (default: whole small
    /// images, refused beside SLIDEO_MASK_GATE) or ffi::SLIDEO_DIRECT_VALID (the valid pixels of the gate's validity map: a
    /// full-screen slide under a speaker thumbnail).  Applied before direct_similarity.
    pub direct_scope: u32,
    /// Some((src_w, src_h, quad, out_w, out_h)): the frame region (slideo_group_set_frame_region): frames of src_w x src_h
    /// stand for the out_w x out_h image rectified from the quad — the source coordinates x, y of the slide's top-left,
    /// top-right, bottom-right and bottom-left corner (slideo_frame_region_from_quad): a filmed projection screen, a slide
    /// in a sub-window.  The reference analyses the whole frame.  None (default) = no region.
    pub frame_region: Option<(i32, i32, [f64; 8], i32, i32)>,
    /// Some((src_w, src_h, cx, cy, f, k1, k2)): the frame lens (slideo_group_set_frame_lens): the radial distortion of a
    /// wide-angle room camera, c + (p - c) (1 + k1 r2 + k2 r2^2) with r2 = |p - c|^2 / f^2, removed in the launch that
    /// rectifies; frame_region's quad is then in ideal coordinates.  Applied after frame_region.  None (default) = no lens.
    pub frame_lens: Option<(i32, i32, f64, f64, f64, f64, f64)>,
    /// (matrix, range, depth): how YUV 4:2:0 frames are read (slideo_group_set_yuv_description): ffi::SLIDEO_YUV_MATRIX_* /
    /// _RANGE_* / _DEPTH_*.  BT.709 for HD recordings, full range for many screen recorders, a 10-bit depth for P010 /
    /// yuv420p10le frames.  The reference reads every stream as BT.601 limited range: the default (0, 0, 0).
    pub yuv_description: (i32, i32, i32),
    /// Where the samples of the YUV frames lie (slideo_group_set_yuv_sampling): ffi::SLIDEO_YUV_SAMPLING_420 (default), _422,
    /// _444 (screen recorders) or _422_PACKED (YUY2 / UYVY of capture cards; 8-bit).  Every call that takes a
    /// slideo_yuv420_layout reads its frames under it.  The reference knows BGR only.
    pub yuv_sampling: i32,
    /// How a pixel's chroma is read from 4:2:0 and 4:2:2 frames (slideo_group_set_yuv_chroma): ffi::SLIDEO_YUV_CHROMA_NEAREST
    /// (default: cvtColor's rule, and what the reference's swscale path does), _BILINEAR_LEFT (the siting of H.264 / HEVC / MPEG-2
    /// streams), _BILINEAR_CENTER (JPEG, MPEG-1) or _BILINEAR_TOPLEFT (BT.2020).  4:4:4 frames are untouched.
    pub yuv_chroma: i32,
    /// HDR frames to SDR (slideo_group_set_yuv_transfer): (ffi::SLIDEO_YUV_TRANSFER_SDR (default) | _HLG | _PQ, white_nits) — both
    /// BT.2020; white_nits is the display light that becomes SDR white, 0 = 203.  Needs a 10-bit depth in yuv_description and
    /// nearest chroma (or 4:4:4).  The reference knows no HDR.
    pub yuv_transfer: (i32, f32),
    /// How the frames of the BGR door are read (slideo_group_set_pixel_format): ffi::SLIDEO_PIXEL_BGR8 (default), _RGB8, the
    /// four-byte _BGRA8 / _RGBA8 / _ARGB8 / _ABGR8 of screen-capture APIs, or the planar _PLANAR_RGB8 / _PLANAR_BGR8 /
    /// _PLANAR_GBR8.  The frame source then hands out frames in that format; pages stay BGR.  The reference only ever sees
    /// OpenCV's BGR.
    pub pixel_format: i32,
    /// A per-channel tone table uint8 [3][256] (B, G, R; slideo_group_set_frame_levels) applied to every frame's analysed image as
    /// the last step in front of the pipeline: what ffi::slideo_frame_levels_lut makes of the points
    /// ffi::slideo_matcher_levels_points learnt from a dim, low-contrast or colour-cast recording.  Pages are untouched; None:
    /// off.  The reference analyses the frames as they are.
    pub frame_levels: Option<Box<[u8; 768]>>,
    /// (aw, ah, cell, gains): a bilinear Q8.8 gain field (slideo_group_set_frame_shading) over the aw x ah analysed image — uint16
    /// [gh + 1][gw + 1] nodes `cell` (16, 32 or 64) pixels apart, 256 = 1.0 — applied in front of frame_levels: what
    /// ffi::slideo_shading_field makes of per-cell sums, for the vignetting of a filmed projection screen.  Pages are untouched;
    /// None: off.
    pub frame_shading: Option<(i32, i32, i32, Vec<u16>)>,
    /// Which frame a gated frame is compared with (slideo_group_set_gate_reference): ffi::SLIDEO_GATE_PREVIOUS (default: the
    /// frame before, the reference's MarkSimilarIter) or ffi::SLIDEO_GATE_ANCHOR (the last frame that was flagged: a change
    /// spread over many frames is still flagged when every decoded frame is fed).  With several devices it needs
    /// group_gate_order = ffi::SLIDEO_GROUP_GATE_CHAIN: without it the group refuses SLIDEO_GATE_ANCHOR when it is built.
    pub gate_reference: u32,
    /// (settle_similarity, max_defer): the gate settle (slideo_group_set_gate_settle), under ffi::SLIDEO_GATE_ANCHOR only: a
    /// frame away from the last matched frame is matched once it is within settle_similarity of the frame before it, or after
    /// max_defer deferred frames; a deferred frame is reported as unchanged.  (0.0, 0): off, the default.
    pub gate_settle: (f32, i32),
    /// How a gated group call hands the gate state from device to device (slideo_group_set_gate_order), applied before
    /// gate_reference and gate_settle: ffi::SLIDEO_GROUP_GATE_HALO (default: a later device's shard is primed from one frame) or
    /// ffi::SLIDEO_GROUP_GATE_CHAIN (every shard receives the whole gate state of the shard before it, so the anchor reference
    /// and a settle run on any number of devices and return what one device returns).
    pub group_gate_order: u32,
    /// The gate memory's capacity (slideo_group_set_gate_memory), under ffi::SLIDEO_GATE_ANCHOR only, applied after
    /// gate_reference and gate_settle: the last `gate_memory` (1 ..= 64) matched frames are remembered and a frame that returns
    /// to one of them is recalled, not matched again; the task emits the remembered verdict at that frame's time.  One device
    /// only.  0: off, the default.
    pub gate_memory: i32,
}

/// The task's side of the gate memory (slideo_amd.h "Gate memory") behind a gate reset to "none": the verdicts of the matched
/// ordinals it remembers (at most `capacity`, the library's own ring), the next frame's ordinal and the last frame's ref.
pub struct GateMemory {
    pub verdicts: std::collections::BTreeMap<i64, ffi::slideo_verdict>,
    pub next: i64,
    pub prev_ref: i64,
    pub capacity: usize,
}

impl GateMemory {
    pub fn new(capacity: usize) -> Self {
        GateMemory { verdicts: std::collections::BTreeMap::new(), next: 0, prev_ref: i64::MIN, capacity }
    }
}

/// What one gated call emits under a gate memory: (index in the call, verdict), in order.  A matched frame emits its own verdict,
/// which is remembered under its ordinal; a frame that is not matched and whose ref >= 0 differs from the ref of the frame before
/// it (a recall, or the return to the anchor behind deferred frames) emits the verdict of the frame it stands behind.
pub fn gate_memory_emission(
    changed: &[u8],
    refs: &[i64],
    verdicts: &[ffi::slideo_verdict],
    memory: &mut GateMemory,
) -> Vec<(usize, ffi::slideo_verdict)> {
    let mut out = Vec::new();
    for i in 0..changed.len() {
        if changed[i] != 0 {
            memory.verdicts.insert(memory.next + i as i64, verdicts[i]);
            while memory.verdicts.len() > memory.capacity {
                let oldest = *memory.verdicts.keys().next().unwrap();
                memory.verdicts.remove(&oldest);
            }
            out.push((i, verdicts[i]));
        } else if refs[i] >= 0 && refs[i] != memory.prev_ref {
            if let Some(v) = memory.verdicts.get(&refs[i]) {
                out.push((i, *v));
            }
        }
        memory.prev_ref = refs[i];
    }
    memory.next += changed.len() as i64;
    out
}

impl HipImageVideoMatcher {
    /// Builder: the gate memory under the anchor reference (sets gate_reference to ffi::SLIDEO_GATE_ANCHOR when it switches one on).
    pub fn gate_memory(mut self, capacity: i32) -> Self {
        if capacity > 0 {
            self.gate_reference = ffi::SLIDEO_GATE_ANCHOR;
        }
        self.gate_memory = capacity;
        self
    }
    /// Builder: the gate settle under the anchor reference (sets gate_reference to ffi::SLIDEO_GATE_ANCHOR when it switches one on).
    pub fn gate_settle(mut self, settle_similarity: f32, max_defer: i32) -> Self {
        if settle_similarity > 0.0 {
            self.gate_reference = ffi::SLIDEO_GATE_ANCHOR;
        }
        self.gate_settle = (settle_similarity, max_defer);
        self
    }
    /// Builder: the group gate order (ffi::SLIDEO_GROUP_GATE_HALO / ffi::SLIDEO_GROUP_GATE_CHAIN).
    pub fn group_gate_order(mut self, order: u32) -> Self {
        self.group_gate_order = order;
        self
    }
}

impl Default for HipImageVideoMatcher {
    fn default() -> Self {
        HipImageVideoMatcher {
            devices: Vec::new(),
            sift_ratio: None,
            frame_mask: None,
            frame_mask_scope: ffi::SLIDEO_MASK_DETECT,
            direct_similarity: 0.0,
            direct_scope: ffi::SLIDEO_DIRECT_WHOLE,
            frame_region: None,
            frame_lens: None,
            yuv_description: (ffi::SLIDEO_YUV_MATRIX_BT601, ffi::SLIDEO_YUV_RANGE_LIMITED, ffi::SLIDEO_YUV_DEPTH_8),
            yuv_sampling: ffi::SLIDEO_YUV_SAMPLING_420,
            yuv_chroma: ffi::SLIDEO_YUV_CHROMA_NEAREST,
            yuv_transfer: (ffi::SLIDEO_YUV_TRANSFER_SDR, 0.0),
            pixel_format: ffi::SLIDEO_PIXEL_BGR8,
            frame_levels: None,
            frame_shading: None,
            gate_reference: ffi::SLIDEO_GATE_PREVIOUS,
            gate_settle: (0.0, 0),
            group_gate_order: ffi::SLIDEO_GROUP_GATE_HALO,
            gate_memory: 0,
        }
    }
}

impl<'i> ImageVideoMatcher<'i> for HipImageVideoMatcher {
    fn create_video_matcher<I: MatchableImage + Send + Sync + Copy + Eq + 'i>(
        &self,
        images: Vec<I>,
        progress_reporter: ProgressReporter,
    ) -> Box<dyn VideoMatcher<'i, I> + 'i> {
        ffi::assert_abi();
        let len = images.len() as u64;
        let mut cfg = std::mem::MaybeUninit::<ffi::slideo_config>::uninit();
        let mut h: *mut ffi::slideo_group = std::ptr::null_mut();
        // no explicit list: n_devices 0 = every gfx950 device of the node, enumerated by the library by its own HIP
        // ordinals (no device at all: create reports it)
        let devices_ptr = if self.devices.is_empty() { std::ptr::null() } else { self.devices.as_ptr() };
        unsafe {
            ffi::slideo_config_default(cfg.as_mut_ptr()); // the reference's literals (mo/feature_extractor.rs:13-23 etc.)
            check(
                std::ptr::null_mut(),
                ffi::slideo_group_create(cfg.as_ptr(), self.devices.len() as i32, devices_ptr, &mut h),
            );
            if self.group_gate_order != ffi::SLIDEO_GROUP_GATE_HALO {
                check(h, ffi::slideo_group_set_gate_order(h, self.group_gate_order));
            }
            if self.gate_reference != ffi::SLIDEO_GATE_PREVIOUS {
                check(h, ffi::slideo_group_set_gate_reference(h, self.gate_reference));
            }
            if self.gate_settle.0 != 0.0 {
                check(h, ffi::slideo_group_set_gate_settle(h, self.gate_settle.0, self.gate_settle.1));
            }
            if self.gate_memory != 0 {
                check(h, ffi::slideo_group_set_gate_memory(h, self.gate_memory));
            }
            if let Some(ratio) = self.sift_ratio {
                let mut sc = std::mem::MaybeUninit::<ffi::slideo_sift_config>::uninit();
                ffi::slideo_sift_config_default(sc.as_mut_ptr());
                check(h, ffi::slideo_group_use_sift(h, sc.as_ptr(), ratio));
            }
            if let Some((sw, sh, quad, ow, oh)) = &self.frame_region {
                let mut m9 = [0f64; 9];
                check(std::ptr::null_mut(), ffi::slideo_frame_region_from_quad(quad.as_ptr(), *ow, *oh, m9.as_mut_ptr()));
                check(h, ffi::slideo_group_set_frame_region(h, *sw, *sh, m9.as_ptr(), *ow, *oh));
            }
            if let Some((sw, sh, cx, cy, f, k1, k2)) = self.frame_lens {
                check(h, ffi::slideo_group_set_frame_lens(h, sw, sh, cx, cy, f, k1, k2));
            }
            if self.yuv_description != (0, 0, 0) {
                let (matrix, range, depth) = self.yuv_description;
                check(h, ffi::slideo_group_set_yuv_description(h, matrix, range, depth));
            }
            if self.yuv_sampling != ffi::SLIDEO_YUV_SAMPLING_420 {
                check(h, ffi::slideo_group_set_yuv_sampling(h, self.yuv_sampling));
            }
            if self.yuv_chroma != ffi::SLIDEO_YUV_CHROMA_NEAREST {
                check(h, ffi::slideo_group_set_yuv_chroma(h, self.yuv_chroma));
            }
            if self.yuv_transfer.0 != ffi::SLIDEO_YUV_TRANSFER_SDR {
                check(h, ffi::slideo_group_set_yuv_transfer(h, self.yuv_transfer.0, self.yuv_transfer.1));
            }
            if self.pixel_format != ffi::SLIDEO_PIXEL_BGR8 {
                check(h, ffi::slideo_group_set_pixel_format(h, self.pixel_format));
            }
            if let Some((aw, ah, cell, gains)) = &self.frame_shading {
                let nodes = ((*aw + *cell - 1) / *cell + 1) as usize * ((*ah + *cell - 1) / *cell + 1) as usize;
                assert_eq!(gains.len(), nodes, "frame_shading is not (gh + 1) x (gw + 1) gains");
                check(h, ffi::slideo_group_set_frame_shading(h, *aw, *ah, *cell, gains.as_ptr()));
            }
            if let Some(lut) = &self.frame_levels {
                check(h, ffi::slideo_group_set_frame_levels(h, lut.as_ptr()));
            }
            if self.frame_mask_scope != ffi::SLIDEO_MASK_DETECT {
                check(h, ffi::slideo_group_set_frame_mask_scope(h, self.frame_mask_scope));
            }
            if let Some((mask, w, hh)) = &self.frame_mask {
                assert_eq!(mask.len(), (*w as usize) * (*hh as usize), "frame_mask is not width x height bytes");
                check(h, ffi::slideo_group_set_frame_mask(h, mask.as_ptr(), *w, *hh, *w));
            }
            if self.direct_scope != ffi::SLIDEO_DIRECT_WHOLE {
                check(h, ffi::slideo_group_set_direct_scope(h, self.direct_scope));
            }
            if self.direct_similarity != 0.0 {
                check(h, ffi::slideo_group_set_direct_similarity(h, self.direct_similarity));
            }
        }
        // Page analysis (mo/lib.rs:43-58).  Pages are decoded on the host and handed over in groups, so that a 1000-page
        // deck does not sit decoded in memory at once; the progress protocol is the reference's and is driven from here
        // (slideo_group_set_progress — a C callback for callers without a reporter of their own — is not needed).
        progress_reporter.report(0, len, "Analyzing PDF pages...");
        let mut done = 0u64;
        let n_members = unsafe { ffi::slideo_group_device_count(h) }.max(1) as usize;
        for group in images.chunks(32 * n_members) {
            let decoded: Vec<decode::BgrImage> =
                group.iter().map(|i| decode::decode_page_bgr(i.get_path())).collect();
            let ptrs: Vec<*const u8> = decoded.iter().map(|d| d.data.as_ptr()).collect();
            let w: Vec<i32> = decoded.iter().map(|d| d.width).collect();
            let hh: Vec<i32> = decoded.iter().map(|d| d.height).collect();
            let stride: Vec<i32> = w.iter().map(|w| w * 3).collect();
            unsafe {
                check(
                    h,
                    ffi::slideo_group_add_pages_bgr8(
                        h,
                        ptrs.len() as i32,
                        ptrs.as_ptr(),
                        w.as_ptr(),
                        hh.as_ptr(),
                        stride.as_ptr(),
                    ),
                );
            }
            // one report per page, counting up (mo/lib.rs:49-53; the reference's come from rayon workers in any order)
            for _ in group {
                done += 1;
                progress_reporter.report(done, len, "Analyzing PDF pages...");
            }
        }
        unsafe { check(h, ffi::slideo_group_finalize_pages(h)) }; // FlannMatcher::new, mo/flann.rs:65-71
        progress_reporter.report(len, len, "PDF page analysis successful."); // mo/lib.rs:58
        Box::new(HipVideoMatcher {
            handle: Arc::new(Handle { raw: Mutex::new(RawHandle(h)) }),
            images: Arc::new(images),
            n_devices: n_members,
            gate_memory: self.gate_memory.max(0) as usize,
        })
    }
}

struct HipVideoMatcher<I> {
    handle: Arc<Handle>,
    images: Arc<Vec<I>>,
    n_devices: usize,
    gate_memory: usize,
}

impl<'i, I: MatchableImage + Send + Sync + Copy + Eq + 'i> VideoMatcher<'i, I> for HipVideoMatcher<I> {
    fn match_images_with_video(
        &self,
        video_path: &Path,
        progress_reporter: ProgressReporter,
    ) -> Box<dyn VideoMatcherTask<I> + 'i> {
        let interval = Duration::from_secs(5); // mo/lib.rs:145
        let vid = decode::sampled_video(video_path, interval);
        let total_time = vid.total_time();
        let frames_to_process = (total_time.as_secs_f64() / interval.as_secs_f64()) as u64; // mo/lib.rs:148
        progress_reporter.report(0, frames_to_process, ""); // mo/lib.rs:150
        Box::new(HipVideoMatcherTask {
            handle: self.handle.clone(),
            images: self.images.clone(),
            n_devices: self.n_devices,
            gate_memory: self.gate_memory,
            video_path: video_path.to_owned(),
            progress_reporter,
        })
    }
}

struct HipVideoMatcherTask<I> {
    handle: Arc<Handle>,
    images: Arc<Vec<I>>,
    n_devices: usize,
    gate_memory: usize,
    video_path: PathBuf,
    progress_reporter: ProgressReporter,
}

impl<I: MatchableImage + Send + Sync + Copy + Eq> VideoMatcherTask<I> for HipVideoMatcherTask<I> {
    fn process(&self) -> Vec<Matching<I>> {
        let interval = Duration::from_secs(5); // mo/lib.rs:175
        let vid = decode::sampled_video(&self.video_path, interval);
        let total_time = vid.total_time();
        let total_frames = vid.total_frames();
        let frames_to_process = (total_time.as_secs_f64() / interval.as_secs_f64()) as u32; // mo/lib.rs:179
        let message = format!(
            "Processing frames of '{}'...",
            self.video_path.file_name().unwrap().to_string_lossy()
        );

        // "Add a matching to indicate the last frame." (mo/lib.rs:185-189)
        let mut results: Vec<Matching<I>> = vec![Matching {
            image: None,
            video_frame_idx: total_frames as usize,
            video_time: total_time,
        }];

        let guard = self.handle.raw.lock().unwrap(); // one caller at a time on the handle
        let h = guard.0;
        let mut progress = 0u64;
        let mut prev_small: Option<Vec<u8>> = None;
        // The changed-frame gate (slideo_amd.h "Changed-frame gate"): the group's gated call, for any member count: one call per
        // batch decides on the devices which frames changed and matches those, every shard after the first primed from the frame
        // before its block; the last small image stays in the group.  CHANGED_GATE false: the stop-and-go mask + kept pair below.
        let gate = CHANGED_GATE;
        if gate {
            // the first frame of the video is always changed
            unsafe { check(h, ffi::slideo_group_gate_reset(h, std::ptr::null(), 0, 0)) };
        }
        let mut memory = GateMemory::new(self.gate_memory);
        // one call = one shard of FRAMES_PER_CALL_PER_DEVICE sampled frames per device (mo/lib.rs:213: one task per frame over the pool)
        for batch in decode::batches(vid, FRAMES_PER_CALL_PER_DEVICE * self.n_devices) {
            let n = batch.meta.len();
            let fb = batch.frame_bytes();
            // MarkSimilarIter (mo/video_capture.rs:86-98): changed <=> similarity to the previous SAMPLED frame < 0.98; the
            // first frame of the video is always changed (prev_small == None); the last small image of this call is the
            // `prev` of the next one.
            let mut changed = vec![0u8; n];
            if gate {
                let mut all = vec![ffi::slideo_verdict::default(); n];
                unsafe {
                    check(
                        h,
                        ffi::slideo_group_match_changed_frames_bgr8(
                            h,
                            n as i32,
                            batch.frames.as_ptr(),
                            batch.width,
                            batch.height,
                            batch.width * 3,
                            fb as i64,
                            changed.as_mut_ptr(),
                            std::ptr::null_mut(),
                            all.as_mut_ptr(),
                        ),
                    );
                }
                // under a gate memory a recalled frame has changed == 0 but shows another page than the frame before it: the
                // verdict of the frame it stands behind is emitted at its time (slideo_amd.h "Gate memory")
                let hits: Vec<(usize, ffi::slideo_verdict)> = if self.gate_memory > 0 {
                    let mut refs = vec![0i64; n];
                    let mut n_refs = 0i64;
                    unsafe { check(h, ffi::slideo_group_last_gate_refs(h, refs.as_mut_ptr(), n as i64, &mut n_refs)) };
                    assert_eq!(n_refs, n as i64, "slideo_group_last_gate_refs: the refs are not the call's");
                    gate_memory_emission(&changed, &refs, &all, &mut memory)
                } else {
                    (0..n).filter(|&i| changed[i] != 0).map(|i| (i, all[i])).collect()
                };
                for (i, v) in hits.iter() {
                    let (time, frame_idx) = batch.meta[*i];
                    results.push(Matching {
                        video_time: time,
                        video_frame_idx: frame_idx,
                        image: if v.page_idx >= 0 { Some(self.images[v.page_idx as usize]) } else { None },
                    });
                }
                for _ in 0..n {
                    progress += 1;
                    self.progress_reporter.report(progress, frames_to_process as u64, &message);
                }
                continue;
            }
            let mut last_small = vec![0u8; small_image_bytes(batch.width, batch.height)];
            unsafe {
                check(
                    h,
                    ffi::slideo_group_changed_mask_bgr8(
                        h,
                        n as i32,
                        batch.frames.as_ptr(),
                        batch.width,
                        batch.height,
                        batch.width * 3,
                        fb as i64,
                        prev_small.as_ref().map_or(std::ptr::null(), |p| p.as_ptr()),
                        last_small.as_mut_ptr(),
                        changed.as_mut_ptr(),
                        std::ptr::null_mut(),
                    ),
                );
            }
            // a change of frame size (never within one video file) restarts the comparison, as a fresh Mat size would
            // make compute_similarity panic in the reference
            prev_small = Some(last_small);

            // the changed frames through match_images_with_frame (mo/lib.rs:213-214): the mask call left every device's block
            // of the upload on that device, slideo_group_match_kept_frames matches a subset by index — no second copy over PCIe
            let sel: Vec<i32> = (0..n as i32).filter(|&i| changed[i as usize] != 0).collect();
            let mut verdicts = vec![ffi::slideo_verdict::default(); sel.len()];
            if !sel.is_empty() {
                unsafe {
                    check(
                        h,
                        ffi::slideo_group_match_kept_frames(h, sel.len() as i32, sel.as_ptr(), verdicts.as_mut_ptr()),
                    );
                }
            }
            for (&i, v) in sel.iter().zip(verdicts.iter()) {
                let (time, frame_idx) = batch.meta[i as usize];
                results.push(Matching {
                    video_time: time,
                    video_frame_idx: frame_idx,
                    image: if v.page_idx >= 0 { Some(self.images[v.page_idx as usize]) } else { None },
                });
            }
            // one report per sampled frame, changed or not (mo/lib.rs:191-212)
            for _ in 0..n {
                progress += 1;
                self.progress_reporter.report(progress, frames_to_process as u64, &message);
            }
        }
        drop(guard);

        self.progress_reporter.report(
            frames_to_process as u64,
            frames_to_process as u64,
            &format!("Finished!"),
        ); // mo/lib.rs:223-227

        timeline(results)
    }
}

/// The task's result as the application stores it (crates/app/src/db.rs:162-191): ordered by time, and a page (or "no page")
/// listed only where it CHANGES — the reference's sort + removal of consecutive duplicates, mo/lib.rs:229-244.  `sort_by_key`
/// is stable, so the end-of-video sentinel and equal-time entries keep their push order, as there.
fn timeline<I: Clone + Eq>(mut results: Vec<Matching<I>>) -> Vec<Matching<I>> {
    results.sort_by_key(|m| m.video_time);
    results.dedup_by(|next, kept| next.image == kept.image); // (Vec::dedup_by keeps the first of a run, drops the followers)
    results
}

/// to_small_image's output size (mo/image_utils.rs:8-20) times 3 channels: what slideo_changed_mask_bgr8 writes to
/// `last_small_out`.
fn small_image_bytes(width: i32, height: i32) -> usize {
    let max_area = 300 * 400;
    let factor = ((max_area as f32) / ((width * height) as f32)).sqrt();
    let sw = ((width as f32) * factor) as i32;
    let sh = ((height as f32) * factor) as i32;
    (sw as usize) * (sh as usize) * 3
}
