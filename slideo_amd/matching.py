"""Host-side mirror of the reference's `matching` trait surface over the C ABI.

Same names, argument meaning and behaviour as crates/matching/src/lib.rs:7-40 and
progress.rs:3-17, implemented over include/slideo_amd.h the way
crates/matching-opencv/src/lib.rs implements it over OpenCV:

    matcher = HipImageVideoMatcher()                       # OpenCVImageVideoMatcher::default()  main.rs:69
    vm   = matcher.create_video_matcher(pages, reporter)   # lib.rs:37-64
    task = vm.match_images_with_video(video_path, rep)     # lib.rs:140-158
    matchings = task.process()                             # lib.rs:168-246

The Rust toolchain is absent from this image, so this Python mirror is what the
tests drive; the Rust shim a maintainer would add is in INTEGRATION.md.  Video
DECODE is outside the hot path (north_star starts at decoded frames; the
reference uses FFmpeg inside OpenCV videoio): `video_path` names a raw frame
container (RawVideo below) or any object with the same reader interface.
"""
import os
import struct
from dataclasses import dataclass
from typing import Any, Callable, List, Optional

import numpy as np

from . import _capi


class ProgressReporter:
    """matching::ProgressReporter (crates/matching/src/progress.rs:3-17)."""

    def __init__(self, handler: Callable[[int, int, str], None]):
        self.handler = handler

    def report(self, processed_count: int, total_count: int, message: str):
        self.handler(processed_count, total_count, message)


@dataclass
class Matching:
    """matching::Matching<I> (crates/matching/src/lib.rs:35-40)."""
    video_time: float            # seconds (std::time::Duration)
    video_frame_idx: int
    image: Optional[Any]         # Option<I>


def _load_bgr(path):
    """imread of a page image -> 8UC3 BGR (the evident intent of lib.rs:98-104)."""
    from PIL import Image
    if not os.path.exists(path):
        raise FileNotFoundError("File '%s' must exist" % path)                 # lib.rs:95-97 (panic)
    return np.ascontiguousarray(np.array(Image.open(path).convert("RGB"))[:, :, ::-1])


class RawVideo:
    """Minimal raw BGR frame container standing in for the decoder (VideoCapture, video_capture.rs:16-40).

    Layout: b'SLVF' u32 width u32 height f64 fps u64 n_frames, then n_frames * h*w*3 bytes.
    """
    MAGIC = b"SLVF"
    HDR = struct.Struct("<4sIIdQ")

    def __init__(self, path):
        self.path = path
        with open(path, "rb") as f:
            magic, self.width, self.height, self.fps, self.n_frames = self.HDR.unpack(f.read(self.HDR.size))
        if magic != self.MAGIC:
            raise ValueError("not a raw frame container: %s" % path)
        self._frame_bytes = self.width * self.height * 3

    @staticmethod
    def write(path, frames, fps):
        frames = np.ascontiguousarray(frames, np.uint8)
        n, h, w, _ = frames.shape
        with open(path, "wb") as f:
            f.write(RawVideo.HDR.pack(RawVideo.MAGIC, w, h, float(fps), n))
            f.write(frames.tobytes())

    def total_frames(self):                      # CAP_PROP_FRAME_COUNT
        return float(self.n_frames)

    def total_time(self):                        # video_capture.rs:34-36
        return self.n_frames / self.fps

    def read(self, idx):
        with open(self.path, "rb") as f:
            f.seek(self.HDR.size + idx * self._frame_bytes)
            buf = f.read(self._frame_bytes)
        return np.frombuffer(buf, np.uint8).reshape(self.height, self.width, 3)


class RawVideoYuv420:
    """The same container for decoded YUV 4:2:0 frames, as a VCN or FFmpeg decoder hands them out (NV12 or I420, tightly packed).

    Layout: b'SLVY' u32 width u32 height f64 fps u64 n_frames u32 format (0 NV12, 2 I420: slideo_yuv420_layout_packed), then
    n_frames * w*h*3/2 bytes.  read() returns a frame's bytes (1-D); the task hands them to the *_yuv420 calls unconverted.
    """
    MAGIC = b"SLVY"
    HDR = struct.Struct("<4sIIdQI")
    FORMATS = {0: "nv12", 2: "i420"}

    def __init__(self, path):
        self.path = path
        with open(path, "rb") as f:
            magic, self.width, self.height, self.fps, self.n_frames, fmt = self.HDR.unpack(f.read(self.HDR.size))
        if magic != self.MAGIC or fmt not in self.FORMATS:
            raise ValueError("not a raw 4:2:0 frame container: %s" % path)
        self.yuv420_format = self.FORMATS[fmt]
        self._frame_bytes = self.width * self.height * 3 // 2

    @staticmethod
    def write(path, frames, width, height, fps, fmt="nv12"):
        """frames: uint8 [n, w*h*3/2] packed `fmt` frames."""
        code = {v: k for k, v in RawVideoYuv420.FORMATS.items()}[fmt]
        frames = np.ascontiguousarray(frames, np.uint8).reshape(-1, width * height * 3 // 2)
        with open(path, "wb") as f:
            f.write(RawVideoYuv420.HDR.pack(RawVideoYuv420.MAGIC, width, height, float(fps), frames.shape[0], code))
            f.write(frames.tobytes())

    def total_frames(self):
        return float(self.n_frames)

    def total_time(self):
        return self.n_frames / self.fps

    def read(self, idx):
        with open(self.path, "rb") as f:
            f.seek(self.HDR.size + idx * self._frame_bytes)
            buf = f.read(self._frame_bytes)
        return np.frombuffer(buf, np.uint8)


def open_raw_video(path):
    """RawVideo or RawVideoYuv420, by the container's magic."""
    with open(path, "rb") as f:
        magic = f.read(4)
    return RawVideoYuv420(path) if magic == RawVideoYuv420.MAGIC else RawVideo(path)


def sampled_frames(video, interval_s=5.0):
    """VideoCaptureIter (video_capture.rs:42-57): grab every frame, retrieve when
    frame_idx % floor(fps * interval) < 1; yields (frame, time_s, frame_idx)."""
    step = float(np.floor(video.fps * interval_s))
    if step <= 0:            # fps < 1 / interval: the reference's `frame_idx % 0.0` is NaN and `NaN < 1.0` is false — no frame is ever retrieved
        return
    for idx in range(int(video.n_frames)):
        if (idx % step) < 1.0:
            yield video.read(idx), idx / video.fps, idx


class HipVideoMatcherTask:
    """OpenCVVideoMatcherTask (lib.rs:161-246)."""

    def __init__(self, matcher, images, video, progress_reporter, batch=None, pages=None):
        self._m, self._images, self._video, self._rep = matcher, images, video, progress_reporter
        self._batch = batch or 64 * len(getattr(matcher, "devices", [0]))       # one shard of 64 sampled frames per device and call
        self._pages = pages          # deck indices of the images this task matches against (None: all of them)

    def process(self) -> List[Matching]:
        if self._pages is None:
            return self._process()
        # a page set of the task's images for the task's frame calls (include/slideo_amd.h "page sets"), released afterwards
        m = self._m
        set_id = m.create_page_set(self._pages)
        try:
            m.use_page_set(set_id)
            return self._process()
        finally:
            m.use_page_set(0)
            m.release_page_set(set_id)

    def _process(self) -> List[Matching]:
        video, m = self._video, self._m
        interval = 5.0
        total_time, total_frames = video.total_time(), video.total_frames()
        frames_to_process = int(total_time / interval)                                 # lib.rs:179
        results = [Matching(video_time=total_time, video_frame_idx=int(total_frames), image=None)]  # sentinel lib.rs:185-189
        name = os.path.basename(getattr(video, "path", "video"))
        progress = [0]

        def report_progress():
            progress[0] += 1
            self._rep.report(progress[0], frames_to_process, "Processing frames of '%s'..." % name)   # lib.rs:192-203

        pend_frames, pend_meta, prev_small = [], [], None
        yuv = getattr(video, "yuv420_format", None)              # RawVideoYuv420: 'nv12' / 'i420'; RawVideo: None (BGR)
        # the changed-frame gate (include/slideo_amd.h "Changed-frame gate"): one gated call per flush, the last small image carried
        # in the matcher (a group: in the group).  None (a handle without the gated calls): the mask + kept pair below.
        gate = _gated_matcher(m)
        if gate is not None:
            gate.gate_reset(None)                                # the first frame of the video is always changed
        capacity = gate.gate_memory() if gate is not None and hasattr(gate, "gate_memory") else 0
        memory = new_gate_memory(capacity) if capacity > 0 else None

        def emit(idx, verdicts):
            for j, v in zip(idx, verdicts):
                t, fi = pend_meta[j]
                img = self._images[v["page_idx"]] if v["page_idx"] >= 0 else None
                results.append(Matching(video_time=t, video_frame_idx=fi, image=img))

        def flush():
            nonlocal prev_small
            if not pend_frames:
                return
            # BGR frames are separate arrays: a library handle takes them as they are, as a frame list ("Frame lists"), without the
            # copy into one batch (_capi._FrameCalls._separate); YUV frames and other handles get the stacked batch
            stack = pend_frames[:] if not yuv and isinstance(m, _capi._FrameCalls) else np.stack(pend_frames)
            if gate is not None:                       # MarkSimilarIter + match_images_with_frame of the changed frames, one call
                if yuv:
                    changed, _, verdicts = gate.match_changed_frames_yuv420(stack, video.width, video.height, yuv)
                else:
                    changed, _, verdicts = gate.match_changed_frames(stack)
                if memory is not None:
                    # under a gate memory a recalled frame has changed == 0 but shows another page than the frame before it: the
                    # verdict of the frame it stands behind is emitted at its time
                    hits = gate_memory_emission(changed, gate.last_gate_refs(), verdicts, memory)
                    emit([j for j, _ in hits], [v for _, v in hits])
                else:
                    idx = np.nonzero(changed)[0]
                    emit(idx, verdicts[idx])
                for _ in pend_frames:
                    report_progress()
                pend_frames.clear(); pend_meta.clear()
                return
            if yuv:                                                                   # decoded 4:2:0 frames: converted on the GPU
                changed, _, prev_small = m.changed_mask_yuv420(stack, video.width, video.height, yuv, prev_small)
            else:
                changed, _, prev_small = m.changed_mask(stack, prev_small)           # MarkSimilarIter, video_capture.rs:86-98
            idx = np.nonzero(changed)[0]
            if len(idx):
                # match_images_with_frame, lib.rs:213-214 — on the copy of the frames the mask call left on the device
                if hasattr(m, "match_kept_frames"):
                    verdicts = m.match_kept_frames(idx)
                elif yuv:
                    verdicts = m.match_frames_yuv420(stack[idx], video.width, video.height, yuv)
                else:
                    verdicts = m.match_frames(np.stack(pend_frames)[idx])
                emit(idx, verdicts)
            for _ in pend_frames:
                report_progress()
            pend_frames.clear(); pend_meta.clear()

        for frame, t, fi in sampled_frames(video, interval):
            pend_frames.append(frame); pend_meta.append((t, fi))
            if len(pend_frames) >= self._batch:
                flush()
        flush()
        self._rep.report(frames_to_process, frames_to_process, "Finished!")           # lib.rs:223-227
        return dedup_timeline(results)


def new_gate_memory(capacity):
    """The task's side of the gate memory (include/slideo_amd.h "Gate memory") behind a gate reset to "none": the verdicts of the
    matched ordinals it remembers (at most `capacity`, the library's own ring), the next frame's ordinal and the last frame's ref."""
    return {"verdicts": {}, "next": 0, "prev_ref": None, "capacity": int(capacity)}


def gate_memory_emission(changed, refs, verdicts, memory):
    """What one gated call emits under a gate memory -> [(index in the call, verdict)], in order.  A matched frame (changed) emits
    its own verdict, which is remembered under its ordinal (the `capacity` most recent are kept).  A frame that is not matched and
    whose ref >= 0 differs from the ref of the frame before it — a recall, or the return to the anchor behind deferred frames —
    emits the verdict remembered for the frame it stands behind.  `memory` (new_gate_memory) carries on from call to call."""
    out = []
    known = memory["verdicts"]
    for i in range(len(changed)):
        ref = int(refs[i])
        if changed[i]:
            known[memory["next"] + i] = verdicts[i]
            for k in sorted(known)[:-memory["capacity"]]:
                del known[k]
            out.append((i, verdicts[i]))
        elif ref >= 0 and ref != memory["prev_ref"] and ref in known:
            out.append((i, known[ref]))
        memory["prev_ref"] = ref
    memory["next"] += len(changed)
    return out


def _gated_matcher(m):
    """The handle whose gated calls serve a task over `m`: m itself — a Matcher, or a Group of any member count (the group's gated
    call shards the frames and primes every later shard from the frame before its block) — or None for a handle without them."""
    return m if hasattr(m, "match_changed_frames") and hasattr(m, "gate_reset") else None


def learn_frame_mask(matcher, frame_batches, *, delta, max_share, grow):
    """A frame mask learnt from the frames' own motion (include/slideo_amd.h "Frame activity map"): the activity map of the host BGR
    batches (each uint8 [n, h, w, 3], in order: the last frame of a batch pairs with the first of the next), thresholded at
    `max_share` of the pairs and grown by `grow` pixels.  `matcher`: a Matcher (of a Group: its member 0), idle; neither pages nor
    finalize are needed.  Returns the mask, uint8 [ah, aw] of 0 / 255 at the analysed size — what frame_mask= takes; nothing is
    installed.  No value has a default: delta, max_share and grow depend on the content (docs/EXTENSIONS.md "Frame activity map")."""
    matcher.activity_begin(delta)
    try:
        for batch in frame_batches:
            matcher.observe_frames(batch)
        mask, _, _ = matcher.activity_mask(max_share, grow)
    finally:
        matcher.activity_end()
    return mask


def learn_frame_region(matcher, frame_batches, *, level, min_share, min_fill, inset=0, out_size=None):
    """A frame region learnt from letterbox bars (include/slideo_amd.h "Frame content box"): the content box of the host BGR batches
    (each uint8 [n, h, w, 3], all of one frame size) — a pixel is lit while max(B, G, R) > level, content while lit in more than
    `min_share` of the frames; a row or column is content while more than `min_fill` of it is —, shrunk by `inset` pixels on each
    side.  `matcher`: a Matcher (of a Group: its member 0), idle; neither pages nor finalize are needed.  Returns (src_w, src_h, quad,
    out_w, out_h) — what frame_region= and Matcher.set_frame_region take; quad: the box's corner pixel centres; out_size None: the
    box's own size, the exact crop.  Nothing is installed.  ValueError when the box is empty or narrower than 2 pixels after the
    inset, or when the frames were not analysed at their own size (a working size reduced them, or a frame region is set): the box
    is then not in source coordinates.  level, min_share and min_fill have no default: they depend on the content
    (docs/EXTENSIONS.md "Frame content box")."""
    inset = int(inset)
    if inset < 0:
        raise ValueError("learn_frame_region: inset %d is negative" % inset)
    size = None
    matcher.content_begin(level)
    try:
        for batch in frame_batches:
            if size is None and len(batch):
                size = (int(np.shape(batch)[2]), int(np.shape(batch)[1]))
            matcher.observe_frames(batch)
        info = matcher.content_info()
        box, _, _, _ = matcher.content_box(min_share, min_fill)
    finally:
        matcher.content_end()
    if (info["aw"], info["ah"]) != size:
        raise ValueError("learn_frame_region: the frames are %dx%d but were analysed at %dx%d (a working size reduced them, or a frame "
                         "region is set): the box is not in source coordinates" % (size + (info["aw"], info["ah"])))
    x0, y0, x1, y1 = box[0] + inset, box[1] + inset, box[2] - inset, box[3] - inset
    if x1 - x0 < 2 or y1 - y0 < 2:
        raise ValueError("learn_frame_region: the content box %s is empty or narrower than 2 pixels on a side after an inset of %d"
                         % (tuple(box), inset))
    out_w, out_h = (x1 - x0, y1 - y0) if out_size is None else (int(out_size[0]), int(out_size[1]))
    quad = [(float(x0), float(y0)), (float(x1 - 1), float(y0)), (float(x1 - 1), float(y1 - 1)), (float(x0), float(y1 - 1))]
    return size[0], size[1], quad, out_w, out_h


def _evidence_counts(matcher, frame_batches, cell, min_inliers):
    """The evidence counts of matching the host BGR batches with `matcher`: (seen, hit, info, frame size)."""
    size = None
    matcher.evidence_begin(cell, min_inliers)
    try:
        for batch in frame_batches:
            if size is None and len(batch):
                size = (int(np.shape(batch)[2]), int(np.shape(batch)[1]))
            matcher.match_frames(batch)
        info = matcher.evidence_info()
        seen, hit, _, _ = matcher.evidence_counts()
    finally:
        matcher.evidence_end()
    if info["aw"] == 0:
        raise ValueError("no frame was matched: the evidence map is empty")
    return seen, hit, info, size


def learn_frame_mask_from_matches(matcher, frame_batches, *, cell, min_inliers, min_seen, min_hit, grow):
    """A frame mask learnt from the matches themselves (include/slideo_amd.h "Match evidence map"): the host BGR batches (each uint8
    [n, h, w, 3], all of one frame size) are matched against the matcher's finalized deck under an evidence session of `cell` and
    `min_inliers`; a cell is clutter when at least `min_seen` keypoints of contributing frames fell into it and less than the share
    `min_hit` of them agreed with the winning page's transform; the other cells, grown by `grow` cells, are kept.  `matcher`: a
    Matcher or a Group, idle, finalized.  Returns the mask, uint8 [ah, aw] of 0 / 255 at the analysed size — what frame_mask= and
    set_frame_mask take; nothing is installed.  No value has a default: they depend on the content (docs/EXTENSIONS.md "Match
    evidence map")."""
    seen, hit, info, _ = _evidence_counts(matcher, frame_batches, cell, min_inliers)
    return _capi.evidence_mask(seen, hit, info["cell"], info["aw"], info["ah"], min_seen, min_hit, grow)


def learn_frame_box_from_matches(matcher, frame_batches, *, cell, min_inliers, min_hits, min_hit, inset=0, out_size=None):
    """A frame region learnt from the matches themselves ("Match evidence map"): the bounding box of the cells into which at least
    `min_hits` keypoints fell that agreed with the winning page's transform, and at least the share `min_hit` of the cell's
    keypoints did, shrunk by `inset` pixels on each side.  Frames and `matcher` as learn_frame_mask_from_matches.  Returns what
    learn_frame_region returns — (src_w, src_h, quad, out_w, out_h), quad: the box's corner pixel centres; out_size None: the box's
    own size, the exact crop — and installs nothing.  ValueError when no cell qualifies, when the box is narrower than 2 pixels
    after the inset, or when the frames were not analysed at their own size (a working size reduced them, or a frame region is set):
    the box is then not in source coordinates.  cell, min_inliers, min_hits and min_hit have no default."""
    inset = int(inset)
    if inset < 0:
        raise ValueError("learn_frame_box_from_matches: inset %d is negative" % inset)
    seen, hit, info, size = _evidence_counts(matcher, frame_batches, cell, min_inliers)
    if (info["aw"], info["ah"]) != size:
        raise ValueError("learn_frame_box_from_matches: the frames are %dx%d but were analysed at %dx%d (a working size reduced them, or a "
                         "frame region is set): the box is not in source coordinates" % (size + (info["aw"], info["ah"])))
    box = _capi.evidence_box(seen, hit, info["cell"], info["aw"], info["ah"], min_hits, min_hit)
    x0, y0, x1, y1 = box[0] + inset, box[1] + inset, box[2] - inset, box[3] - inset
    if box[0] < 0 or x1 - x0 < 2 or y1 - y0 < 2:
        raise ValueError("learn_frame_box_from_matches: the evidence box %s is empty or narrower than 2 pixels on a side after an inset of %d"
                         % (tuple(box), inset))
    out_w, out_h = (x1 - x0, y1 - y0) if out_size is None else (int(out_size[0]), int(out_size[1]))
    quad = [(float(x0), float(y0)), (float(x1 - 1), float(y0)), (float(x1 - 1), float(y1 - 1)), (float(x0), float(y1 - 1))]
    return size[0], size[1], quad, out_w, out_h


def learn_frame_levels(matcher, frame_batches, low=0.01, high=0.01):
    """A frame levels table learnt from the frames' own histogram (include/slideo_amd.h "Frame levels"): the per-channel histogram of
    the host BGR batches (each uint8 [n, h, w, 3], or the array shape of the pixel format in force; any sizes), cut by the share `low`
    at the dark end and `high` at the bright end of every channel, and the linear stretch between the two points.  `matcher`: a
    Matcher (of a Group: its member 0), idle; neither pages nor finalize are needed.  Returns the table uint8 [3, 256] (B, G, R) — what
    frame_levels= and set_frame_levels take; nothing is installed.  ValueError while a table is set (a table learnt on levelled
    frames is not the source's), or when a channel's points coincide (a constant picture has no stretch)."""
    if matcher.frame_levels() is not None:
        raise ValueError("learn_frame_levels: a frame levels table is set, and a table learnt on levelled frames is not the source's "
                         "(set_frame_levels(None) first)")
    matcher.levels_begin()
    try:
        for batch in frame_batches:
            matcher.observe_frames(batch)
        lo, hi = matcher.levels_points(low, high)
    finally:
        matcher.levels_end()
    return _capi.frame_levels_lut(lo, hi)


def learn_frame_levels_from_matches(matcher, frame_batches, *, min_inliers, min_hits, flat=255, min_count):
    """A frame levels table learnt from the matches themselves (include/slideo_amd.h "Match tone table"): the host BGR batches (each
    uint8 [n, h, w, 3]) are matched against the matcher's finalized deck under a tone session of `min_inliers`, `min_hits` and
    `flat`; per channel, the mean page value of the samples of every frame value seen at least `min_count` times, made monotone
    and interpolated (slideo_tone_lut).  `matcher`: a Matcher or a Group, idle, finalized.  Returns the table uint8 [3, 256]
    (B, G, R) — what frame_levels= and set_frame_levels take; nothing is installed.  While the matcher carries a levels table T1
    the samples are the levelled image's, and what is returned is the COMPOSITION lut[c][T1[c][x]]: the table for the frames as
    they come, to be set in T1's place.  ValueError when no frame contributed.  min_inliers, min_hits and min_count have no default:
    they depend on the content (docs/EXTENSIONS.md "Match tone table")."""
    t1 = matcher.frame_levels()
    matcher.tone_begin(min_inliers, min_hits, flat)
    try:
        for batch in frame_batches:
            matcher.match_frames(batch)
        cnt, sm, through, counted = matcher.tone_counts()
    finally:
        matcher.tone_end()
    if counted == 0:
        raise ValueError("learn_frame_levels_from_matches: none of the %d frames contributed (no candidate with a model, %d inliers and "
                         "%d hits): the tone table is empty" % (through, int(min_inliers), int(min_hits)))
    lut = _capi.tone_lut(cnt, sm, min_count)
    if t1 is not None:
        lut = np.stack([lut[c][t1[c]] for c in range(3)])
    return lut


def learn_frame_shading_from_matches(matcher, frame_batches, *, cell, min_inliers, min_hits, flat, min_count, min_gain, max_gain, smooth):
    """A frame shading learnt from the matches themselves (include/slideo_amd.h "Match shading map"): the host BGR batches (each uint8
    [n, h, w, 3], all of one frame size) are matched against the matcher's finalized deck under a shading session of `cell`,
    `min_inliers`, `min_hits` and `flat`; every cell with at least `min_count` samples gives the ratio of its page side's sum to its
    frame side's, and slideo_shading_field fills, smooths (`smooth` rounds) and clamps them to min_gain .. max_gain (Q8.8 integers,
    256 = 1.0) on the grid's nodes.  `matcher`: a Matcher or a Group, idle, finalized, with neither a frame shading nor a frame levels
    table set (learn the field first and the table second); the camera and the screen must not move over the batches.  Returns
    (aw, ah, cell, gains uint16 [gh + 1, gw + 1]) — what frame_shading= and set_frame_shading(*result) take; nothing is installed.
    ValueError when no frame contributed.  No parameter has a default: they depend on the content (docs/EXTENSIONS.md "Match shading
    map")."""
    matcher.shading_begin(cell, min_inliers, min_hits, flat)
    try:
        for batch in frame_batches:
            matcher.match_frames(batch)
        info = matcher.shading_info()
        sums, through, counted = matcher.shading_sums()
    finally:
        matcher.shading_end()
    if counted == 0:
        raise ValueError("learn_frame_shading_from_matches: none of the %d frames contributed (no candidate with a model, %d inliers and "
                         "%d hits): the shading map is empty" % (through, int(min_inliers), int(min_hits)))
    gains, _ = _capi.shading_field(sums[0], sums[1], sums[2], cell, min_count, min_gain, max_gain, smooth)
    return info["aw"], info["ah"], int(cell), gains


def learn_frame_quad_from_matches(matcher, frame_batches, *, cell, min_inliers, reach, min_count, trim, rounds, inset=0, out_size=None):
    """A keystoned frame region learnt from the matches themselves (include/slideo_amd.h "Match placement map"): the host BGR batches
    (each uint8 [n, h, w, 3], all of one frame size) are matched against the matcher's finalized deck under a placement session of
    `cell`, `min_inliers` and `reach`; every cell with at least `min_count` explained keypoints is one correspondence between the
    unit slide and the frame, and slideo_placement_quad fits the homography to them, dropping cells further than `trim` pixels
    from it at most `rounds` times.  `matcher`: a Matcher or a Group, idle, finalized; the camera and the screen must not move over
    the batches.  Returns what learn_frame_region returns — (src_w, src_h, quad, out_w, out_h), quad: where the slide's corner
    pixel centres lie in the frame, top-left, top-right, bottom-right, bottom-left — and installs nothing.  inset: the slide's
    corners are taken `inset` pixels inside the slide on every side (measured along the quad's mean edge lengths, mapped through
    the fitted homography).  out_size None: the rounded mean lengths of the quad's opposite edge pairs, at least 2.  ValueError when
    no frame was matched, or when the frames were not analysed at their own size (a working size reduced them, or a frame region is
    set): the quad is then not in source coordinates; SlideoError when the cells determine no quad.  No threshold has a default."""
    inset = float(inset)
    if inset < 0:
        raise ValueError("learn_frame_quad_from_matches: inset %g is negative" % inset)
    size = None
    matcher.placement_begin(cell, min_inliers, reach)
    try:
        for batch in frame_batches:
            if size is None and len(batch):
                size = (int(np.shape(batch)[2]), int(np.shape(batch)[1]))
            matcher.match_frames(batch)
        info = matcher.placement_info()
        sums, _, _ = matcher.placement_sums()
    finally:
        matcher.placement_end()
    if info["aw"] == 0:
        raise ValueError("no frame was matched: the placement map is empty")
    if (info["aw"], info["ah"]) != size:
        raise ValueError("learn_frame_quad_from_matches: the frames are %dx%d but were analysed at %dx%d (a working size reduced them, or a "
                         "frame region is set): the quad is not in source coordinates" % (size + (info["aw"], info["ah"])))
    quad, H, _, _ = _capi.placement_quad(sums, info["cell"], info["aw"], info["ah"], min_count, trim, rounds)

    def edges(q):
        d = lambda a, b: float(np.hypot(q[a][0] - q[b][0], q[a][1] - q[b][1]))
        return (d(0, 1) + d(3, 2)) / 2, (d(0, 3) + d(1, 2)) / 2
    if inset > 0:
        ew, eh = edges(quad)
        if not (2 * inset < ew and 2 * inset < eh):
            raise ValueError("learn_frame_quad_from_matches: an inset of %g leaves nothing of a quad of mean edges %.1f x %.1f" % (inset, ew, eh))
        s = float(max(info["aw"], info["ah"]))
        eu, ev = inset / ew, inset / eh
        quad = []
        for u, v in ((eu, ev), (1 - eu, ev), (1 - eu, 1 - ev), (eu, 1 - ev)):
            p = H @ np.array([u, v, 1.0])
            quad.append((float(s * p[0] / p[2]), float(s * p[1] / p[2])))
    if out_size is None:
        ew, eh = edges(quad)
        out_w, out_h = max(2, int(round(ew))), max(2, int(round(eh)))
    else:
        out_w, out_h = int(out_size[0]), int(out_size[1])
    return size[0], size[1], quad, out_w, out_h


def learn_frame_lens_from_matches(matcher, frame_batches, *, cell, min_inliers, reach, min_count, trim_px, rounds, order, centre=None, f=None):
    """A frame lens and the quad beside it, learnt jointly from the matches (include/slideo_amd.h "Placement lens"): the host BGR
    batches (each uint8 [n, h, w, 3], all of one frame size) are matched against the matcher's finalized deck under a placement
    session of `cell`, `min_inliers` and `reach`, with NO lens and NO region set; slideo_placement_lens fits a homography and the
    radial terms k1 (order 1) or k1 and k2 (order 2) to the cells with at least `min_count` explained keypoints, dropping cells
    further than `trim_px` from the joint fit at most `rounds` times.  `matcher`: a Matcher or a Group, idle, finalized; camera and
    screen must not move over the batches.  centre None: the image centre ((aw - 1) / 2, (ah - 1) / 2); f None: half the diagonal.
    Returns (frame_lens, quad): frame_lens = (src_w, src_h, cx, cy, f, k1, k2), what frame_lens= and set_frame_lens(*frame_lens)
    take; quad: the slide's corners in IDEAL coordinates, top-left, top-right, bottom-right, bottom-left — what a frame region takes
    while that lens is set.  Nothing is installed.  ValueError when no frame was matched, when a lens or a region is set, or when a
    working size reduced the frames; SlideoError when the cells determine no fit.  No threshold has a default."""
    if matcher.frame_lens is not None or matcher.frame_region is not None:
        raise ValueError("learn_frame_lens_from_matches: a frame lens or a frame region is set: the sums are then not the source's")
    size = None
    matcher.placement_begin(cell, min_inliers, reach)
    try:
        for batch in frame_batches:
            if size is None and len(batch):
                size = (int(np.shape(batch)[2]), int(np.shape(batch)[1]))
            matcher.match_frames(batch)
        info = matcher.placement_info()
        sums, _, _ = matcher.placement_sums()
    finally:
        matcher.placement_end()
    if info["aw"] == 0:
        raise ValueError("no frame was matched: the placement map is empty")
    if (info["aw"], info["ah"]) != size:
        raise ValueError("learn_frame_lens_from_matches: the frames are %dx%d but were analysed at %dx%d (a working size reduced them): the "
                         "fit is not in source coordinates" % (size + (info["aw"], info["ah"])))
    cx, cy, f = _capi.frame_lens_defaults(size[0], size[1], None if centre is None else centre[0], None if centre is None else centre[1], f)
    k, quad, _, _, _ = _capi.placement_lens(sums, info["cell"], info["aw"], info["ah"], min_count, cx, cy, f, order, trim_px, rounds,
                                            LENS_FIT_ITERS)
    return (size[0], size[1], cx, cy, f, k[0], k[1]), quad


# the damped Gauss-Newton steps learn_frame_lens_from_matches allows a run of the iteration (it stops on its own rule long before)
LENS_FIT_ITERS = 100


def dedup_timeline(mappings: List[Matching]) -> List[Matching]:
    """lib.rs:229-244: stable sort by time, drop consecutive mappings with the same image."""
    mappings = sorted(mappings, key=lambda mm: mm.video_time)
    cleaned, last = [], None
    for mm in mappings:
        if last is not None and _same_image(last.image, mm.image):
            continue
        last = mm
        cleaned.append(mm)
    return cleaned


def _same_image(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a == b


class HipVideoMatcher:
    """OpenCVVideoMatcher (lib.rs:134-158): owns the page-derived state shared by every task."""

    def __init__(self, matcher, images):
        self._m, self._images = matcher, images

    def match_images_with_video(self, video_path, progress_reporter: ProgressReporter, images=None) -> HipVideoMatcherTask:
        """images (an extension): a subset of the images this matcher was created with.  The task then matches the video against
        those pages only, on a page set of the one page analysis (the upstream README's "lecture1 <-> video1, lecture2 <-> video2",
        without a second matcher), and every Matching.image it returns is one of them.  None: every image, as upstream."""
        pages = None if images is None else self._page_indices(images)
        video = open_raw_video(video_path) if isinstance(video_path, (str, os.PathLike)) else video_path
        frames_to_process = int(video.total_time() / 5.0)                             # lib.rs:148
        progress_reporter.report(0, frames_to_process, "")                            # lib.rs:150
        return HipVideoMatcherTask(self._m, self._images, video, progress_reporter, pages=pages)

    def _page_indices(self, images):
        """Deck indices of `images` (each one of the matcher's images: the same object, or an equal one), ascending."""
        idx = set()
        for im in images:
            hit = next((i for i, own in enumerate(self._images) if own is im), None)
            if hit is None:
                hit = next((i for i, own in enumerate(self._images) if own == im), None)
            if hit is None:
                raise ValueError("image %r is not one this video matcher was created with" % (im,))
            idx.add(hit)
        if not idx:
            raise ValueError("images: at least one image is needed")
        return sorted(idx)


class HipImageVideoMatcher:
    """Drop-in for OpenCVImageVideoMatcher (lib.rs:34-73) behind matching::ImageVideoMatcher."""

    def __init__(self, cfg=None, device=None, sift=None, devices=None, working_size=None, frame_mask=None, frame_mask_scope=None,
                 direct_similarity=None, direct_scope=None, frame_region=None, yuv_description=None, gate_reference=None, gate_settle=None,
                 group_gate_order=None, yuv_sampling=None, gate_memory=None, pixel_format=None, frame_levels=None, frame_shading=None, yuv_chroma=None,
                 yuv_transfer=None, frame_lens=None):
        """devices: HIP ordinals, one matcher each behind one slideo_group (the reference fans out over the whole machine, the
        global rayon pool of lib.rs:45,174); None = every gfx950 device of the node; `device` = d is short for devices = [d].
        sift = (slideo_sift_config, ratio): the north-star's SIFT + L2 front end instead of the reference's ORB + Hamming
        (slideo_group_use_sift; ratio 0 = the path's own tolerance vote, > 0 = Lowe's ratio test); None = the reference's.
        working_size = (max_w, max_h): frames beyond it are reduced on the GPU before matching (slideo_group_set_working_size;
        the reference never reduces a frame: verdicts are then those of the reduced video); None = frames as they arrive.
        frame_mask = uint8 [h, w], nonzero = detect here: ORB keypoints of the frames are detected under it (slideo_group_set_frame_mask;
        a speaker inset, a logo or subtitles stay out of the features; detection only; the frames' analysed size must be the
        mask's; the reference passes no mask); None = no mask.
        frame_mask_scope = _capi.MASK_DETECT | _capi.MASK_GATE bits (slideo_group_set_frame_mask_scope): with MASK_GATE the
        changed-frame gate ignores the masked regions too, so that an inset which moves on every frame does not flag every held
        slide as changed; None = the default, MASK_DETECT.
        direct_similarity = t in (0, 1] (slideo_group_set_direct_similarity): a changed frame whose small image is at least that
        similar to a page's is resolved to that page without ORB, search or verify — full-screen slide frames of a screen
        recording (the reference never decides without keypoints); not together with MASK_GATE unless direct_scope says so;
        None = off.
        direct_scope = _capi.DIRECT_WHOLE or _capi.DIRECT_VALID (slideo_group_set_direct_scope): with DIRECT_VALID the look-up
        compares what the gate compares, the valid pixels of the gate's validity map, so MASK_GATE and direct_similarity work
        together (a full-screen slide under a speaker thumbnail); applied before direct_similarity; None = DIRECT_WHOLE.
        frame_region = (src_w, src_h, M_or_quad, out_w, out_h) (slideo_group_set_frame_region): frames of src_w x src_h stand for
        the out_w x out_h image rectified from a fixed quadrilateral of them — a filmed projection screen, a slide in a
        sub-window; M_or_quad: the 3x3 map from the rectified image into the frame, or the slide's four corners in the frame
        (top-left, top-right, bottom-right, bottom-left); a frame mask is then of the output size, and the output must fit a
        working size (the reference analyses the whole frame); None = no region.
        frame_lens = (src_w, src_h, cx, cy, f, k1, k2) (slideo_group_set_frame_lens): the radial distortion of a wide-angle room
        camera, c + (p - c) (1 + k1 r2 + k2 r2^2) with r2 = |p - c|^2 / f^2, removed in the same launch that rectifies — what
        learn_frame_lens_from_matches returns; a frame_region's quad is then given in ideal (undistorted) coordinates; applied
        after frame_region; the reference analyses the frame as the camera saw it; None = no lens.
        yuv_description = (matrix, range) or (matrix, range, depth), as Matcher.set_yuv_description takes them
        (slideo_group_set_yuv_description): how the YUV 4:2:0 videos are read — ("bt709", "limited") for HD recordings,
        ("bt709", "full") for many screen recorders; the reference reads every stream as BT.601 limited range; RawVideoYuv420
        files hold 8-bit samples, so depth stays 8 for them; None = BT.601 limited, 8-bit.
        yuv_sampling = "420" | "422" | "444" | "422_packed" (slideo_group_set_yuv_sampling): where the frames' samples lie — 4:4:4
        for screen recorders, 4:2:2 for ProRes / broadcast recorders, packed 4:2:2 (YUY2, UYVY) for capture cards; every call that
        takes a layout then reads its frames under it; the reference knows BGR only; None = 4:2:0.
        yuv_chroma = "nearest" | "left" | "center" | "topleft" (slideo_group_set_yuv_chroma): how a pixel's chroma is read from 4:2:0
        and 4:2:2 frames — "left" is the bilinear filter at the siting of H.264 / HEVC / MPEG-2 streams, "center" JPEG's and MPEG-1's,
        "topleft" BT.2020's; cvtColor and the reference's swscale path take the nearest sample; None = nearest.
        yuv_transfer = ("hlg" | "pq" | "sdr", white_nits) or the name alone (slideo_group_set_yuv_transfer): HDR frames — HLG / BT.2020
        of phones, PQ / BT.2020 of HDR screen recorders and capture — are converted to SDR on the GPU: full 10-bit samples, the
        BT.2020 matrix, linear light with white_nits (0 = 203) as SDR white, BT.2020 -> BT.709, sRGB; needs a 10-bit yuv_description;
        the reference knows no HDR; None = SDR.
        pixel_format = "bgr" | "rgb" | "bgra" | "rgba" | "argb" | "abgr" | "planar_rgb" | "planar_bgr" | "planar_gbr"
        (slideo_group_set_pixel_format): how the frames of the BGR door are read.  The frame source then yields frames in that
        format — [h, w, 3], [h, w, 4] or [3, h, w] — and no swizzle pass runs on the host; page images stay BGR; the reference only
        ever sees OpenCV's BGR; None = "bgr".
        frame_levels = uint8 [3, 256] (B, G, R; slideo_group_set_frame_levels): a per-channel tone table applied to every frame's
        analysed image as the last step in front of the pipeline — what learn_frame_levels returns for dim, low-contrast or
        colour-cast recordings; pages are untouched; the reference analyses the frames as they are; None = off.
        frame_shading = (aw, ah, cell, gains uint16 [gh + 1, gw + 1]) (slideo_group_set_frame_shading): a bilinear Q8.8 gain field
        over the aw x ah analysed image, applied in front of frame_levels — for the vignetting and gradients of a filmed projection
        screen, which one table per channel cannot undo; pages are untouched; frames analysed at another size are refused; None = off.
        gate_reference = "previous" or "anchor" (slideo_group_set_gate_reference): with "anchor" a frame is compared with the last
        frame that was flagged, not the frame before it, so a change spread over many frames (a cross-fade, an animated build) is
        still flagged when every decoded frame is fed; with several devices it needs group_gate_order = "chain" — without it the
        group refuses it here, when it is built (SLIDEO_ERR_UNSUPPORTED); None = "previous", the reference's MarkSimilarIter.
        gate_settle = (similarity, max_defer) (slideo_group_set_gate_settle), under gate_reference "anchor" only: a frame away
        from the last matched frame is matched once it is within `similarity` of the frame before it — the picture stands
        still — or after max_defer deferred frames, so a cross-fade costs one verdict, not one for every second frame of it; a
        deferred frame is reported as unchanged; None = off.
        gate_memory = M in 1 .. 64 (slideo_group_set_gate_memory), under gate_reference "anchor" only, applied after gate_reference
        and gate_settle: the last M matched frames are remembered, and a frame that returns to one of them — a cut back to the
        slide, a flip back — is recalled instead of matched again; the task then emits the remembered verdict at that frame's time
        (gate_memory_emission).  One device only; None or 0 = off.
        group_gate_order = "halo" or "chain" (slideo_group_set_gate_order), applied before gate_reference and gate_settle: with
        "chain" every device's shard of a gated call receives the whole gate state of the shard before it, so "anchor" and a
        settle run on any number of devices and return what one device returns; None = "halo", a shard primed from one frame."""
        self._cfg, self._sift = cfg, sift
        self._working_size = working_size
        self._frame_mask = frame_mask
        self._frame_mask_scope = frame_mask_scope
        self._direct_similarity = direct_similarity
        self._direct_scope = direct_scope
        self._frame_region = frame_region
        self._frame_lens = tuple(frame_lens) if frame_lens is not None else None
        self._yuv_description = tuple(yuv_description) if yuv_description is not None else None
        self._yuv_sampling = yuv_sampling
        self._yuv_chroma = yuv_chroma
        self._yuv_transfer = (yuv_transfer, 0) if isinstance(yuv_transfer, (str, int)) else tuple(yuv_transfer) if yuv_transfer is not None else None
        self._pixel_format = pixel_format
        self._frame_levels = frame_levels
        self._frame_shading = tuple(frame_shading) if frame_shading is not None else None
        self._gate_reference = gate_reference
        self._gate_settle = tuple(gate_settle) if gate_settle is not None else None
        self._gate_memory = gate_memory
        self._group_gate_order = group_gate_order
        self._devices = [device] if device is not None else devices

    def create_video_matcher(self, images, progress_reporter: ProgressReporter) -> HipVideoMatcher:
        """images: objects with get_path() (matching::MatchableImage, lib.rs:31-33)."""
        images = list(images)
        m = _capi.Group(self._cfg, self._devices)
        if self._group_gate_order is not None:
            m.set_gate_order(self._group_gate_order)
        if self._gate_reference is not None:
            m.set_gate_reference(self._gate_reference)
        if self._gate_settle is not None:
            m.set_gate_settle(*self._gate_settle)
        if self._gate_memory is not None:
            m.set_gate_memory(self._gate_memory)
        if self._sift is not None:
            m.use_sift(*self._sift)
        if self._working_size is not None:
            m.set_working_size(*self._working_size)
        if self._frame_region is not None:
            m.set_frame_region(*self._frame_region)
        if self._frame_lens is not None:
            m.set_frame_lens(*self._frame_lens)
        if self._yuv_description is not None:
            m.set_yuv_description(*self._yuv_description)
        if self._yuv_sampling is not None:
            m.set_yuv_sampling(self._yuv_sampling)
        if self._yuv_chroma is not None:
            m.set_yuv_chroma(self._yuv_chroma)
        if self._yuv_transfer is not None:
            m.set_yuv_transfer(*self._yuv_transfer)
        if self._pixel_format is not None:
            m.set_pixel_format(self._pixel_format)
        if self._frame_shading is not None:
            m.set_frame_shading(*self._frame_shading)
        if self._frame_levels is not None:
            m.set_frame_levels(self._frame_levels)
        if self._frame_mask_scope is not None:
            m.set_frame_mask_scope(self._frame_mask_scope)
        if self._frame_mask is not None:
            m.set_frame_mask(self._frame_mask)
        if self._direct_scope is not None:
            m.set_direct_scope(self._direct_scope)
        if self._direct_similarity is not None:
            m.set_direct_similarity(self._direct_similarity)
        m.set_progress(progress_reporter.report)        # "Analyzing PDF pages..." protocol, lib.rs:43-58
        CH = 32 * len(m.devices)
        for i in range(0, len(images), CH):
            m.add_pages([_load_bgr(str(im.get_path())) for im in images[i:i + CH]])
        if not images:
            progress_reporter.report(0, 0, "Analyzing PDF pages...")
            progress_reporter.report(0, 0, "PDF page analysis successful.")
        m.set_progress(None)
        m.finalize()                                    # FlannMatcher::new, flann.rs:65-71 (raises on an empty index)
        return HipVideoMatcher(m, images)
