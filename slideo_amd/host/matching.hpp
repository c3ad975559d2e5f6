// matching.hpp — C++ host-side mirror of the reference's `matching` trait surface over the C ABI.
//
// The reference is compiled code (Rust); its toolchain is absent from this image, so the compiled host side
// above include/slideo_amd.h is C++.  Same names, argument meaning and behaviour as
// crates/matching/src/lib.rs:7-40 and progress.rs:3-17, implemented the way
// crates/matching-opencv/src/lib.rs implements them over OpenCV (cited below as mo/lib.rs:<line>).
//
//   HipImageVideoMatcher matcher;                                   // OpenCVImageVideoMatcher::default()   main.rs:69
//   auto vm   = matcher.create_video_matcher(pages, reporter);      // mo/lib.rs:37-64
//   auto task = vm->match_images_with_video(video_path, reporter);  // mo/lib.rs:140-158
//   auto out  = task->process();                                    // mo/lib.rs:168-246
//
// Errors: the reference panics (unwrap()/panic! throughout); here every non-zero status of the C ABI throws
// std::runtime_error.  Video decode and PNG decode are outside the hot path: frames come from a raw
// container (RawVideo), page images through a caller-supplied loader (default: binary PPM "P6").
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <filesystem>
#include <fstream>
#include <functional>
#include <map>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

#include "slideo_amd.h"
#include "png.hpp"

namespace slideo_host {

// matching::ProgressReporter (crates/matching/src/progress.rs:3-17)
class ProgressReporter {
public:
    using Handler = std::function<void(uint64_t, uint64_t, const std::string&)>;
    explicit ProgressReporter(Handler h = nullptr) : handler_(std::move(h)) {}
    void report(uint64_t processed_count, uint64_t total_count, const std::string& message) const {
        if (handler_) handler_(processed_count, total_count, message);
    }
private:
    Handler handler_;
};

// matching::Matching<I> (crates/matching/src/lib.rs:35-40)
// ---- timeline output contract of crates/app -----------------------------------------
// videos_mapping rows (db.rs:162-191) and PdfVideoMatching records (db.rs:194-201, 209-260); host logic only.
struct VideoMappingRow { uint32_t video_ms; bool has_pdf; std::string pdf_hash; uint32_t page; };
struct PdfVideoMatching { uint32_t video_offset_ms; std::string pdf_hash, video_hash; uint32_t page_idx, duration_ms; };

// I must expose .pdf_hash (std::string) and .page_nr (1-based), like PdfPage (pdf_to_images.rs:19-31)
template <class MatchingT>
inline std::vector<VideoMappingRow> videos_mapping_rows(const std::vector<MatchingT>& matchings) {
    std::vector<VideoMappingRow> rows;
    for (const auto& m : matchings) {
        VideoMappingRow r;
        r.video_ms = (uint32_t)(uint64_t)(m.video_time_s * 1000.0);           // as_millis() as u32   (db.rs:176)
        r.has_pdf = (bool)m.image;
        r.pdf_hash = m.image ? m.image->pdf_hash : std::string();             // db.rs:175
        r.page = m.image ? (uint32_t)(m.image->page_nr - 1) : 0u;             // db.rs:177
        rows.push_back(r);
    }
    return rows;
}

inline std::vector<PdfVideoMatching> pdf_video_matchings(std::vector<VideoMappingRow> rows, const std::string& pdf_hash,
                                                        const std::string& video_hash) {
    std::stable_sort(rows.begin(), rows.end(), [](const VideoMappingRow& a, const VideoMappingRow& b) { return a.video_ms < b.video_ms; });
    std::vector<PdfVideoMatching> out;
    for (size_t i = 0; i < rows.size(); ++i) {
        const uint32_t duration = i + 1 < rows.size() ? rows[i + 1].video_ms - rows[i].video_ms : 5000u;   // db.rs:239-245
        if (rows[i].has_pdf && rows[i].pdf_hash == pdf_hash)
            out.push_back({rows[i].video_ms, rows[i].pdf_hash, video_hash, rows[i].page, duration});
    }
    return out;
}

template <class I>
struct Matching {
    double video_time_s;
    size_t video_frame_idx;
    std::optional<I> image;
};

struct Image8 { int w = 0, h = 0; std::vector<uint8_t> bgr; };
using ImageLoader = std::function<Image8(const std::string& path)>;

inline Image8 load_ppm_bgr(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("File '" + path + "' must exist");                       // mo/lib.rs:95-97
    std::string magic; int w, h, maxv;
    f >> magic >> w >> h >> maxv;
    f.get();
    if (magic != "P6" || maxv != 255) throw std::runtime_error("Could not read file '" + path + "'");   // mo/lib.rs:99-101
    Image8 im; im.w = w; im.h = h; im.bgr.resize((size_t)w * h * 3);
    f.read(reinterpret_cast<char*>(im.bgr.data()), (std::streamsize)im.bgr.size());
    for (size_t i = 0; i < im.bgr.size(); i += 3) std::swap(im.bgr[i], im.bgr[i + 2]);        // RGB -> BGR
    return im;
}

// imread stand-in of the page ingest (mo/lib.rs:98-104): PNG (what pdftocairo writes) or binary PPM, by extension
inline Image8 load_image_bgr(const std::string& path) {
    const auto dot = path.rfind('.');
    std::string ext = dot == std::string::npos ? "" : path.substr(dot + 1);
    for (auto& c : ext) c = (char)std::tolower((unsigned char)c);
    if (ext == "png") { PngImage p = decode_png_bgr(path); Image8 im; im.w = p.w; im.h = p.h; im.bgr = std::move(p.bgr); return im; }
    return load_ppm_bgr(path);
}

// Page list of one PDF as the app builds it: every entry of the pdftocairo target directory is
// named "p-<nr>.png" (zero padded to the page count's width), page_nr = the number after "p-", pages sorted by it
// (crates/pdftocairo/src/pdftocairo.rs:216-231); PdfPage{page_nr (1-based), image_path, pdf_path, pdf_hash}
// (crates/app/src/pdf_to_images.rs:19-31,138-146).  A foreign file name is a panic there and an exception here.
struct PdfPage {
    size_t page_nr = 0; std::string image_path, pdf_path, pdf_hash;
    std::string get_path() const { return image_path; }                                     // MatchableImage, pdf_to_images.rs:33-37
    bool operator==(const PdfPage& o) const { return page_nr == o.page_nr && pdf_hash == o.pdf_hash; }
};

inline std::vector<PdfPage> scan_page_dir(const std::string& target_dir, const std::string& pdf_hash, const std::string& pdf_path = "") {
    std::vector<PdfPage> pages;
    for (const auto& item : std::filesystem::directory_iterator(target_dir)) {
        const std::string file_name = item.path().filename().string();                     // e.g. p-01.png
        const std::string stem = file_name.substr(0, file_name.find('.'));
        size_t used = 0; unsigned long nr = 0;
        bool ok = stem.size() > 2;
        if (ok) { try { nr = std::stoul(stem.substr(2), &used); } catch (const std::exception&) { ok = false; } }
        if (!ok || used != stem.size() - 2) throw std::runtime_error("unexpected file '" + file_name + "' in page directory '" + target_dir + "'");
        pages.push_back({(size_t)nr, item.path().string(), pdf_path, pdf_hash});
    }
    std::stable_sort(pages.begin(), pages.end(), [](const PdfPage& a, const PdfPage& b) { return a.page_nr < b.page_nr; });
    return pages;
}

// Raw BGR frame container standing in for VideoCapture (mo/video_capture.rs:16-40):
// "SLVF" u32 w u32 h f64 fps u64 n, then n * h*w*3 bytes (same layout as slideo_amd/matching.py RawVideo).
class RawVideo {
public:
    explicit RawVideo(const std::string& path) : path_(path), f_(path, std::ios::binary) {
        char magic[4];
        if (!f_ || !f_.read(magic, 4) || std::string(magic, 4) != "SLVF") throw std::runtime_error("not a raw frame container: " + path);
        uint32_t w, h; double fps; uint64_t n;
        f_.read(reinterpret_cast<char*>(&w), 4); f_.read(reinterpret_cast<char*>(&h), 4);
        f_.read(reinterpret_cast<char*>(&fps), 8); f_.read(reinterpret_cast<char*>(&n), 8);
        width = (int)w; height = (int)h; this->fps = fps; n_frames = n;
    }
    double total_frames() const { return (double)n_frames; }
    double total_time() const { return (double)n_frames / fps; }                                 // video_capture.rs:34-36
    void read(uint64_t idx, uint8_t* dst) {
        const size_t fb = (size_t)width * height * 3;
        f_.seekg((std::streamoff)(28 + idx * fb));
        f_.read(reinterpret_cast<char*>(dst), (std::streamsize)fb);
    }
    const std::string& path() const { return path_; }
    int width = 0, height = 0; double fps = 0; uint64_t n_frames = 0;
private:
    std::string path_;
    std::ifstream f_;
};

namespace detail {
// one slideo_group = one matcher per GPU of the node behind one handle (include/slideo_amd.h, "N-device group"): the N-device
// counterpart of the reference's fan-out over the global rayon pool (mo/lib.rs:45,174,213)
struct Handle {
    slideo_group* g = nullptr;
    int n_devices = 1;
    int32_t work_w = 0, work_h = 0;          // the working size the group was given (0, 0: none)
    int32_t reg_w = 0, reg_h = 0;            // the output size of the frame region the group was given (0, 0: none)
    bool gated = true;                       // tasks use the group's gated call (false: the stop-and-go mask + kept pair)
    int32_t gate_memory = 0;                 // the gate memory's capacity the group was given (0: none)
    ~Handle() { if (g) slideo_group_destroy(g); }
    void check(int32_t rc) const {
        if (rc != SLIDEO_OK) throw std::runtime_error(std::string("slideo_amd error ") + std::to_string(rc) + ": " + slideo_group_last_error(g));
    }
};
// The task's side of the gate memory (include/slideo_amd.h "Gate memory") behind a gate reset to "none": the verdicts of the matched
// ordinals it remembers (at most `capacity`, the library's own ring), the next frame's ordinal and the last frame's ref
struct GateMemory {
    std::map<int64_t, slideo_verdict> verdicts;
    int64_t next = 0, prev_ref = INT64_MIN;
    int32_t capacity = 0;
};
// What one gated call of n frames emits under a gate memory: (index in the call, verdict), in order.  A matched frame emits its own
// verdict, which is remembered under its ordinal; a frame that is not matched and whose ref >= 0 differs from the ref of the frame
// before it — a recall, or the return to the anchor behind deferred frames — emits the verdict of the frame it stands behind
inline void gate_memory_emission(int n, const uint8_t* changed, const int64_t* refs, const slideo_verdict* verdicts, GateMemory& mem,
                                 std::vector<int32_t>& idx, std::vector<slideo_verdict>& v) {
    for (int i = 0; i < n; ++i) {
        if (changed[i]) {
            mem.verdicts[mem.next + i] = verdicts[i];
            while ((int64_t)mem.verdicts.size() > mem.capacity) mem.verdicts.erase(mem.verdicts.begin());
            idx.push_back(i); v.push_back(verdicts[i]);
        } else if (refs[i] >= 0 && refs[i] != mem.prev_ref) {
            const auto it = mem.verdicts.find(refs[i]);
            if (it != mem.verdicts.end()) { idx.push_back(i); v.push_back(it->second); }
        }
        mem.prev_ref = refs[i];
    }
    mem.next += n;
}
inline void tramp(void* user, uint64_t d, uint64_t t, const char* msg) {
    static_cast<const ProgressReporter*>(user)->report(d, t, msg ? msg : "");
}
}  // namespace detail

template <class I>
class VideoMatcherTask {                                       // matching::VideoMatcherTask (lib.rs:26-29)
public:
    virtual ~VideoMatcherTask() = default;
    virtual std::vector<Matching<I>> process() = 0;
};

template <class I>
class VideoMatcher {                                           // matching::VideoMatcher (lib.rs:16-24)
public:
    virtual ~VideoMatcher() = default;
    virtual std::unique_ptr<VideoMatcherTask<I>> match_images_with_video(const std::string& video_path, ProgressReporter reporter) = 0;
};

template <class I>
class HipVideoMatcherTask : public VideoMatcherTask<I> {       // OpenCVVideoMatcherTask (mo/lib.rs:161-246)
public:
    HipVideoMatcherTask(std::shared_ptr<detail::Handle> h, std::shared_ptr<std::vector<I>> images, std::string video_path,
                        ProgressReporter rep, float changed_similarity)
        : h_(std::move(h)), images_(std::move(images)), video_path_(std::move(video_path)), rep_(std::move(rep)) { (void)changed_similarity; }

    std::vector<Matching<I>> process() override {
        RawVideo video(video_path_);
        const double interval = 5.0;
        const double total_time = video.total_time();
        const uint64_t frames_to_process = (uint64_t)(total_time / interval);                       // mo/lib.rs:179
        std::vector<Matching<I>> results;
        results.push_back({total_time, (size_t)video.total_frames(), std::nullopt});                // sentinel, mo/lib.rs:185-189
        const std::string name = video_path_.substr(video_path_.find_last_of("/\\") + 1);
        uint64_t progress = 0;
        const double step = std::floor(video.fps * interval);
        const size_t fb = (size_t)video.width * video.height * 3;
        const int batch = 64 * h_->n_devices;             // one shard of 64 sampled frames per device and call
        std::vector<uint8_t> frames, prev_small, last_small;
        std::vector<std::pair<double, size_t>> meta;
        int sw = 0, sh = 0;
        // the changed-frame gate (slideo_amd.h "Changed-frame gate"): the group's gated call for any member count, one call per flush,
        // every shard after the first primed from the frame before its block, the last small image carried in the group
        const bool gate = h_->gated;
        if (gate) h_->check(slideo_group_gate_reset(h_->g, nullptr, 0, 0));             // the first frame of the video is always changed
        detail::GateMemory memory;
        memory.capacity = h_->gate_memory;
        auto emit = [&](const std::vector<int32_t>& idx, const slideo_verdict* v) {
            for (size_t k = 0; k < idx.size(); ++k) {
                std::optional<I> img;
                if (v[k].page_idx >= 0) img = (*images_)[(size_t)v[k].page_idx];
                results.push_back({meta[idx[k]].first, meta[idx[k]].second, img});
            }
        };
        auto flush = [&]() {
            if (meta.empty()) return;
            const int n = (int)meta.size();
            std::vector<uint8_t> changed(n);
            if (gate) {       // MarkSimilarIter + match_images_with_frame of the changed frames (mo/lib.rs:205-214) in one call
                std::vector<slideo_verdict> all(n), v;
                h_->check(slideo_group_match_changed_frames_bgr8(h_->g, n, frames.data(), video.width, video.height, video.width * 3, (int64_t)fb,
                                                                 changed.data(), nullptr, all.data()));
                std::vector<int32_t> idx;
                if (memory.capacity > 0) {
                    // a recalled frame has changed == 0 but shows another page than the frame before it: the verdict of the frame
                    // it stands behind is emitted at its time (slideo_amd.h "Gate memory")
                    std::vector<int64_t> refs((size_t)n);
                    int64_t nrefs = 0;
                    h_->check(slideo_group_last_gate_refs(h_->g, refs.data(), n, &nrefs));
                    if (nrefs != n) throw std::runtime_error("slideo_group_last_gate_refs: the refs are not the call's");
                    detail::gate_memory_emission(n, changed.data(), refs.data(), all.data(), memory, idx, v);
                } else
                    for (int i = 0; i < n; ++i) if (changed[i]) { idx.push_back(i); v.push_back(all[i]); }
                emit(idx, v.data());
                for (int i = 0; i < n; ++i) rep_.report(++progress, frames_to_process, "Processing frames of '" + name + "'...");   // mo/lib.rs:192-203
                meta.clear(); frames.clear();
                return;
            }
            if (last_small.empty()) {       // size of the small image: ask once
                std::vector<uint8_t> tmp(fb), red;
                const uint8_t* img = frames.data();
                int32_t a, b, uw = video.width, uh = video.height;
                if (h_->reg_w > 0) {                                 // the mask compares the small images of the RECTIFIED frames
                    uw = h_->reg_w; uh = h_->reg_h;
                    red.resize((size_t)uw * uh * 3);
                    h_->check(slideo_rectify_bgr8(slideo_group_member(h_->g, 0), frames.data(), video.width, video.height, video.width * 3, red.data(), (int64_t)red.size()));
                    img = red.data();
                } else if (h_->work_w > 0) h_->check(slideo_working_size(video.width, video.height, h_->work_w, h_->work_h, &uw, &uh));
                if (h_->reg_w == 0 && (uw != video.width || uh != video.height)) {      // the mask compares the small images of the REDUCED frames
                    red.resize((size_t)uw * uh * 3);
                    h_->check(slideo_reduce_bgr8(slideo_group_member(h_->g, 0), frames.data(), video.width, video.height, video.width * 3, uw, uh, red.data(), (int64_t)red.size()));
                    img = red.data();
                }
                h_->check(slideo_small_image_bgr8(slideo_group_member(h_->g, 0), img, uw, uh, uw * 3, tmp.data(), (int64_t)tmp.size(), &a, &b));
                sw = a; sh = b; last_small.resize((size_t)sw * sh * 3);
            }
            h_->check(slideo_group_changed_mask_bgr8(h_->g, n, frames.data(), video.width, video.height, video.width * 3, (int64_t)fb,
                                               prev_small.empty() ? nullptr : prev_small.data(), last_small.data(), changed.data(), nullptr));   // video_capture.rs:86-98
            prev_small = last_small;
            std::vector<int32_t> idx;
            for (int i = 0; i < n; ++i) if (changed[i]) idx.push_back(i);
            if (!idx.empty()) {
                std::vector<slideo_verdict> v(idx.size());
                // mo/lib.rs:213-214 on the copy of the frames the mask call left on the devices (no second upload)
                h_->check(slideo_group_match_kept_frames(h_->g, (int32_t)idx.size(), idx.data(), v.data()));
                emit(idx, v.data());
            }
            for (int i = 0; i < n; ++i) rep_.report(++progress, frames_to_process, "Processing frames of '" + name + "'...");   // mo/lib.rs:192-203
            meta.clear(); frames.clear();
        };
        for (uint64_t idx = 0; idx < video.n_frames; ++idx) {                                      // VideoCaptureIter, video_capture.rs:42-57
            if (step <= 0 || !(std::fmod((double)idx, step) < 1.0)) continue;   // step 0 (fps < 0.2): `idx % 0.0` is NaN in the reference, nothing is retrieved (video_capture.rs:53)
            frames.resize(frames.size() + fb);
            video.read(idx, frames.data() + frames.size() - fb);
            meta.push_back({(double)idx / video.fps, (size_t)idx});
            if ((int)meta.size() >= batch) flush();
        }
        flush();
        rep_.report(frames_to_process, frames_to_process, "Finished!");                              // mo/lib.rs:223-227
        // mo/lib.rs:229-244: stable sort by time, drop consecutive mappings with the same image
        std::stable_sort(results.begin(), results.end(), [](const Matching<I>& a, const Matching<I>& b) { return a.video_time_s < b.video_time_s; });
        std::vector<Matching<I>> cleaned;
        for (auto& mm : results) {
            if (!cleaned.empty() && cleaned.back().image == mm.image) continue;
            cleaned.push_back(mm);
        }
        return cleaned;
    }
private:
    std::shared_ptr<detail::Handle> h_;
    std::shared_ptr<std::vector<I>> images_;
    std::string video_path_;
    ProgressReporter rep_;
};

template <class I>
class HipVideoMatcher : public VideoMatcher<I> {               // OpenCVVideoMatcher (mo/lib.rs:134-158)
public:
    HipVideoMatcher(std::shared_ptr<detail::Handle> h, std::shared_ptr<std::vector<I>> images) : h_(std::move(h)), images_(std::move(images)) {}
    std::unique_ptr<VideoMatcherTask<I>> match_images_with_video(const std::string& video_path, ProgressReporter reporter) override {
        RawVideo video(video_path);
        reporter.report(0, (uint64_t)(video.total_time() / 5.0), "");                               // mo/lib.rs:148-150
        return std::make_unique<HipVideoMatcherTask<I>>(h_, images_, video_path, std::move(reporter), 0.98f);
    }
    // Frame lists (include/slideo_amd.h "Frame lists"; an extension): a batch given as per-frame plane pointers — one cv::Mat or one
    // AVFrame per frame — instead of one contiguous buffer.  Host lists; the results are the contiguous calls' bit for bit.
    // bgr_frame_list: the record of n BGR-door frames, each its own buffer with rows `stride_bytes` apart (planes: 3 n entries, filled
    // here and kept by the caller until the call returns).
    static slideo_frame_list bgr_frame_list(const std::vector<const uint8_t*>& frames, int32_t width, int32_t height, int64_t stride_bytes,
                                            std::vector<const void*>& planes) {
        planes.assign(frames.size() * 3, nullptr);
        for (size_t i = 0; i < frames.size(); ++i) planes[3 * i] = frames[i];
        slideo_frame_list L{};
        L.door = SLIDEO_FRAME_LIST_BGR; L.n_frames = (int32_t)frames.size(); L.width = width; L.height = height;
        L.stride[0] = stride_bytes;
        L.planes = planes.data();
        return L;
    }
    std::vector<slideo_verdict> match_frames_list(const slideo_frame_list& list) {
        std::vector<slideo_verdict> out((size_t)std::max(list.n_frames, 0));
        h_->check(slideo_group_match_frames_list(h_->g, &list, out.data()));
        return out;
    }
    // -> verdicts; changed [n] and similarity [n] (may be null) as slideo_group_match_changed_frames_bgr8 fills them
    std::vector<slideo_verdict> match_changed_frames_list(const slideo_frame_list& list, uint8_t* changed, float* similarity = nullptr) {
        std::vector<slideo_verdict> out((size_t)std::max(list.n_frames, 0));
        h_->check(slideo_group_match_changed_frames_list(h_->g, &list, changed, similarity, out.data()));
        return out;
    }
    void changed_mask_list(const slideo_frame_list& list, const uint8_t* prev_small, uint8_t* last_small_out, uint8_t* changed, float* similarity = nullptr) {
        h_->check(slideo_group_changed_mask_list(h_->g, &list, prev_small, last_small_out, changed, similarity));
    }
    // Match evidence map (include/slideo_amd.h "Match evidence map"; an extension): while a session is open, the tasks' match calls
    // count where the keypoints of matched frames fall (seen) and which of them the winning page's transform explains (hit), per
    // cell x cell cell of the analysed image, summed over the devices.  No task may be running at begin, counts or end.  The counts go
    // to slideo_evidence_mask / slideo_evidence_box; nothing is installed, and no value has a default.
    struct EvidenceCounts {
        int32_t cell = 0, min_inliers = 0, aw = 0, ah = 0, gw = 0, gh = 0;
        int64_t frames_through = 0, frames_counted = 0;
        std::vector<uint32_t> seen, hit;               // gh rows of gw elements (evidence_info leaves them empty)
    };
    void evidence_begin(int32_t cell, int32_t min_inliers) { h_->check(slideo_group_evidence_begin(h_->g, cell, min_inliers)); }
    void evidence_end() { h_->check(slideo_group_evidence_end(h_->g)); }
    EvidenceCounts evidence_info() const {
        EvidenceCounts e;
        h_->check(slideo_group_evidence_info(h_->g, &e.cell, &e.min_inliers, &e.aw, &e.ah, &e.gw, &e.gh, &e.frames_through, &e.frames_counted));
        return e;
    }
    EvidenceCounts evidence_counts() const {
        EvidenceCounts e = evidence_info();
        const size_t nc = (size_t)e.gw * e.gh;
        e.seen.assign(nc, 0); e.hit.assign(nc, 0);
        if (nc) h_->check(slideo_group_evidence_counts(h_->g, e.seen.data(), e.hit.data(), (int64_t)nc, &e.gw, &e.gh, &e.frames_through, &e.frames_counted));
        return e;
    }
    // Match tone table (include/slideo_amd.h "Match tone table"; an extension): while a session is open, the tasks' match calls count,
    // per channel and frame value, the page values of the small-image pixels that the contributing candidate's hits enclose, summed
    // over the devices.  No task may be running at begin, counts or end.  tone_lut makes the levels table of the counts (what
    // slideo_group_set_frame_levels takes); nothing is installed, and no value has a default.
    struct ToneCounts {
        int32_t min_inliers = 0, min_hits = 0, flat = 0;
        int64_t frames_through = 0, frames_counted = 0;
        std::vector<uint64_t> cnt, sum;                // 3 x 256 each: B, G, R by frame value (tone_info leaves them empty)
    };
    void tone_begin(int32_t min_inliers, int32_t min_hits, int32_t flat) { h_->check(slideo_group_tone_begin(h_->g, min_inliers, min_hits, flat)); }
    void tone_end() { h_->check(slideo_group_tone_end(h_->g)); }
    ToneCounts tone_info() const {
        ToneCounts t;
        h_->check(slideo_group_tone_info(h_->g, &t.min_inliers, &t.min_hits, &t.flat, &t.frames_through));
        return t;
    }
    ToneCounts tone_counts() const {
        ToneCounts t = tone_info();
        t.cnt.assign(768, 0); t.sum.assign(768, 0);
        h_->check(slideo_group_tone_counts(h_->g, t.cnt.data(), t.sum.data(), &t.frames_through, &t.frames_counted));
        return t;
    }
    // the table of the counts; false: a channel in which no frame value was seen min_count times
    static bool tone_lut(const ToneCounts& t, int64_t min_count, std::vector<uint8_t>& lut768) {
        lut768.assign(768, 0);
        return t.cnt.size() == 768 && t.sum.size() == 768 && slideo_tone_lut(t.cnt.data(), t.sum.data(), min_count, lut768.data()) == SLIDEO_OK;
    }
    // Match placement map (include/slideo_amd.h "Match placement map"; an extension): while a session is open, the tasks' match calls
    // sum, per cell of the analysed image, the frame positions of the keypoints that the contributing candidate explains within
    // `reach` pixels and the unit-slide positions of their page points, over the devices.  No task may be running at begin, sums or
    // end.  placement_quad fits the keystoned quad (what slideo_frame_region_from_quad takes); nothing is installed, no value has a default.
    struct PlacementSums {
        int32_t cell = 0, min_inliers = 0, aw = 0, ah = 0, gw = 0, gh = 0;
        double reach = 0;
        int64_t frames_through = 0, frames_counted = 0;
        std::vector<uint64_t> n, sfx, sfy, su, sv;     // gh rows of gw each (placement_info leaves them empty)
    };
    struct PlacementQuad { double quad[8] = {0}, H[9] = {0}, rms_px = 0; int32_t cells_used = 0; };
    void placement_begin(int32_t cell, int32_t min_inliers, double reach) { h_->check(slideo_group_placement_begin(h_->g, cell, min_inliers, reach)); }
    void placement_end() { h_->check(slideo_group_placement_end(h_->g)); }
    PlacementSums placement_info() const {
        PlacementSums p;
        h_->check(slideo_group_placement_info(h_->g, &p.cell, &p.min_inliers, &p.reach, &p.aw, &p.ah, &p.gw, &p.gh, &p.frames_through));
        return p;
    }
    PlacementSums placement_sums() const {
        PlacementSums p = placement_info();
        const size_t nc = (size_t)p.gw * (size_t)p.gh;
        p.n.assign(nc, 0); p.sfx.assign(nc, 0); p.sfy.assign(nc, 0); p.su.assign(nc, 0); p.sv.assign(nc, 0);
        if (nc)
            h_->check(slideo_group_placement_sums(h_->g, p.n.data(), p.sfx.data(), p.sfy.data(), p.su.data(), p.sv.data(), (int64_t)nc, &p.gw, &p.gh,
                                                  &p.frames_through, &p.frames_counted));
        return p;
    }
    // Match shading map (include/slideo_amd.h "Match shading map"; an extension): while a session is open, the tasks' match calls sum,
    // per cell of the analysed image, the samples of the tone table's sampler that land there and the B + G + R of their frame and
    // page pixels, over the devices.  No task may be running at begin, sums or end; refused while a frame shading or a levels table
    // is set.  shading_field makes the gains (what with_frame_shading takes); nothing is installed, no value has a default.
    struct ShadingSums {
        int32_t cell = 0, min_inliers = 0, min_hits = 0, flat = 0, aw = 0, ah = 0, gw = 0, gh = 0;
        int64_t frames_through = 0, frames_counted = 0;
        std::vector<uint64_t> cnt, sum_f, sum_p;       // gh rows of gw each (shading_info leaves them empty)
    };
    void shading_begin(int32_t cell, int32_t min_inliers, int32_t min_hits, int32_t flat) {
        h_->check(slideo_group_shading_begin(h_->g, cell, min_inliers, min_hits, flat));
    }
    void shading_end() { h_->check(slideo_group_shading_end(h_->g)); }
    ShadingSums shading_info() const {
        ShadingSums p;
        h_->check(slideo_group_shading_info(h_->g, &p.cell, &p.min_inliers, &p.min_hits, &p.flat, &p.aw, &p.ah, &p.gw, &p.gh, &p.frames_through));
        return p;
    }
    ShadingSums shading_sums() const {
        ShadingSums p = shading_info();
        const size_t nc = (size_t)p.gw * (size_t)p.gh;
        p.cnt.assign(nc, 0); p.sum_f.assign(nc, 0); p.sum_p.assign(nc, 0);
        if (nc)
            h_->check(slideo_group_shading_sums(h_->g, p.cnt.data(), p.sum_f.data(), p.sum_p.data(), (int64_t)nc, &p.gw, &p.gh, &p.frames_through,
                                                &p.frames_counted));
        return p;
    }
    // the field of the sums, (gh + 1) * (gw + 1) Q8.8 nodes; false: a bad argument or no cell of min_count samples
    static bool shading_field(const ShadingSums& p, int64_t min_count, int32_t min_gain_q8, int32_t max_gain_q8, int32_t smooth, std::vector<uint16_t>& gains) {
        const size_t nc = (size_t)p.gw * (size_t)p.gh;
        if (!nc || p.cnt.size() != nc || p.sum_f.size() != nc || p.sum_p.size() != nc) return false;
        gains.assign((size_t)(p.gw + 1) * (size_t)(p.gh + 1), 256);
        return slideo_shading_field(p.cnt.data(), p.sum_f.data(), p.sum_p.data(), p.gw, p.gh, p.cell, min_count, min_gain_q8, max_gain_q8, smooth,
                                    gains.data(), nullptr) == SLIDEO_OK;
    }
    // the quad of the sums; false: fewer than 4 cells of min_count keypoints at a stage, or cells that determine no homography
    static bool placement_quad(const PlacementSums& p, int64_t min_count, double trim_px, int32_t rounds, PlacementQuad& out) {
        const size_t nc = (size_t)p.gw * (size_t)p.gh;
        if (!nc || p.n.size() != nc || p.sfx.size() != nc || p.sfy.size() != nc || p.su.size() != nc || p.sv.size() != nc) return false;
        return slideo_placement_quad(p.n.data(), p.sfx.data(), p.sfy.data(), p.su.data(), p.sv.data(), p.gw, p.gh, p.cell, p.aw, p.ah, min_count, trim_px,
                                     rounds, out.quad, out.H, &out.cells_used, &out.rms_px) == SLIDEO_OK;
    }
    // the lens and the quad of the sums, fitted jointly (slideo_placement_lens, include/slideo_amd.h "Placement lens"): the sums of a
    // session that ran with no lens and no region; cx, cy, f: the lens's centre and normaliser, given; order 1 (k1) or 2 (k1, k2).
    // out.quad is in IDEAL coordinates (what with_frame_region takes beside with_frame_lens).  false: refused
    struct PlacementLens { double k[2] = {0, 0}, quad[8] = {0}, H[9] = {0}, rms_px = 0; int32_t cells_used = 0; };
    static bool placement_lens(const PlacementSums& p, int64_t min_count, double cx, double cy, double f, int32_t order, double trim_px, int32_t rounds,
                               int32_t iters, PlacementLens& out) {
        const size_t nc = (size_t)p.gw * (size_t)p.gh;
        if (!nc || p.n.size() != nc || p.sfx.size() != nc || p.sfy.size() != nc || p.su.size() != nc || p.sv.size() != nc) return false;
        return slideo_placement_lens(p.n.data(), p.sfx.data(), p.sfy.data(), p.su.data(), p.sv.data(), p.gw, p.gh, p.cell, p.aw, p.ah, min_count, cx, cy, f,
                                     order, trim_px, rounds, iters, out.k, out.quad, out.H, &out.cells_used, &out.rms_px) == SLIDEO_OK;
    }
private:
    std::shared_ptr<detail::Handle> h_;
    std::shared_ptr<std::vector<I>> images_;
};

// Drop-in for OpenCVImageVideoMatcher behind matching::ImageVideoMatcher (mo/lib.rs:34-73).
// I must provide `std::string get_path() const` (matching::MatchableImage, lib.rs:31-33) and operator==.
class HipImageVideoMatcher {
public:
    // device >= 0: that one device; -1 (default): every gfx950 device of the node (with_devices names them explicitly)
    explicit HipImageVideoMatcher(int device = -1, const slideo_config* cfg = nullptr, ImageLoader loader = load_image_bgr)
        : loader_(std::move(loader)) {
        if (device >= 0) devices_.push_back(device);
        slideo_config_default(&cfg_);
        if (cfg) cfg_ = *cfg;
    }
    HipImageVideoMatcher& with_devices(std::vector<int32_t> devices) { devices_ = std::move(devices); return *this; }
    // SIFT features + squared-L2 search instead of the reference's ORB + Hamming (slideo_group_use_sift).  ratio 0 (default): the
    // path's own 5 % tolerance vote on the L2 distances — the robust choice on decks whose pages share a template; ratio in
    // (0, 1]: Lowe's ratio test on the two nearest rows (the north_star's wording)
    HipImageVideoMatcher& with_sift(float ratio = 0.f) { sift_on_ = true; sift_ratio_ = ratio; return *this; }
    // Frames beyond max_w x max_h are reduced on the GPU before matching (slideo_group_set_working_size; include/slideo_amd.h
    // "Working size").  The reference never reduces a frame: verdicts are then those of the reduced video.  Default: none
    HipImageVideoMatcher& with_working_size(int32_t max_w, int32_t max_h) { work_w_ = max_w; work_h_ = max_h; return *this; }
    // ORB keypoints of the frames are detected under `mask` (width x height bytes, nonzero = detect here; slideo_group_set_frame_mask,
    // include/slideo_amd.h "Frame mask"): a speaker inset, a logo or subtitles stay out of the features.  Detection only; the frames'
    // analysed size must be the mask's.  The reference passes no mask.  Default: none
    // Frames of src_w x src_h stand for the out_w x out_h image rectified from `quad`: the source coordinates x, y of the slide's
    // top-left, top-right, bottom-right and bottom-left corner (slideo_frame_region_from_quad, slideo_group_set_frame_region;
    // include/slideo_amd.h "Frame region"): a filmed projection screen, a slide in a sub-window.  The output must fit a working
    // size.  The reference analyses the whole frame.  Default: none
    HipImageVideoMatcher& with_frame_region(int32_t src_w, int32_t src_h, const double (&quad)[8], int32_t out_w, int32_t out_h) {
        if (slideo_frame_region_from_quad(quad, out_w, out_h, reg_M_) != SLIDEO_OK) throw std::runtime_error("with_frame_region: a degenerate or non-convex quad");
        reg_sw_ = src_w; reg_sh_ = src_h; reg_ow_ = out_w; reg_oh_ = out_h;
        return *this;
    }
    // The radial lens of a wide-angle room camera (slideo_group_set_frame_lens, include/slideo_amd.h "Frame lens"): a point p of the
    // ideal source plane is seen at c + (p - c) (1 + k1 r2 + k2 r2^2), r2 = |p - c|^2 / f^2, and frames of src_w x src_h are
    // undistorted in the launch that rectifies; a region's quad is then given in ideal coordinates.  cx, cy, f < 0: the image centre
    // and half the source diagonal.  Applied after the region.  The reference analyses the frame as the camera saw it.  Default: none
    HipImageVideoMatcher& with_frame_lens(int32_t src_w, int32_t src_h, double k1, double k2 = 0.0, double cx = -1.0, double cy = -1.0, double f = -1.0) {
        lens_sw_ = src_w; lens_sh_ = src_h; lens_k1_ = k1; lens_k2_ = k2;
        lens_cx_ = cx < 0 ? (src_w - 1) / 2.0 : cx; lens_cy_ = cy < 0 ? (src_h - 1) / 2.0 : cy;
        lens_f_ = f < 0 ? 0.5 * std::sqrt((double)src_w * src_w + (double)src_h * src_h) : f;
        return *this;
    }
    HipImageVideoMatcher& with_frame_mask(std::vector<uint8_t> mask, int32_t width, int32_t height) {
        if (width < 1 || height < 1 || mask.size() != (size_t)width * (size_t)height) throw std::runtime_error("with_frame_mask: mask is not width x height bytes");
        mask_ = std::move(mask); mask_w_ = width; mask_h_ = height;
        return *this;
    }
    // Which stages the frame mask applies to: SLIDEO_MASK_DETECT (default), SLIDEO_MASK_GATE or both (slideo_group_set_frame_mask_scope,
    // include/slideo_amd.h "Frame mask scope").  With SLIDEO_MASK_GATE the changed-frame gate ignores the masked regions too: an
    // inset that moves on every frame no longer flags every held slide as changed
    HipImageVideoMatcher& with_frame_mask_scope(uint32_t scope) { mask_scope_ = scope; return *this; }
    // The direct page look-up (slideo_group_set_direct_similarity, include/slideo_amd.h "Direct page look-up"): t in (0, 1]; a
    // changed frame whose small image is at least that similar to a page's is resolved to that page without ORB, search or
    // verify (full-screen slide frames of a screen recording; the reference never decides without keypoints).  Not together with
    // SLIDEO_MASK_GATE.  Default 0: off
    HipImageVideoMatcher& with_direct_similarity(float t) { direct_t_ = t; return *this; }
    // What the direct page look-up compares (slideo_group_set_direct_scope, include/slideo_amd.h "Direct look-up scope"):
    // SLIDEO_DIRECT_WHOLE (default: whole small images, refused beside SLIDEO_MASK_GATE) or SLIDEO_DIRECT_VALID (the valid pixels
    // of the gate's validity map: a full-screen slide under a speaker thumbnail).  Applied before the direct similarity
    HipImageVideoMatcher& with_direct_scope(uint32_t scope) { direct_scope_ = scope; return *this; }
    // How YUV 4:2:0 frames are read (slideo_group_set_yuv_description, include/slideo_amd.h "YUV colour description"):
    // SLIDEO_YUV_MATRIX_* / _RANGE_* / _DEPTH_*; BT.709 for HD recordings, full range for many screen recorders, a 10-bit depth for
    // P010 / yuv420p10le frames (layouts then count bytes of 16-bit containers).  The reference reads every stream as BT.601
    // limited range.  Default: BT601, LIMITED, 8-bit
    HipImageVideoMatcher& with_yuv_description(int32_t matrix, int32_t range, int32_t depth = SLIDEO_YUV_DEPTH_8) {
        yuv_matrix_ = matrix; yuv_range_ = range; yuv_depth_ = depth;
        return *this;
    }
    // Where the samples of the YUV frames lie (slideo_group_set_yuv_sampling, include/slideo_amd.h "YUV sampling"):
    // SLIDEO_YUV_SAMPLING_420 (default), _422, _444 (screen recorders) or _422_PACKED (YUY2 / UYVY of capture cards; 8-bit).  Every
    // call that takes a slideo_yuv420_layout reads its frames under it.  The reference knows BGR only
    HipImageVideoMatcher& with_yuv_sampling(int32_t sampling) { yuv_sampling_ = sampling; return *this; }
    // How a pixel's chroma is read from 4:2:0 and 4:2:2 frames (slideo_group_set_yuv_chroma, include/slideo_amd.h "YUV chroma
    // filter"): SLIDEO_YUV_CHROMA_NEAREST (default: cvtColor's rule), _BILINEAR_LEFT (H.264 / HEVC / MPEG-2 siting), _BILINEAR_CENTER
    // (JPEG, MPEG-1) or _BILINEAR_TOPLEFT (BT.2020).  The reference's swscale path takes the nearest sample
    HipImageVideoMatcher& with_yuv_chroma(int32_t filter) { yuv_chroma_ = filter; return *this; }
    // HDR frames to SDR (slideo_group_set_yuv_transfer, include/slideo_amd.h "YUV transfer"): SLIDEO_YUV_TRANSFER_SDR (default),
    // _HLG or _PQ, both BT.2020; white_nits: the display light that becomes SDR white (0 = 203).  Needs a 10-bit depth and nearest
    // chroma (or 4:4:4).  The reference knows no HDR
    HipImageVideoMatcher& with_yuv_transfer(int32_t transfer, float white_nits = 0.f) { yuv_transfer_ = transfer; yuv_white_nits_ = white_nits; return *this; }
    // How the frames of the BGR door are read (slideo_group_set_pixel_format, include/slideo_amd.h "Frame pixel format"):
    // SLIDEO_PIXEL_BGR8 (default), _RGB8, the four-byte _BGRA8 / _RGBA8 / _ARGB8 / _ABGR8 of screen-capture APIs, or the planar
    // _PLANAR_RGB8 / _PLANAR_BGR8 / _PLANAR_GBR8.  The frame source then hands out frames in that format; pages stay BGR.  The
    // reference only ever sees OpenCV's BGR
    HipImageVideoMatcher& with_pixel_format(int32_t format) { pixel_format_ = format; return *this; }
    // A per-channel tone table uint8 [3][256] (B, G, R; slideo_group_set_frame_levels, include/slideo_amd.h "Frame levels") applied to
    // every frame's analysed image as the last step in front of the pipeline: what slideo_frame_levels_lut makes of the points
    // slideo_matcher_levels_points learnt from a dim, low-contrast or colour-cast recording.  Pages are untouched; null: off.  The
    // reference analyses the frames as they are
    HipImageVideoMatcher& with_frame_levels(const uint8_t* lut768) {
        if (lut768) frame_levels_.assign(lut768, lut768 + 768); else frame_levels_.clear();
        return *this;
    }
    // A bilinear Q8.8 gain field (slideo_group_set_frame_shading, include/slideo_amd.h "Frame shading") over the aw x ah analysed image:
    // uint16 [gh + 1][gw + 1] nodes cell (16, 32 or 64) pixels apart, 256 = 1.0, applied in front of the frame levels — what
    // slideo_shading_field makes of per-cell sums, for the vignetting of a filmed projection screen.  Pages are untouched; null: off
    HipImageVideoMatcher& with_frame_shading(int32_t aw, int32_t ah, int32_t cell, const uint16_t* gains) {
        shading_.clear();
        if (gains && cell > 0 && aw > 0 && ah > 0) shading_.assign(gains, gains + (size_t)((aw + cell - 1) / cell + 1) * ((ah + cell - 1) / cell + 1));
        shading_aw_ = aw; shading_ah_ = ah; shading_cell_ = cell;
        return *this;
    }
    // Which frame a gated frame is compared with (slideo_group_set_gate_reference, include/slideo_amd.h "Gate reference"):
    // SLIDEO_GATE_PREVIOUS (default: the frame before, the reference's MarkSimilarIter) or SLIDEO_GATE_ANCHOR (the last frame that
    // was flagged: a change spread over many frames is still flagged when every decoded frame is fed).  One device only: a group of
    // several refuses SLIDEO_GATE_ANCHOR when it is built (SLIDEO_ERR_UNSUPPORTED)
    HipImageVideoMatcher& with_gate_reference(uint32_t ref) { gate_ref_ = ref; return *this; }
    // The gate settle (slideo_group_set_gate_settle, include/slideo_amd.h "Gate settle"), under SLIDEO_GATE_ANCHOR only: a frame away
    // from the last matched frame is matched once it is within settle_similarity of the frame before it, or after max_defer
    // deferred frames; a deferred frame is reported as unchanged.  0: off (default)
    HipImageVideoMatcher& with_gate_settle(float settle_similarity, int32_t max_defer) {
        settle_similarity_ = settle_similarity; settle_max_defer_ = max_defer;
        return *this;
    }
    // The gate memory (slideo_group_set_gate_memory, include/slideo_amd.h "Gate memory"), under SLIDEO_GATE_ANCHOR only, applied after
    // the gate reference and the settle: the last `capacity` (1 .. 64) matched frames are remembered and a frame that returns to one
    // of them is recalled, not matched again; the task emits the remembered verdict at that frame's time.  One device only.  0: off
    HipImageVideoMatcher& with_gate_memory(int32_t capacity) { gate_memory_ = capacity; return *this; }
    // The group gate order (slideo_group_set_gate_order, include/slideo_amd.h "Group gate order"), applied before the gate reference
    // and the settle: SLIDEO_GROUP_GATE_HALO (default: a later device's shard is primed from one frame) or SLIDEO_GROUP_GATE_CHAIN
    // (every shard receives the whole gate state of the shard before it: SLIDEO_GATE_ANCHOR and a settle on any number of devices)
    HipImageVideoMatcher& with_group_gate_order(uint32_t order) { gate_order_ = order; return *this; }
    // false: tasks run the stop-and-go pair slideo_group_changed_mask_bgr8 + slideo_group_match_kept_frames in place of the group's
    // gated call (the same timeline; for comparisons).  Default: gated
    HipImageVideoMatcher& with_changed_gate(bool on) { gated_ = on; return *this; }
    template <class I>
    std::unique_ptr<VideoMatcher<I>> create_video_matcher(std::vector<I> images, ProgressReporter reporter) const {
        auto h = std::make_shared<detail::Handle>();
        // no explicit list: every gfx950 device of the node, enumerated by the library (n_devices 0; no device at all: create reports it)
        int32_t rc = slideo_group_create(&cfg_, (int32_t)devices_.size(), devices_.empty() ? nullptr : devices_.data(), &h->g);
        if (rc != SLIDEO_OK) throw std::runtime_error(std::string("slideo_amd error ") + std::to_string(rc) + ": " + slideo_group_last_error(nullptr));
        h->n_devices = (int)slideo_group_device_count(h->g);
        h->gated = gated_;
        if (gate_order_ != SLIDEO_GROUP_GATE_HALO) h->check(slideo_group_set_gate_order(h->g, gate_order_));
        if (gate_ref_ != SLIDEO_GATE_PREVIOUS) h->check(slideo_group_set_gate_reference(h->g, gate_ref_));
        if (settle_similarity_ != 0.f) h->check(slideo_group_set_gate_settle(h->g, settle_similarity_, settle_max_defer_));
        if (gate_memory_ != 0) { h->check(slideo_group_set_gate_memory(h->g, gate_memory_)); h->gate_memory = gate_memory_; }
        if (sift_on_) {                                                                             // the north-star's SIFT + L2 front end
            slideo_sift_config sc;
            slideo_sift_config_default(&sc);
            h->check(slideo_group_use_sift(h->g, &sc, sift_ratio_));
        }
        if (work_w_ > 0 || work_h_ > 0) {
            h->check(slideo_group_set_working_size(h->g, work_w_, work_h_));
            h->work_w = work_w_; h->work_h = work_h_;
        }
        if (reg_ow_ > 0) {
            h->check(slideo_group_set_frame_region(h->g, reg_sw_, reg_sh_, reg_M_, reg_ow_, reg_oh_));
            h->reg_w = reg_ow_; h->reg_h = reg_oh_;
        }
        if (lens_k1_ != 0.0 || lens_k2_ != 0.0)
            h->check(slideo_group_set_frame_lens(h->g, lens_sw_, lens_sh_, lens_cx_, lens_cy_, lens_f_, lens_k1_, lens_k2_));
        if (yuv_matrix_ != SLIDEO_YUV_MATRIX_BT601 || yuv_range_ != SLIDEO_YUV_RANGE_LIMITED || yuv_depth_ != SLIDEO_YUV_DEPTH_8)
            h->check(slideo_group_set_yuv_description(h->g, yuv_matrix_, yuv_range_, yuv_depth_));
        if (yuv_sampling_ != SLIDEO_YUV_SAMPLING_420) h->check(slideo_group_set_yuv_sampling(h->g, yuv_sampling_));
        if (yuv_chroma_ != SLIDEO_YUV_CHROMA_NEAREST) h->check(slideo_group_set_yuv_chroma(h->g, yuv_chroma_));
        if (yuv_transfer_ != SLIDEO_YUV_TRANSFER_SDR) h->check(slideo_group_set_yuv_transfer(h->g, yuv_transfer_, yuv_white_nits_));
        if (pixel_format_ != SLIDEO_PIXEL_BGR8) h->check(slideo_group_set_pixel_format(h->g, pixel_format_));
        if (!shading_.empty()) h->check(slideo_group_set_frame_shading(h->g, shading_aw_, shading_ah_, shading_cell_, shading_.data()));
        if (!frame_levels_.empty()) h->check(slideo_group_set_frame_levels(h->g, frame_levels_.data()));
        if (mask_scope_ != SLIDEO_MASK_DETECT) h->check(slideo_group_set_frame_mask_scope(h->g, mask_scope_));
        if (!mask_.empty()) h->check(slideo_group_set_frame_mask(h->g, mask_.data(), mask_w_, mask_h_, mask_w_));
        if (direct_scope_ != SLIDEO_DIRECT_WHOLE) h->check(slideo_group_set_direct_scope(h->g, direct_scope_));
        if (direct_t_ != 0.f) h->check(slideo_group_set_direct_similarity(h->g, direct_t_));
        h->check(slideo_group_set_progress(h->g, detail::tramp, &reporter));                         // "Analyzing PDF pages..." protocol, mo/lib.rs:43-58
        const size_t CH = 32 * (size_t)h->n_devices;
        for (size_t i = 0; i < images.size(); i += CH) {
            std::vector<Image8> dec;
            for (size_t j = i; j < std::min(images.size(), i + CH); ++j) dec.push_back(loader_(images[j].get_path()));
            std::vector<const uint8_t*> ptrs; std::vector<int32_t> w, hh, st;
            for (auto& d : dec) { ptrs.push_back(d.bgr.data()); w.push_back(d.w); hh.push_back(d.h); st.push_back(d.w * 3); }
            h->check(slideo_group_add_pages_bgr8(h->g, (int32_t)dec.size(), ptrs.data(), w.data(), hh.data(), st.data()));
        }
        h->check(slideo_group_set_progress(h->g, nullptr, nullptr));
        h->check(slideo_group_finalize_pages(h->g));                                              // FlannMatcher::new, mo/flann.rs:65-71
        return std::make_unique<HipVideoMatcher<I>>(h, std::make_shared<std::vector<I>>(std::move(images)));
    }
private:
    std::vector<int32_t> devices_;
    bool sift_on_ = false, gated_ = true;
    float sift_ratio_ = 0.f, direct_t_ = 0.f;
    int32_t work_w_ = 0, work_h_ = 0;
    int32_t reg_sw_ = 0, reg_sh_ = 0, reg_ow_ = 0, reg_oh_ = 0;
    double reg_M_[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    int32_t lens_sw_ = 0, lens_sh_ = 0;
    double lens_cx_ = 0, lens_cy_ = 0, lens_f_ = 0, lens_k1_ = 0, lens_k2_ = 0;
    std::vector<uint8_t> mask_;
    int32_t mask_w_ = 0, mask_h_ = 0;
    int32_t yuv_matrix_ = SLIDEO_YUV_MATRIX_BT601, yuv_range_ = SLIDEO_YUV_RANGE_LIMITED, yuv_depth_ = SLIDEO_YUV_DEPTH_8;
    int32_t yuv_sampling_ = SLIDEO_YUV_SAMPLING_420;
    int32_t yuv_chroma_ = SLIDEO_YUV_CHROMA_NEAREST;
    int32_t yuv_transfer_ = SLIDEO_YUV_TRANSFER_SDR;
    float yuv_white_nits_ = 0.f;
    int32_t pixel_format_ = SLIDEO_PIXEL_BGR8;
    std::vector<uint8_t> frame_levels_;
    std::vector<uint16_t> shading_;
    int32_t shading_aw_ = 0, shading_ah_ = 0, shading_cell_ = 0;
    uint32_t mask_scope_ = SLIDEO_MASK_DETECT, direct_scope_ = SLIDEO_DIRECT_WHOLE, gate_ref_ = SLIDEO_GATE_PREVIOUS;
    uint32_t gate_order_ = SLIDEO_GROUP_GATE_HALO;
    float settle_similarity_ = 0.f;
    int32_t settle_max_defer_ = 0;
    int32_t gate_memory_ = 0;
    slideo_config cfg_;
    ImageLoader loader_;
};

}  // namespace slideo_host
