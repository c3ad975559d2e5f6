/*
 * slideo_amd.h — C ABI of the MI355X-native slide <-> video-frame matcher.
 *
 * This is the drop-in boundary for the hot path of hediet/slideo's
 * crates/matching-opencv.  The reference has no C ABI of its own (its only FFI
 * is the `opencv` crate's generated shims into OpenCV 4.5.2); each entry point
 * below names the reference call it replaces.  Paths are relative to the
 * reference repository root, shorthand `mo/` = crates/matching-opencv/src/.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++/torch types cross this boundary;
 *   - every function returns int32_t status (SLIDEO_OK == 0); the message for
 *     the last failure on a handle is slideo_last_error(handle);
 *   - the reference surface has no Result anywhere (it panics, mo/lib.rs:95-104,
 *     mo/flann.rs:15-46); a binding mirrors that by panicking on status != 0;
 *   - no C++ exception crosses the ABI;
 *   - images are 8-bit, 3 channels, BGR interleaved, row-major with a byte
 *     stride (the cv::Mat 8UC3 layout the reference holds, mo/lib.rs:77-83);
 *     the frame entry points also come as *_yuv420 twins that take decoded
 *     YUV 4:2:0 frames (NV12 / NV21 / I420 / YV12, section "YUV 4:2:0 frames";
 *     BT.709, full range and 10-bit samples: section "YUV colour description");
 *   - "page" = one rasterised PDF page, "frame" = one decoded video frame,
 *     page indices are 0-based positions in the order pages were added.
 *   - there is NO CPU fallback: without a gfx950 device every compute entry
 *     point fails with SLIDEO_ERR_NO_DEVICE;
 *   - a matcher is NOT re-entrant: calls on one handle must come from one thread at
 *     a time (the reference's caller is single threaded, crates/app/src/main.rs:77-93,
 *     and parallelism lives inside the call); different handles are independent.
 *
 * Limits (each is checked; beyond it the call fails with SLIDEO_ERR_UNSUPPORTED and says which one — nothing is clamped):
 *   image width / height   1..4096        x and y of a FAST candidate travel packed in 12 bits each (geom.h MAX_DIM); the
 *                                         reference's inputs are <= 1920x1080 video frames and 2001x1125 renders, the 4K
 *                                         config is 3840x2160
 *   train descriptors      < 2^23         a k-NN key is distance << 23 | row; 500 pages x ~1850 = 0.92 M rows, 4000 pages fit
 *   pages                  <= 16384       the vote kernel keeps one counter per page in LDS
 *   knn_k                  1..32          the per-query list lives in registers (the reference uses 30)
 *   max_candidate_pages    1..64, max_rated 1..16, nlevels 1..16, ransac_max_iters 1..1000000
 *   lsh_tables 1..8, lsh_key_bits 1..16, lsh_multi_probe 0..2 (matcher 1)
 *   page / frame area      >= small_area  to_small_image (mo/image_utils.rs:8-20) only ever SHRINKS here; for an image below
 *                                         120 000 px OpenCV's INTER_AREA turns into a bilinear upscale, which is not restated
 *                                         (the reference's frames are >= 640x360)
 *   NOT limits: keypoints per frame (beyond 8192 the canonical sort moves from LDS to global memory; a frame beyond the
 *   capacity the asynchronous path provides for is re-run through the exact-size path), the RANSAC sample schedule (the
 *   pre-drawn cv::RNG stream is extended on demand), frames per call (cut into units that fit the workspace budget).
 *
 * Environment (read by slideo_matcher_create unless marked "per unit"; NONE changes a result — they select between code paths
 * that the tests hold bit-identical, or size workspaces; everything else that used to be switchable this way was removed):
 *   SLIDEO_KNN_ENGINE 0..3        initial value of slideo_matcher_set_knn_engine
 *   SLIDEO_KNN_SHARE=0 / 1        exact Hamming search: always two / always one block per CU (default: one while other units are in flight)
 *                      =3 / 4    the 12-wave block (three search waves per SIMD, one block per CU) while other units are in flight / always
 *   SLIDEO_KNN_W12_RATIO x        default rule: that 12-wave block while units share the chip when a unit carries >= x (query, train row) pairs per frame
 *                                 pixel (290: decks of ~750 pages x ORB-1000 and up at 1080p; 0 = never) — the fuller matrix pipe then outweighs the
 *                                 co-runners' occupancy (configs[3] + 6.8 %, configs[4] + 4.7 %; headline - 2..4 %, hence the rule)
 *   SLIDEO_KNN_DEDUP=0            search all M train rows instead of the distinct ones (slideo_matcher_unique_descriptor_count)
 *   SLIDEO_LSH_ENGINE=gather      matcher 1 by bucket gathering instead of the filtered matrix-core stream
 *   SLIDEO_ASYNC_SUBMIT=0         units through the exact-size path (one host wait for the keypoint counts in mid-unit)
 *   SLIDEO_ORB_CHAIN=0            ORB stages of consecutive units free-running instead of taking turns
 *   SLIDEO_STREAM_PICK=0          the slots' streams in plain creation order instead of picked by measurement to sit on hardware queues of their own (below)
 *   SLIDEO_RESIZE_GENERIC=1       every pyramid level through resize_kernel (any shrink factor) instead of resize_quad_kernel [per unit]
 *   SLIDEO_HOST_UNIT n            frames per unit of a host-memory batch (32; 0 = the device-path rule)
 *   SLIDEO_WS_GB x                workspace budget of all slots together (48)
 *   SLIDEO_SIFT_WS_MB n           SIFT pyramid budget per pass (98304 on a device with >= 192 GB, else 24576)  [per call]
 *   SLIDEO_SIFT_LIST_CAP n        start capacity of SIFT's per-frame extrema list (65536; the tests force its growth path) [per call]
 *   SLIDEO_RNG_STREAM_LEN n       start length of the pre-drawn cv::RNG stream (the tests force its growth path)
 *   SLIDEO_EVIDENCE_MAX_FRAMES n  the frames limit of an evidence session, read at evidence_begin, 1..2^20 (the tests reach the refusal with it)
 *   SLIDEO_TONE_MAX_FRAMES n      the frames limit of a tone session, read at tone_begin, 1..2^31 (the tests reach the refusal with it)
 *   SLIDEO_PLACEMENT_MAX_FRAMES n the frames limit of a placement session, read at placement_begin, 1..2^20 (the tests reach the refusal with it)
 *   SLIDEO_SHADING_MAX_FRAMES n  the frames limit of a shading session, read at shading_begin, 1..2^20 (the tests reach the refusal with it)
 *   SLIDEO_RANSAC_WINDOW=0        ransac_kernel's redraw schedule by the fixed point only                       [per unit]
 *   SLIDEO_RH_TAIL_ROUNDS n       verify_model 1: rounds before a candidate moves to ransac_h_tail_kernel (256; 0 = never) [per unit]
 *   SLIDEO_REFINE_LANE_LM 0|1     verify_model 1: the small candidates' LM in refine_h_kernel<1> / in the eigen kernel's lanes [per unit]
 *   (not the library's, but it decides how its streams run) GPU_MAX_HW_QUEUES — the HIP runtime maps a process's streams onto this many
 *       hardware queues (default 4) in creation order, and a matcher's four slot streams must not share one (their units' kernels would
 *       serialise: - 10 %, measured behind an initialised RCCL communicator, whose streams come first: profiles/r06_experiments.txt 6).
 *       slideo_matcher_create therefore PICKS its slot streams by measurement (a candidate is kept iff a kernel on it completes while spin
 *       kernels keep the streams kept so far busy; a few ms); with fewer hardware queues than slots it takes what there is.
 *   build time only: SLIDEO_HIP_EXTRA_FLAGS (slideo_amd/build.py), SLIDEO_LIB_PATH / SLIDEO_REBUILD (slideo_amd/_capi.py)
 */
#ifndef SLIDEO_AMD_H
#define SLIDEO_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SLIDEO_ABI_VERSION 7

enum {
    SLIDEO_OK = 0,
    SLIDEO_ERR_INVALID_ARG = 1,   /* null pointer, bad size, bad config        */
    SLIDEO_ERR_NO_DEVICE = 2,     /* no HIP device / not gfx950                */
    SLIDEO_ERR_HIP = 3,           /* a HIP runtime call failed                 */
    SLIDEO_ERR_STATE = 4,         /* call order violated (e.g. match before finalize) */
    SLIDEO_ERR_UNSUPPORTED = 5,   /* config outside what the kernels implement */
    SLIDEO_ERR_EMPTY_INDEX = 6,   /* no page produced a descriptor (reference: FLANN train on empty set throws, mo/flann.rs:45-47) */
    SLIDEO_ERR_CAPACITY = 7       /* caller-provided output buffer too small   */
};

/* OpenCV-semantics switches.  The arithmetic of the reference's hot path lives in OpenCV 4.5.2 C++
 * (Cargo.lock:1723-1724, .github/workflows/ci.yml:18), whose source is neither under the reference
 * repository nor in this image; every primitive whose exact rounding could only be RECALLED (SURVEY.md
 * Appendix A, confidence M / L) is therefore restated in more than one form, selected here, shared by the
 * kernels' host tables (csrc/geom.h) and by the CPU restatement (oracle/).  Value 0 is the default of every switch that
 * restates a call the reference makes = the best estimate of what a stock 4.5.2 build (SSE3 baseline, AVX2 dispatch, IPP on:
 * ci/install-bionic.sh) runs for it; DESIGN.md section 5 says why.  (`hdlt`, which belongs to an extension the reference never
 * runs, defaults to 1: see there.)  tools/pin_opencv.py dumps OpenCV's own
 * outputs where cv2 4.5.2 exists, and tests/test_opencv_pin.py then names the matching value of each switch.
 * The HIP library implements the values marked [hip]; others fail slideo_matcher_create with
 * SLIDEO_ERR_UNSUPPORTED (the CPU restatement implements all of them). */
typedef struct slideo_ocv_variants {
    /* cvtColor(BGR2GRAY) inside ORB::detectAndCompute, mo/feature_extractor.rs:32-40 [OCV A.1]
     *   0 [hip] Q15 coefficients 3735/19235/9798, (x + 2^14) >> 15   (4.x color_rgb.simd.hpp)
     *   1 [hip] Q14 coefficients 1868/9617/4899,  (x + 2^13) >> 14   (2.4 / 3.x)                      */
    int32_t gray;
    /* GaussianBlur(level, 7x7, sigma 2, BORDER_REFLECT_101) inside ORB, same call [OCV A.6].  ORB blurs a
     * SUBMATRIX of its pyramid buffer, which GaussianBlur's fixed-point branch excludes
     * (smooth.dispatch.cpp: `sdepth == CV_8U && ((borderType & BORDER_ISOLATED) || !src.isSubmatrix())`), so the
     * call falls through to sepFilter2D with the CV_32F kernel:
     *   0 [hip] sepFilter2D in f32 (4.2+: createBitExactKernel_32S rejects a kernel whose taps x 256 are not
     *           integers): row pass k0*p0 then += k_i*p_i, column pass k3*c then += k_j*(r_+j + r_-j),
     *           saturate_cast<uchar>(cvRound); products CONTRACTED to fma (the AVX2-dispatched filter.avx2.cpp
     *           of a stock build is compiled with -mfma and GCC's default -ffp-contract=fast)
     *   1 [hip] the same without contraction (hosts without AVX2, or baseline-only builds)
     *   2 [hip] sepFilter2D in Q8 integers (before 4.2: taps cvRound(k * 256) = 18 34 49 55 49 34 18, sum 257),
     *           (sum + 2^15) >> 16, saturated
     *   3 [hip] GaussianBlur's bit-exact fixed-point path (what a non-submatrix source takes): error-diffused
     *           taps 18 34 48 56 48 34 18 (sum 256), (sum + 2^15) >> 16                                */
    int32_t blur;
    /* resize(prev level, INTER_LINEAR_EXACT) inside ORB [OCV A.2]: rounding of the 8.8 coefficient
     *   0 [hip] cvRound(frac * 256), ties to even (softdouble -> ufixedpoint16)
     *   1 [hip] floor(frac * 256 + 0.5), ties up                                                      */
    int32_t resize;
    /* fastAtan2 in ORB's ICAngles [OCV A.5]: the odd degree-7 polynomial
     *   0 [hip] plain f32 multiplies and adds (scalar baseline code, SSE3: no fma)
     *   1 [hip] the Horner steps contracted to fma (a build whose BASELINE has FMA3)                  */
    int32_t atan;
    /* warpAffine(nearest, WARP_INVERSE_MAP), mo/lib.rs:339-347 [OCV A.10]
     *   0 [hip] 10-bit fixed point: (saturate<int>(M0 x * 1024) + saturate<int>((M1 y + M2) * 1024) + 512) >> 10
     *   1       cvRound of the f64 coordinate M0 x + M1 y + M2 (no fixed point; definitional cross-check) */
    int32_t warp;
    /* resize(INTER_AREA) tap construction, mo/image_utils.rs:17 [OCV A.11]
     *   0 [hip] computeResizeAreaTab: f32 weights, edge taps dropped below 1e-3 of a source cell
     *   1 [hip] exact box-overlap weights, no cut-off (definitional cross-check)                      */
    int32_t area;
    /* Levenberg-Marquardt step of estimateAffinePartial2D's refinement, mo/image_utils.rs:52 [OCV A.9]
     *   0 [hip] damped normal equations by Gaussian elimination with partial pivoting
     *   1       by Jacobi eigen-decomposition + back-substitution (cv::solve(DECOMP_EIG)); equal to f64 round-off */
    int32_t lm;
    /* cv::RNG multiplier (RANSAC sample schedule [OCV A.9], BRIEF pattern [OCV A.7]); any value [hip] */
    uint32_t rng_mul;             /* 4164903690 */
    /* verify_model 1 only: the homography of a point set, HomographyEstimatorCallback::runKernel of
     * calib3d/src/fundam.cpp (recalled; no counterpart in the reference, which never fits a homography)
     * DEFAULT 1 since ABI 6: the three forms give identical verdicts, survivals and inlier counts on all 9000 candidates of
     * the headline shape (profiles/r04_hdlt_agreement.json; form 2: 99.98 %), form 0 costs 7.5x the whole step, and there
     * is no reference behaviour to be faithful to — 0 stays as the switch for fidelity to cv::findHomography's rounding.
     *   0 [hip] normalised DLT: centroid / mean-absolute-deviation normalisation, the 9x9 normal matrix L^T L
     *           accumulated in f64, cv::eigen = the Jacobi sweep of core/src/lapack.cpp (JacobiImpl_, pivot =
     *           largest off-diagonal element, its own hypot), H = the eigenvector of the smallest eigenvalue,
     *           de-normalised and scaled by 1 / H[8]
     *   1 [hip] minimal samples (4 pairs) only: the 8x8 system with h33 = 1 on the same normalised points by
     *           Gaussian elimination with partial pivoting; point sets of more than 4 pairs (the refit over the
     *           inliers) still take form 0.  Agrees with form 0 to f64 round-off (same samples, same masks in every
     *           test) at 1 / 60 of its cost: a RANSAC iteration of form 0 is a 9x9 eigen-decomposition (~140
     *           Jacobi rotations).  The fast choice when fidelity to cv::eigen's rounding is not the point.
     *   2 [hip] minimal samples only: the same model in closed form — the projective maps of the unit square onto the two
     *           normalised quadrilaterals (Heckbert), H = S_to * adj(S_from): ~90 multiplications and two divisions, no
     *           pivoting; again equal to f64 round-off, and the cheapest of the three. */
    int32_t hdlt;
} slideo_ocv_variants;

/* Every literal the reference hard-codes on the hot path, as one struct whose
 * defaults (slideo_config_default) equal those literals. */
typedef struct slideo_config {
    /* cv::ORB::create arguments, mo/feature_extractor.rs:13-23 */
    int32_t nfeatures;            /* 2000 */
    float   scale_factor;         /* 1.2f */
    int32_t nlevels;              /* 8    */
    int32_t edge_threshold;       /* 62   */
    int32_t patch_size;           /* 62   */
    int32_t fast_threshold;       /* 20   */
    /* matcher: k of knn_match, mo/lib.rs:266 */
    int32_t knn_k;                /* 30   */
    /* tolerance vote, mo/lib.rs:275 */
    float   vote_tolerance;       /* 1.05f */
    /* candidate pages kept, mo/lib.rs:295 */
    int32_t max_candidate_pages;  /* 40   */
    /* estimate_affine_partial_2d arguments, mo/image_utils.rs:52 */
    double  ransac_threshold;     /* 3.0  */
    int32_t ransac_max_iters;     /* 2000 */
    double  ransac_confidence;    /* 0.99 */
    int32_t refine_iters;         /* 10   */
    /* rating filter, mo/lib.rs:330,333 */
    int32_t max_rated;            /* 10   */
    double  min_rating;           /* 50.0 (strict >) */
    double  min_rating_ratio;     /* 0.2  (strict >) */
    /* verdict, mo/lib.rs:381 */
    float   min_similarity;       /* 0.5f (strict >) */
    /* to_small_image, mo/image_utils.rs:11 */
    int32_t small_area;           /* 300*400 */
    /* MarkSimilarIter, mo/video_capture.rs:98 */
    float   changed_similarity;   /* 0.98f (changed <=> similarity < this) */
    /* Extension with no reference counterpart (BASELINE.json north_star / configs[1] wording): 0 = off, the
     * reference's tolerance vote above.  r > 0 replaces it by the ratio test on the two nearest neighbours:
     * a query votes for its nearest row iff it has a second neighbour and (float)d1 < r * (float)d2 (f32,
     * strict); needs knn_k >= 2. */
    float   ratio_test;           /* 0.0f */
    /* Extension with no reference counterpart (BASELINE.json north_star "RANSAC homography verification",
     * configs[4]): the geometric model of the verification step.
     *   0 = the reference's estimateAffinePartial2D (4-DOF similarity, 2-point samples, mo/image_utils.rs:45-60)
     *       followed by warpAffine (mo/lib.rs:339-347);
     *   1 = an 8-DOF homography: what cv::findHomography(from, to, RANSAC, ransac_threshold, mask,
     *       ransac_max_iters, ransac_confidence) computes (calib3d/src/fundam.cpp, recalled: 4-point samples drawn
     *       by RANSACPointSetRegistrator::getSubset with HomographyEstimatorCallback::checkSubset, normalised DLT,
     *       f32 re-projection error, the same cv::RNG(-1) schedule and sequential acceptance as the similarity
     *       path, then — refine_iters > 0 and more than 4 pairs — a DLT over all inliers and refine_iters
     *       Levenberg-Marquardt steps on the 8 parameters; the mask is not recomputed), followed by
     *       warpPerspective(nearest, WARP_INVERSE_MAP) (imgproc/src/imgwarp.cpp) in the re-projection. */
    int32_t verify_model;         /* 0 */
    /* The descriptor index.  0 = exact brute-force Hamming k-NN (north_star; what this library is built around).
     * 1 = LSH-compatible approximate search: the candidate rule of the index the reference really builds —
     * FlannBasedMatcher over FLANN's LshIndex with table_number 6, key_size 12, multi_probe_level 1 (mo/flann.rs:14-26):
     * lsh_tables hash tables, each keyed by lsh_key_bits descriptor bits (cv::randShuffle of the 256 bit positions on
     * cv::RNG's default state, the first lsh_key_bits of it, as flann/lsh_table.h does — recalled), a train row is a
     * CANDIDATE of a query iff in some table its key differs from the query's in at most lsh_multi_probe bits; the
     * result is the knn_k nearest candidates by (distance, row).  (FLANN's KNNUniqueResultSet breaks distance ties
     * at the k-th place by visiting order; here ties go to the lower row: canonical)  Recall < 1, like
     * the reference's; `SearchParams.checks` (32, mo/flann.rs:21) is ignored by LshIndex and has no counterpart. */
    int32_t matcher;              /* 0 */
    int32_t lsh_tables;           /* 6  (mo/flann.rs:16) */
    int32_t lsh_key_bits;         /* 12 (mo/flann.rs:17) */
    int32_t lsh_multi_probe;      /* 1  (mo/flann.rs:18) */
    /* Opt-in DEPARTURE from the reference's verdict (mo/lib.rs:370-389: survivors sorted by re-projection similarity, the
     * first above min_similarity wins).  0 = that rule.  1 = survivors keep their RATING order (inlier count descending, ties
     * in candidate order: mo/lib.rs:329) and the first whose similarity exceeds min_similarity wins — the similarity becomes
     * an acceptance test instead of the ranking.  Why it exists: with verify_model 1 a template-sharing sibling page
     * re-projects its shared template as well as the true page and wins by a few thousandths of similarity on ~13 % of the
     * synthetic headline frames, while the true page has the most inliers (DESIGN.md section 5 has the measured effect). */
    int32_t verdict_rule;         /* 0 */
    /* which restatement of each OpenCV primitive to run.  Defaults: all 0 EXCEPT hdlt = 1 (ABI 6), rng_mul 4164903690 — obtain
     * them from slideo_config_default: a zero-initialised ocv selects hdlt 0, a different (60x slower) form than the default */
    slideo_ocv_variants ocv;
} slideo_config;

/* cv::KeyPoint as the reference consumes it (pt, size, angle, response,
 * octave); class_id is never read (mo/lib.rs:299-302). 24 bytes. */
typedef struct slideo_keypoint {
    float   x, y;       /* level-0 pixel coordinates                         */
    float   size;       /* patch_size * scale(octave)                        */
    float   angle;      /* degrees, [0,360)                                  */
    float   response;   /* FAST score                                        */
    int32_t octave;     /* pyramid level                                     */
} slideo_keypoint;

/* One per-frame verdict = the `image: Option<I>` of matching::Matching
 * (crates/matching/src/lib.rs:35-40) plus the two numbers that decided it. */
typedef struct slideo_verdict {
    int32_t page_idx;     /* -1 = None                                        */
    float   similarity;   /* of the winning page, 0 when page_idx == -1       */
    int32_t inliers;      /* RANSAC inlier count of the winning page, else 0  */
    int32_t n_keypoints;  /* ORB keypoints found in the frame                 */
} slideo_verdict;

typedef struct slideo_matcher slideo_matcher;

/* matching::ProgressReporter (crates/matching/src/progress.rs:3-17).  May be
 * invoked from any thread; the reference invokes it from rayon workers
 * (mo/lib.rs:49-53,192-203). */
typedef void (*slideo_progress_fn)(void* user, uint64_t done, uint64_t total, const char* msg);

uint32_t    slideo_abi_version(void);

/* Fills *cfg with the reference's literals (table above). */
void        slideo_config_default(slideo_config* cfg);

/* Replaces OpenCVImageVideoMatcher::default() + FeatureExtractor::default()
 * (crates/app/src/main.rs:69; mo/feature_extractor.rs:12-27).
 * device: HIP device ordinal. */
int32_t     slideo_matcher_create(const slideo_config* cfg, int32_t device, slideo_matcher** out);
void        slideo_matcher_destroy(slideo_matcher* m);

/* Message of the last failure on `m` (or of the last failed create when m is
 * NULL).  Never NULL; valid until the next call on the same handle. */
const char* slideo_last_error(const slideo_matcher* m);

/* Replaces ProcessedImage::compute over all pages (mo/lib.rs:45-56,92-131):
 * ORB detect+describe and to_small_image per page.  Host buffers.  May be
 * called repeatedly before finalize; pages keep their add order. */
int32_t     slideo_matcher_add_pages_bgr8(slideo_matcher* m, int32_t n_pages,
                                          const uint8_t* const* data,
                                          const int32_t* width, const int32_t* height,
                                          const int32_t* stride_bytes);

/* The page side of ProcessedImage (mo/lib.rs:77-83) computed elsewhere — by another rank that analysed a share of the deck
 * (the page-sharded build of SURVEY.md section 8e: ranks all-gather these records instead of each analysing every page) or by
 * an earlier run (the reference caches per-PDF state, crates/app/src/db.rs).  Appends ONE page: its size, its keypoints and
 * descriptors in canonical order (as slideo_matcher_get_page_features returns them) and its small image (as
 * slideo_matcher_get_page_small returns it; small_w x small_h x 3 bytes, must be the to_small_image size of the page).
 * A matcher built from imported pages behaves exactly like one that analysed the images itself. */
int32_t     slideo_matcher_add_page_features(slideo_matcher* m, int32_t width, int32_t height, int32_t n_keypoints,
                                             const slideo_keypoint* kp, const uint8_t* desc32,
                                             const uint8_t* small_bgr, int32_t small_w, int32_t small_h);
/* Copies page `page_idx`'s small image (to_small_image, mo/lib.rs:128) to host; *sw, *sh receive its size. */
int32_t     slideo_matcher_get_page_small(const slideo_matcher* m, int32_t page_idx, uint8_t* out, int64_t out_capacity,
                                          int32_t* sw, int32_t* sh);

/* Replaces FlannMatcher::new (mo/flann.rs:65-71; add :28-34, train :45-47):
 * freezes the page descriptor set into the device-resident train matrix. */
int32_t     slideo_matcher_finalize_pages(slideo_matcher* m);

int32_t     slideo_matcher_page_count(const slideo_matcher* m);
/* Total descriptors over all pages (M).  -1 before finalize. */
int64_t     slideo_matcher_descriptor_count(const slideo_matcher* m);
/* Distinct descriptors among them (<= M).  The matcher's k-NN stage searches these and then restores, exactly, what a search
 * over all M rows returns (csrc/knn.hip.h knn_expand_dups_kernel): FlannMatcher::knn_match returns every matching row
 * (mo/flann.rs:73-89) and the vote counts per row (mo/lib.rs:268-282), so equal rows of different pages all vote.  Decks
 * repeat templates: 21 % of the rows of the 500-page benchmark deck are duplicates.  -1 before finalize. */
int64_t     slideo_matcher_unique_descriptor_count(const slideo_matcher* m);
/* Copies page `page_idx`'s keypoints/descriptors (canonical order) to host. */
int32_t     slideo_matcher_get_page_features(const slideo_matcher* m, int32_t page_idx,
                                             slideo_keypoint* kp, uint8_t* desc32,
                                             int32_t capacity, int32_t* n_out);

/* Replaces OpenCVVideoMatcherTask::match_images_with_frame (mo/lib.rs:249-413)
 * for a batch of equally sized frames held in HOST memory; verdicts to host. */
int32_t     slideo_match_frames_bgr8(slideo_matcher* m, int32_t n_frames,
                                     const uint8_t* frames, int32_t width, int32_t height,
                                     int32_t stride_bytes, int64_t frame_stride_bytes,
                                     slideo_verdict* verdicts_out);

/* Same, frames already resident in HBM (device pointer); verdicts to host.
 * `hip_stream` is a hipStream_t (NULL = the matcher's own stream). */
int32_t     slideo_match_frames_bgr8_dev(slideo_matcher* m, int32_t n_frames,
                                         const uint8_t* frames_dev, int32_t width, int32_t height,
                                         int32_t stride_bytes, int64_t frame_stride_bytes,
                                         slideo_verdict* verdicts_out, void* hip_stream);

/* Streaming form of the same call for callers that keep the GPU fed: submit a unit of frames (device
 * memory, must stay valid until collected), later collect its verdicts.  At most
 * slideo_matcher_max_in_flight() units (4) are in flight; each runs on its own internal stream and workspace
 * slot so that the ORB and verification stages of some units share the GPU with the matrix-core bound kNN of
 * others (the reference gets the same effect from rayon's work stealing, mo/lib.rs:174,213).  Tickets must
 * be collected in submission order.  The synchronous entry points above use the same machinery on two
 * halves of their batch. */
int32_t     slideo_matcher_max_in_flight(const slideo_matcher* m);
int32_t     slideo_match_frames_submit_dev(slideo_matcher* m, int32_t n_frames,
                                           const uint8_t* frames_dev, int32_t width, int32_t height,
                                           int32_t stride_bytes, int64_t frame_stride_bytes,
                                           void* hip_stream, int64_t* ticket_out);
int32_t     slideo_match_frames_collect(slideo_matcher* m, int64_t ticket, slideo_verdict* verdicts_out);
/* The same, and the unit's verdict records are also left in caller-provided DEVICE memory (n_frames records of
 * slideo_verdict, complete when the call returns): what a multi-GPU caller hands to its one all-gather of verdicts
 *  without a host round trip.  verdicts_dev_out may be NULL. */
int32_t     slideo_match_frames_collect_dev(slideo_matcher* m, int64_t ticket, slideo_verdict* verdicts_out, void* verdicts_dev_out);

/* Replaces MarkSimilarIter (mo/video_capture.rs:86-98) for a run of sampled
 * frames in host memory: changed[i] = 1 iff similarity(small(frame i-1),
 * small(frame i)) < cfg.changed_similarity; the first frame compares against
 * `prev_small` (w*h*3 small image returned by an earlier call) or, when that
 * is NULL, is always changed.  similarity_out may be NULL. */
int32_t     slideo_changed_mask_bgr8(slideo_matcher* m, int32_t n_frames,
                                     const uint8_t* frames, int32_t width, int32_t height,
                                     int32_t stride_bytes, int64_t frame_stride_bytes,
                                     const uint8_t* prev_small, uint8_t* last_small_out,
                                     uint8_t* changed_out, float* similarity_out);

/* The frames of the LAST slideo_changed_mask_bgr8 call are still on the device when it returns.  This matches a subset of
 * them — sel[i] = index into that call's frames, ascending or not — exactly as slideo_match_frames_bgr8 would match the same
 * frames, without uploading them a second time: what OpenCVVideoMatcherTask::process does with the frames MarkSimilarIter
 * flagged as changed (mo/lib.rs:205-214).  Must directly follow the mask call on this handle (any other call that uploads
 * frames invalidates the kept ones: SLIDEO_ERR_STATE). */
int32_t     slideo_match_kept_frames(slideo_matcher* m, int32_t n_sel, const int32_t* sel, slideo_verdict* verdicts_out);

/* Optional: page-lock a frame buffer the caller reuses across calls (hipHostRegister / hipHostUnregister), so that the H2D
 * copies read it by DMA directly.  Not needed for correctness; pageable memory is staged by the runtime. */
int32_t     slideo_host_register(void* ptr, size_t bytes);
int32_t     slideo_host_unregister(void* ptr);

/* Optional progress sink for add_pages / match_frames. */
int32_t     slideo_matcher_set_progress(slideo_matcher* m, slideo_progress_fn fn, void* user);


/* ---- page sets (extension: the reference has no counterpart; its README advises one invocation per PDF instead) ------------
 * A page set S is a non-empty set of deck page indices of a finalized matcher.  A frame call made while S is selected searches
 * S's pages only, and every result — slideo_verdict (page, similarity, inliers, keypoints) and the slideo_last_frame_candidates
 * trace (votes, inliers, survived, similarity, transform) — equals, bit for bit, what a REFERENCE SUB-MATCHER returns for the
 * same frames: a matcher of the same config built from exactly S's pages in ascending deck order (slideo_matcher_add_page_features
 * with this matcher's slideo_matcher_get_page_features / slideo_matcher_get_page_small output), its page index j mapped to the
 * j-th smallest index of S.  (Keys carry deck row ids, which keep the sub-matcher's row order; candidates tie by ascending page,
 * which the map keeps; duplicate rows are chained within S only, so a descriptor shared with an unselected page votes for the
 * selected one alone.)  A set is a second search operand plus a second duplicate chain, built on the device from the finalized
 * deck in a few launches (csrc/stage_page_set.hip); the deck's pages, keypoints and small images are shared.
 * Set 0 is the whole deck and the default: a matcher that never selects a set behaves as before.  The selection is state of the
 * matcher that every frame call reads (BGR and YUV 4:2:0, host and device, sync and submit / collect, slideo_match_kept_frames).
 * Sets cover the exact Hamming search (matcher 0) with engines 0 / 2 / 3; LSH (matcher 1), slideo_matcher_use_sift and the VALU
 * engine (set_knn_engine(1)) are refused with SLIDEO_ERR_UNSUPPORTED at slideo_matcher_use_page_set or at the first frame call
 * under a set, whichever comes first (slideo_matcher_create_page_set refuses LSH and SIFT matchers too).
 * Status: SLIDEO_ERR_STATE before finalize; SLIDEO_ERR_INVALID_ARG for n_pages < 1, an index out of range or listed twice, an
 * unknown set id (and set 0 in release); SLIDEO_ERR_EMPTY_INDEX when the selected pages hold no descriptor; SLIDEO_ERR_STATE for
 * releasing the selected set or a set an uncollected unit searches; SLIDEO_ERR_UNSUPPORTED beyond 64 live sets. */
/* After finalize.  pages: n_pages distinct deck indices, any order.  *set_out >= 1 (ids are not reused). */
int32_t     slideo_matcher_create_page_set(slideo_matcher* m, int32_t n_pages, const int32_t* pages, int32_t* set_out);
/* Units submitted from now on search `set` (0 = whole deck).  Units already in flight keep theirs. */
int32_t     slideo_matcher_use_page_set(slideo_matcher* m, int32_t set);
int32_t     slideo_matcher_release_page_set(slideo_matcher* m, int32_t set);
/* Selected pages, their descriptor rows, the distinct rows among them (what the search streams), device bytes the set's operand
 * and chain hold.  Set 0: the deck's.  Any output may be NULL. */
int32_t     slideo_matcher_page_set_info(const slideo_matcher* m, int32_t set, int32_t* n_pages, int64_t* rows, int64_t* unique_rows,
                                         int64_t* bytes);

/* ---- measurement ---------------------------------------------------------- */

/* Stage timing with HIP events recorded on the stream the kernels are launched
 * on (bench.py's roofline figures come from here).  enable != 0 starts
 * accumulating; reading returns and clears the accumulators.  Stages:
 *   0 orb (gray..describe)  1 knn (knn_hamming_kernel [+ merge])  2 verify
 *   (vote, ransac, rate, reproject, verdict)  3 whole sub-batch incl. copies.
 * launches_out[i] = number of timed intervals of stage i; for stage 1 each
 * interval is exactly one knn_hamming_kernel launch (+ its merge when split). */
/* kNN engine: 0 = FP4 matrix cores, wave shape chosen per launch (default), 1 = integer-VALU popcount kernel,
 * 2 = FP4 matrix cores forced to 2 waves per SIMD x 4 query tiles per wave (leaves half of every SIMD's registers
 * and 96 KB of LDS per CU to the kernels of the other unit in flight; what 0 picks when the queries fill the chip),
 * 3 = forced to 4 waves per SIMD x 2 query tiles per wave (what 0 picks for smaller query sets).
 * All are exact and return identical results; the switch exists for A/B measurement. */
int32_t     slideo_matcher_set_knn_engine(slideo_matcher* m, int32_t engine);

/* The matcher's kNN stage is fused with the acceptance rule of its only consumer, the tolerance vote
 * (mo/lib.rs:268-282: a neighbour counts iff d < best * 1.05): by default it keeps the k-NN lists exact only
 * for the neighbours that can still pass that test (every such neighbour, in canonical order), which spares
 * most of the list maintenance.  Verdicts, votes and candidates are identical either way; on != 0 makes the
 * stage keep the full exact k-NN lists (A/B measurement, tests).  slideo_knn_hamming is always exact. */
int32_t     slideo_matcher_set_knn_exact_lists(slideo_matcher* m, int32_t on);

#define SLIDEO_N_STAGES 4
int32_t     slideo_matcher_set_profiling(slideo_matcher* m, int32_t enable);
int32_t     slideo_matcher_read_profile(slideo_matcher* m, double* ms_out /*[4]*/,
                                        int64_t* launches_out /*[4]*/, int64_t* knn_pairs_out);
/* ABI 7.  The shader clock (MHz) the search kernel's waves ran at since profiling was switched on or this was last read:
 * wave 0 of every 8th search block sums its s_memtime (shader cycles) and s_memrealtime (100 MHz) deltas in device memory
 * (csrc/knn_tile.hip.h KtClock); *samples_out = the blocks that recorded (0: no search ran while profiling; *mhz_out is 0
 * then).  Measurement only (bench.py roofline.shader_clock_mhz): the chip clocks to its power budget, 2.1 - 2.3 of 2.4 GHz
 * under this load.  The matcher must be idle. */
int32_t     slideo_matcher_read_shader_clock(slideo_matcher* m, double* mhz_out, int64_t* samples_out);

/* ---- debug taps used by the parity tests ------------------------------ */

/* FeatureExtractor::find_keypoints_and_descriptors (mo/feature_extractor.rs:29-46)
 * on one host image.  Output in canonical order (octave, y, x).  *n_out is the
 * number found even when it exceeds `capacity` (then SLIDEO_ERR_CAPACITY). */
int32_t     slideo_orb_bgr8(slideo_matcher* m, const uint8_t* bgr, int32_t width, int32_t height,
                            int32_t stride_bytes, slideo_keypoint* kp, uint8_t* desc32,
                            int32_t capacity, int32_t* n_out);

/* Pyramid level `level` (gray, unblurred or blurred) of one host image; out is
 * lw*lh bytes, dimensions returned in *lw,*lh. */
int32_t     slideo_pyramid_level_bgr8(slideo_matcher* m, const uint8_t* bgr, int32_t width,
                                      int32_t height, int32_t stride_bytes, int32_t level,
                                      int32_t blurred, uint8_t* out, int64_t out_capacity,
                                      int32_t* lw, int32_t* lh);

/* Exact Hamming k-NN (replaces FlannMatcher::knn_match, mo/flann.rs:73-89 with
 * the brute-force search north_star asks for).  q: nq*32 bytes, t: nt*32 bytes
 * (host).  Out: idx[nq*k] (global train row, -1 padding when nt<k) and
 * dist[nq*k] (65535 padding), ascending by (distance, train row). */
int32_t     slideo_knn_hamming(slideo_matcher* m, const uint8_t* q, int32_t nq,
                               const uint8_t* t, int32_t nt, int32_t k,
                               int32_t* idx_out, uint16_t* dist_out);

/* The LSH-compatible search (slideo_config.matcher 1) as a tap: the k nearest (distance, row) among the rows of t that are
 * LSH candidates of each query under cfg's lsh_* parameters.  Same output format as slideo_knn_hamming. */
int32_t     slideo_knn_lsh(slideo_matcher* m, const uint8_t* q, int32_t nq, const uint8_t* t, int32_t nt, int32_t k,
                           int32_t* idx_out, uint16_t* dist_out);

/* North-star extension without a counterpart in the reference (BASELINE configs[2], SURVEY §8(d) "cfg2" / §8(f) N4):
 * exact squared-L2 k-NN between 128-dimensional u8 descriptors (SIFT-shaped: OpenCV's SIFT descriptors are
 * integer-valued 0..255), computed as an N x M x 128 integer contraction on the matrix cores
 * (v_mfma_i32_32x32x32_i8 on centred components).  q: nq x 128 bytes, t: nt x 128 bytes (nt < 2^23), 1 <= k <= 32.
 * idx_out[nq*k]: train row or -1; dist_out[nq*k]: squared distance (0xFFFFFFFF where idx is -1).  Neighbours in
 * ascending (distance, row) order — what cv::BFMatcher(NORM_L2).knnMatch would return up to the square root.
 * The parity target is this repository's CPU restatement (oracle so_knn_l2_u8). */
int32_t     slideo_knn_l2_u8(slideo_matcher* m, const uint8_t* q, int32_t nq, const uint8_t* t, int32_t nt, int32_t k,
                             int32_t* idx_out, uint32_t* dist_out);

/* The same search with the train set prepared once and kept on the device (what a SIFT matcher over a page DB would hold:
 * the counterpart of FlannMatcher::new for float descriptors) and queries / results in device memory.  kernel_ms (may be
 * null) receives the HIP-event time of the search kernels of this call.  bench.py --workload cfg2 times this. */
int32_t     slideo_l2_set_train(slideo_matcher* m, const uint8_t* t, int32_t nt);
int32_t     slideo_l2_knn_dev(slideo_matcher* m, const void* q_dev, int32_t nq, int32_t k, void* idx_dev /* i32 [nq*k] */,
                              void* dist_dev /* u32 [nq*k] */, float* kernel_ms);

/* ---- SIFT (north-star extension, BASELINE configs[2]; no counterpart in the reference, whose only extractor is ORB:
 * mo/feature_extractor.rs:3-4,13).  cv::SIFT::detectAndCompute of OpenCV 4.5.2 as restated in oracle/sift_oracle.h (the
 * parity target; its header lists the two documented departures): doubled first octave, nOctaveLayers + 3 Gaussian layers per
 * octave, DoG extrema with sub-pixel refinement, contrast and edge tests, orientation histogram (one keypoint per peak),
 * retainBest(nfeatures) by response with ties kept, 4 x 4 x 8 descriptors as 128 bytes (OpenCV's are integer-valued 0..255).
 * Keypoints come back in canonical order (octave, layer, row, column, orientation bin); `octave` holds OpenCV's packed field
 * (octave & 255 | layer << 8 | sub-layer << 16), x / y / size in input-image pixels.  The descriptors feed slideo_l2_knn_dev.
 * Limits: n_octave_layers must be 3; the sides of the image the extractor reads <= 4095 (the doubled image's coordinates travel
 * in 13 bits): pages, and frames after the working-size reduce — a 4096-wide frame is accepted under a working size that reduces
 * it ("Working size"). */
typedef struct slideo_sift_config {
    int32_t nfeatures;            /* 0 = keep every keypoint (cv::SIFT::create default)  */
    int32_t n_octave_layers;      /* 3    */
    double  contrast_threshold;   /* 0.04 */
    double  edge_threshold;       /* 10   */
    double  sigma;                /* 1.6  */
} slideo_sift_config;
void        slideo_sift_config_default(slideo_sift_config* cfg);
/* One host image.  *n_out = keypoints found even when it exceeds `capacity` (then SLIDEO_ERR_CAPACITY). */
int32_t     slideo_sift_bgr8(slideo_matcher* m, const slideo_sift_config* cfg, const uint8_t* bgr, int32_t width, int32_t height,
                             int32_t stride_bytes, slideo_keypoint* kp, uint8_t* desc128, int32_t capacity, int32_t* n_out);
/* A batch of equally sized frames in DEVICE memory -> keypoints and descriptors in DEVICE memory, frame after frame:
 * frame f owns rows [qofs_out[f], qofs_out[f + 1]) of kp_dev (slideo_keypoint) and desc_dev (128 bytes each).  qofs_out: n + 1
 * host values.  capacity_total rows must fit (else SLIDEO_ERR_CAPACITY).  kernel_ms (may be null): HIP-event time of the call's
 * kernels.  bench.py --workload cfg2 times this + slideo_l2_knn_dev. */
int32_t     slideo_sift_frames_dev(slideo_matcher* m, const slideo_sift_config* cfg, int32_t n_frames, const uint8_t* frames_dev,
                                   int32_t width, int32_t height, int32_t stride_bytes, int64_t frame_stride_bytes,
                                   int64_t capacity_total, void* kp_dev, void* desc_dev, uint32_t* qofs_out, float* kernel_ms);
/* Pyramid tap (parity tests): Gaussian layer (dog == 0, layer 0 .. 5) or difference layer (dog != 0, layer 0 .. 4) of `octave`. */
int32_t     slideo_sift_layer_bgr8(slideo_matcher* m, const slideo_sift_config* cfg, const uint8_t* bgr, int32_t width, int32_t height,
                                   int32_t stride_bytes, int32_t octave, int32_t layer, int32_t dog, float* out, int64_t out_capacity,
                                   int32_t* lw, int32_t* lh);

/* North-star / BASELINE configs[2] as a COMPLETE matcher (no reference counterpart: the reference extracts ORB only,
 * mo/feature_extractor.rs:3-4,13): SIFT-128 features instead of ORB for pages and frames, brute-force squared-L2 k-NN (k = 2) on
 * the int8 matrix cores with Lowe's ratio test — a query votes for its nearest row iff sqrt(d1) < ratio * sqrt(d2) (f32) —
 * instead of the Hamming k-NN + tolerance vote.  Everything from the per-page vote on (candidate ranking, RANSAC per
 * verify_model, rating, re-projection, verdict) and every entry point (add_pages, finalize, match_frames*, submit / collect,
 * changed mask + kept frames, the candidate trace) is the path's own.  Must be called before the first page is added; cfg as
 * for slideo_sift_bgr8 (nfeatures 0 = all keypoints), 0 < ratio <= 1.  ratio == 0: no ratio test — the path's own tolerance
 * vote (mo/lib.rs:268-282) on the knn_k nearest rows instead: a neighbour counts iff sqrt(d) < sqrt(d_best) * vote_tolerance
 * (f32), which — unlike Lowe's test — keeps the matches whose descriptor also sits on a twin page of the same template.
 * slideo_matcher_get_page_features (here 128 bytes per keypoint) works; slideo_matcher_
 * add_page_features (32-byte descriptors) returns SLIDEO_ERR_UNSUPPORTED in this mode; descriptor_count is the number of SIFT
 * rows.  Parity target: the oracle's so_db_use_sift + so_match_frame. */
int32_t     slideo_matcher_use_sift(slideo_matcher* m, const slideo_sift_config* cfg, float ratio);

/* to_small_image (mo/image_utils.rs:8-20) of one host image. */
int32_t     slideo_small_image_bgr8(slideo_matcher* m, const uint8_t* bgr, int32_t width,
                                    int32_t height, int32_t stride_bytes, uint8_t* out,
                                    int64_t out_capacity, int32_t* sw, int32_t* sh);

/* Per-frame trace of the decision steps for one frame of the LAST
 * slideo_match_frames_* call (parity tests compare these with the oracle). */
typedef struct slideo_candidate {
    int32_t page_idx;
    int32_t n_votes;      /* matches surviving the tolerance vote (mo/lib.rs:268-282) */
    int32_t inliers;      /* rating (mo/lib.rs:310)                                    */
    int32_t survived;     /* passed the rating filter (mo/lib.rs:333)                  */
    float   similarity;   /* mo/lib.rs:351, 0 when not computed                        */
    double  transform[9]; /* 3x3 row-major, slide -> frame; verify_model 0: rows 0-1 = the 2x3 of
                             estimateAffinePartial2D (mo/image_utils.rs:52), row 2 = 0 0 1 (all 0 when no model was found) */
} slideo_candidate;

int32_t     slideo_last_frame_candidates(const slideo_matcher* m, int32_t frame_in_batch,
                                         slideo_candidate* out, int32_t capacity, int32_t* n_out);

/* slideo_match_frames_bgr8 from the frames' features on (the frame-side counterpart of slideo_matcher_add_page_features, for the
 * tests of the verify stage): frame f's keypoints and 32-byte descriptors are rows [sum kp_counts[0..f), + kp_counts[f]) of kp /
 * desc32 and take the place of ORB's output; the search, the vote, RANSAC, the rating, the re-projection (which reads the n
 * equally sized host frames) and the verdict run as in a frame call.  Synchronous, one unit, the exact-size search; verdicts as
 * slideo_match_frames_bgr8 returns them, slideo_last_frame_candidates works after it.  ORB mode with the exact Hamming search
 * (matcher 0) only, frames as given (no working size, no frame region): otherwise SLIDEO_ERR_INVALID_ARG; SLIDEO_ERR_STATE before
 * slideo_matcher_finalize_pages or with a unit in flight.  At most 4096 frames. */
int32_t     slideo_match_frames_features_bgr8(slideo_matcher* m, int32_t n_frames, const uint8_t* frames, int32_t width,
                                              int32_t height, int32_t stride_bytes, int64_t frame_stride_bytes,
                                              const int32_t* kp_counts, const slideo_keypoint* kp, const uint8_t* desc32,
                                              slideo_verdict* verdicts_out);

/* ---- N-device group ----------------------------------------------------------------------------------------------
 * One matcher per device behind ONE handle: what the reference's fan-out over every core of the machine becomes on a node
 * with several GPUs (rayon: one task per changed frame, mo/lib.rs:174,213; pages par_iter, mo/lib.rs:45-47).  The page
 * database is replicated on every member device, a call's frames are cut into contiguous shards — member r
 * takes the r-th contiguous block, the blocks differing in size by at most one (the first n mod N take one more) — each shard runs through its device's matcher
 * on a host thread of its own, and every shard's verdicts land in the caller's array at the shard's offset: the gather of the
 * in-process form is the device-to-host copy each member makes anyway.  Page analysis is sharded the same way and every
 * member appends the whole call in page order.  Results are those of a single matcher, bit for bit, whatever N is.
 * `devices`: HIP ordinals, one member each (an ordinal may repeat: two members then share a device).  A group is not
 * re-entrant (like a matcher); progress callbacks fire from the member threads, one at a time, with a count that never
 * decreases.  (One PROCESS per GPU — where every rank needs
 * the whole timeline — is the other multi-GPU form: slideo_match_frames_collect_dev leaves a rank's records in device memory
 * for ONE RCCL all-gather, bench.py / slideo_amd/distributed.py.) */
typedef struct slideo_group slideo_group;
/* gfx950 devices visible to this process (0 when there is none: nothing here runs without one). */
int32_t     slideo_device_count(void);
/* Their HIP ordinals, ascending: fills at most `capacity` entries of ordinals_out (may be NULL) and returns how many there
 * are.  On a node whose HIP ordinals also name other architectures the ordinals are not 0 .. count-1. */
int32_t     slideo_device_list(int32_t* ordinals_out, int32_t capacity);
/* n_devices == 0 (devices may then be NULL): one member per gfx950 device of the node = slideo_device_list's ordinals. */
int32_t     slideo_group_create(const slideo_config* cfg, int32_t n_devices, const int32_t* devices, slideo_group** out);
void        slideo_group_destroy(slideo_group* g);
/* Message of the last failure on `g` (of the last failed create when g is NULL); names the member and its device. */
const char* slideo_group_last_error(const slideo_group* g);
int32_t     slideo_group_device_count(const slideo_group* g);
/* Member i's matcher (owned by the group): for the introspection calls, the taps and the measurement hooks above. */
slideo_matcher* slideo_group_member(slideo_group* g, int32_t i);
int32_t     slideo_group_set_progress(slideo_group* g, slideo_progress_fn fn, void* user);
/* slideo_matcher_use_sift on every member (before the first page). */
int32_t     slideo_group_use_sift(slideo_group* g, const slideo_sift_config* cfg, float ratio);
/* slideo_matcher_add_pages_bgr8 with the call's pages analysed across the members (mo/lib.rs:45-56). */
int32_t     slideo_group_add_pages_bgr8(slideo_group* g, int32_t n_pages, const uint8_t* const* data,
                                        const int32_t* width, const int32_t* height, const int32_t* stride_bytes);
int32_t     slideo_group_finalize_pages(slideo_group* g);
int32_t     slideo_group_page_count(const slideo_group* g);
int64_t     slideo_group_descriptor_count(const slideo_group* g);
/* slideo_match_frames_bgr8 with the frames sharded over the members (mo/lib.rs:213-214: one independent task per frame). */
int32_t     slideo_group_match_frames_bgr8(slideo_group* g, int32_t n_frames, const uint8_t* frames, int32_t width, int32_t height,
                                           int32_t stride_bytes, int64_t frame_stride_bytes, slideo_verdict* verdicts_out);
/* Trace of frame `frame_in_batch` of the LAST slideo_group_match_frames_bgr8 call (from the member that matched it). */
int32_t     slideo_group_last_frame_candidates(const slideo_group* g, int32_t frame_in_batch, slideo_candidate* out, int32_t capacity,
                                               int32_t* n_out);
/* slideo_changed_mask_bgr8 over the members: a shard reads the one frame before its block (the previous sampled frame
 * MarkSimilarIter compares with, mo/video_capture.rs:86-98) — flags equal the single matcher's.  Every member keeps its
 * block's frames for slideo_group_match_kept_frames, which matches each selected frame on the member that holds it. */
int32_t     slideo_group_changed_mask_bgr8(slideo_group* g, int32_t n_frames, const uint8_t* frames, int32_t width, int32_t height,
                                           int32_t stride_bytes, int64_t frame_stride_bytes, const uint8_t* prev_small,
                                           uint8_t* last_small_out, uint8_t* changed_out, float* similarity_out);
int32_t     slideo_group_match_kept_frames(slideo_group* g, int32_t n_sel, const int32_t* sel, slideo_verdict* verdicts_out);
/* Page sets on every member (the members hand out identical ids); results equal a single matcher's under the same set. */
int32_t     slideo_group_create_page_set(slideo_group* g, int32_t n_pages, const int32_t* pages, int32_t* set_out);
int32_t     slideo_group_use_page_set(slideo_group* g, int32_t set);
int32_t     slideo_group_release_page_set(slideo_group* g, int32_t set);

/* ---- YUV 4:2:0 frames ----------------------------------------------------------------------------------------------
 * Video decoders (VCN, FFmpeg's software H.264 / HEVC decoders, VA-API) hand out YUV 4:2:0 — NV12, or planar I420 — not BGR.
 * Every frame entry point above has a *_yuv420 twin that takes such frames: half the bytes of BGR over PCIe, converted on the
 * GPU (csrc/yuv420.hip.h yuv420_to_bgr_kernel) into the BGR image the rest of the pipeline reads, unchanged.
 *
 * Semantics: a 4:2:0 frame STANDS FOR the BGR image OpenCV 4.x cvtColor(COLOR_YUV2BGR_NV12 / _NV21 / _I420 / _YV12) makes of it
 * [OCV A.14, recalled from imgproc/src/color_yuv.simd.hpp, confidence M]: BT.601 limited range, nearest chroma (pixel (x, y) takes
 * the chroma sample (x/2, y/2)), fixed point with SHIFT 20:
 *     CY = 1220542, CUB = 2116026, CUG = -409993, CVG = -852492, CVR = 1673527, half = 1 << 19
 *     u = U - 128, v = V - 128, y = max(0, Y - 16) * CY                       (int32; >> is arithmetic)
 *     R = sat_u8((y + half + CVR*v) >> 20)
 *     G = sat_u8((y + half + CVG*v + CUG*u) >> 20)
 *     B = sat_u8((y + half + CUB*u) >> 20)
 * Contract: every *_yuv420 call returns exactly what the matching *_bgr8 call returns on that BGR image, bit for bit (verdicts,
 * candidate traces, changed flags, similarities, small images).  slideo_yuv420_to_bgr8 returns the image itself.
 * DEPARTURE: the reference's own BGR comes from swscale inside OpenCV's FFmpeg backend (mo/video_capture.rs:42-57), not from
 * cvtColor, and is not reproduced bit for bit; both read the stream as BT.601 (OpenCV 4.5.2's FFmpeg backend sets no
 * sws_setColorspaceDetails — also recalled).
 * Width and height must be even (as cvtColor requires): else SLIDEO_ERR_UNSUPPORTED.  A bad layout is SLIDEO_ERR_INVALID_ARG,
 * and the message names the rule: uv_step 1 or 2; offsets >= 0; y_stride >= width; uv_stride >= (width/2) * uv_step; with
 * uv_step 2 the V byte sits next to the U byte (|v_offset - u_offset| == 1); the Y, U and V planes do not overlap (an interleaved
 * chroma plane counts as one); frame_stride covers the furthest byte of every plane. */
typedef struct slideo_yuv420_layout {
    int32_t y_stride;     /* bytes between luma rows, >= width                                                       */
    int32_t uv_stride;    /* bytes between chroma rows                                                               */
    int64_t u_offset;     /* byte offset of the first U sample from the frame's base; the Y plane starts at the base */
    int64_t v_offset;     /* byte offset of the first V sample                                                       */
    int32_t uv_step;      /* 2 = interleaved (NV12: v_offset = u_offset + 1; NV21: the reverse); 1 = planar (I420, YV12) */
    int32_t _pad;
} slideo_yuv420_layout;   /* 32 bytes.  Decoder surfaces are pitched: the chroma plane sits at pitch * aligned_height */

#define SLIDEO_YUV420_NV12 0
#define SLIDEO_YUV420_NV21 1
#define SLIDEO_YUV420_I420 2
#define SLIDEO_YUV420_YV12 3
/* The tightly packed layout of `format` (SLIDEO_YUV420_*) at width x height: y_stride = width, chroma right after the luma rows
 * (I420: U then V, each (width/2) x (height/2); YV12: V then U).  Such a frame is width * height * 3 / 2 bytes. */
int32_t     slideo_yuv420_layout_packed(int32_t format, int32_t width, int32_t height, slideo_yuv420_layout* out);

/* The twins.  Each takes (frames, width, height, layout, frame_stride_bytes) in place of (frames, width, height, stride_bytes,
 * frame_stride_bytes); everything else is as for the BGR call.  Host calls upload the YUV bytes (the furthest byte of each frame)
 * and convert on the GPU; device calls convert from the caller's memory.  The BGR image lives in the matcher's workspace until
 * the unit is collected: slideo_match_frames_collect[_dev] collects what slideo_match_frames_submit_yuv420_dev submits, and
 * slideo_match_kept_frames / slideo_group_match_kept_frames work after the YUV mask calls unchanged. */
int32_t     slideo_match_frames_yuv420(slideo_matcher* m, int32_t n_frames, const uint8_t* frames, int32_t width, int32_t height,
                                       const slideo_yuv420_layout* layout, int64_t frame_stride_bytes, slideo_verdict* verdicts_out);
int32_t     slideo_match_frames_yuv420_dev(slideo_matcher* m, int32_t n_frames, const uint8_t* frames_dev, int32_t width, int32_t height,
                                           const slideo_yuv420_layout* layout, int64_t frame_stride_bytes, slideo_verdict* verdicts_out,
                                           void* hip_stream);
int32_t     slideo_match_frames_submit_yuv420_dev(slideo_matcher* m, int32_t n_frames, const uint8_t* frames_dev, int32_t width,
                                                  int32_t height, const slideo_yuv420_layout* layout, int64_t frame_stride_bytes,
                                                  void* hip_stream, int64_t* ticket_out);
int32_t     slideo_changed_mask_yuv420(slideo_matcher* m, int32_t n_frames, const uint8_t* frames, int32_t width, int32_t height,
                                       const slideo_yuv420_layout* layout, int64_t frame_stride_bytes, const uint8_t* prev_small,
                                       uint8_t* last_small_out, uint8_t* changed_out, float* similarity_out);
/* Tap: the BGR image (stride width * 3, out_capacity >= width * height * 3) of one host frame. */
int32_t     slideo_yuv420_to_bgr8(slideo_matcher* m, const uint8_t* frame, int32_t width, int32_t height,
                                  const slideo_yuv420_layout* layout, uint8_t* bgr_out, int64_t out_capacity);
int32_t     slideo_group_match_frames_yuv420(slideo_group* g, int32_t n_frames, const uint8_t* frames, int32_t width, int32_t height,
                                             const slideo_yuv420_layout* layout, int64_t frame_stride_bytes, slideo_verdict* verdicts_out);
int32_t     slideo_group_changed_mask_yuv420(slideo_group* g, int32_t n_frames, const uint8_t* frames, int32_t width, int32_t height,
                                             const slideo_yuv420_layout* layout, int64_t frame_stride_bytes, const uint8_t* prev_small,
                                             uint8_t* last_small_out, uint8_t* changed_out, float* similarity_out);

/* ---- YUV colour description (extension: how the *_yuv420 calls read their samples) -------------------------------------------------
 * The "YUV 4:2:0 frames" door reads 8-bit samples as BT.601 limited range: OpenCV's cvtColor constants.  HD and 4K material is
 * BT.709, screen recorders often write full range, and 10-bit streams (HEVC Main10, AV1) decode to P010 (VCN, VA-API) or
 * yuv420p10le (FFmpeg).  A matcher carries a YUV DESCRIPTION (matrix, range, depth), a frame setting like the working size; the
 * default (BT601, LIMITED, 8) is exactly "YUV 4:2:0 frames", and under it every call launches exactly what it launched before.
 * It applies to EVERY call that takes a slideo_yuv420_layout — the match, submit, changed-mask and gated calls,
 * slideo_matcher_gate_reset_from_frame_yuv420[_dev], the group's forms and the tap slideo_yuv420_to_bgr8.  BGR calls never look at it.
 * Semantics: under a description a 4:2:0 frame STANDS FOR this BGR image (int32 arithmetic, >> arithmetic, half = 1 << 19,
 * nearest chroma, as "YUV 4:2:0 frames"):
 *     s8 = sample                     (SLIDEO_YUV_DEPTH_8)
 *     s8 = sample16 >> 8              (SLIDEO_YUV_DEPTH_10_MSB: the container's high byte)
 *     s8 = min(sample16, 1023) >> 2   (SLIDEO_YUV_DEPTH_10_LSB)
 *     u = U8 - 128, v = V8 - 128, y = max(0, Y8 - y_offset) * CY
 *     R = sat_u8((y + half + CVR*v) >> 20)
 *     G = sat_u8((y + half + CVG*v + CUG*u) >> 20)
 *     B = sat_u8((y + half + CUB*u) >> 20)
 * Constants.  (BT601, LIMITED) keeps cvtColor's literals.  Every other pair by ONE rule, evaluated in float64 on the host: with
 * Kr, Kb of the matrix (601: 0.299, 0.114; 709: 0.2126, 0.0722), Kg = 1 - Kr - Kb, sy = 255/219 and sc = 255/224 (both 1 for full
 * range), y_offset = 16 (0 for full range):
 *     CY = rint(sy * 2^20)   CVR = rint(sc * 2(1-Kr) * 2^20)   CUB = rint(sc * 2(1-Kb) * 2^20)
 *     CUG = -rint(sc * 2(1-Kb) Kb/Kg * 2^20)                   CVG = -rint(sc * 2(1-Kr) Kr/Kg * 2^20)
 *                         CY       CUB      CUG      CVG      CVR   y_offset
 *     BT601 LIMITED   1220542  2116026  -409993  -852492  1673527   16
 *     BT601 FULL      1048576  1858077  -360853  -748826  1470104    0
 *     BT709 LIMITED   1220945  2215014  -223607  -558796  1879825   16
 *     BT709 FULL      1048576  1945738  -196424  -490864  1651297    0
 * Every coefficient is below 2^23 in magnitude and every other factor fits 9 signed bits (Y8 - y_offset in 0..255, u / v in
 * -128..127): every operand fits 24 signed bits; every product (at most 255 * 1220945 = 3.11e8, 128 * 2215014 = 2.84e8) and every
 * sum (at most 3.11e8 + 2^19 + 2.84e8) fits int32.  The kernel's 24-bit multiplies rely on it (csrc/yuv420.hip.h
 * yuv420_to_bgr_desc_kernel).
 * Contract: every *_yuv420 call under a description returns, bit for bit, what the matching *_bgr8 call returns on that image:
 * verdicts, candidate traces, changed flags, similarities, small images.  Working size, frame region, frame mask and scopes, the
 * direct look-up, page sets and SIFT mode see the converted BGR image.
 * 16-BIT CONTAINERS (both 10-bit depths): samples are 16-bit little-endian.  All strides and offsets REMAIN BYTES, and the layout
 * rules count two bytes per sample: y_stride >= 2 * width; uv_stride >= 2 * (width/2) * uv_step; strides, offsets and
 * frame_stride even; with uv_step 2, |v_offset - u_offset| == 2; plane overlap and frame_stride count two bytes per sample.  A
 * layout that is valid for 8-bit samples but not for the matcher's depth is SLIDEO_ERR_INVALID_ARG, the rule named.  A host
 * frame is then 3 bytes per pixel of upload and staging.
 * DEPARTURE: the reference reads every stream as BT.601 limited range; a non-default description departs from it on purpose.
 * The 10-bit narrowing is TRUNCATION (the top 8 of the 10 bits) and is the library's own definition; swscale rounds differently. */
#define SLIDEO_YUV_MATRIX_BT601   0   /* default */
#define SLIDEO_YUV_MATRIX_BT709   1
#define SLIDEO_YUV_RANGE_LIMITED  0   /* default */
#define SLIDEO_YUV_RANGE_FULL     1
#define SLIDEO_YUV_DEPTH_8        0   /* default: one byte per sample */
#define SLIDEO_YUV_DEPTH_10_MSB   1   /* 16-bit little-endian containers, value in the top 10 bits (P010, and its planar form) */
#define SLIDEO_YUV_DEPTH_10_LSB   2   /* 16-bit little-endian containers, value in the low 10 bits (yuv420p10le / I010, P010-LSB) */
/* Before or after finalize, any number of times.  SLIDEO_ERR_STATE with units in flight; a value outside the enumerations is
 * SLIDEO_ERR_INVALID_ARG and the state before stays.  Ends the kept frames of an earlier mask call and resets the gate state to
 * "none", as slideo_matcher_set_frame_region does. */
int32_t     slideo_matcher_set_yuv_description(slideo_matcher* m, int32_t matrix, int32_t range, int32_t depth);
int32_t     slideo_matcher_yuv_description(const slideo_matcher* m, int32_t* matrix, int32_t* range, int32_t* depth);
/* Validates every member before changing any; resets the group's gate state. */
int32_t     slideo_group_set_yuv_description(slideo_group* g, int32_t matrix, int32_t range, int32_t depth);
/* The seven integers of the fixed-point conversion under (matrix, range): CY, CUB, CUG, CVG, CVR, y_offset, and SHIFT (20).  A pure
 * host function (no device). */
int32_t     slideo_yuv_coefficients(int32_t matrix, int32_t range, int32_t* out7);
/* The tight layout of `format` with 16-bit containers (strides and offsets in BYTES): slideo_yuv420_layout_packed's, doubled.  Such
 * a frame is width * height * 3 bytes. */
int32_t     slideo_yuv420_layout_packed16(int32_t format, int32_t width, int32_t height, slideo_yuv420_layout* out);

/* ---- YUV sampling (extension: 4:2:2, 4:4:4 and packed 4:2:2 frames through the *_yuv420 calls) ------------------------------------
 * Screen recorders write 4:4:4 (OBS "I444", x264 High 4:4:4: 4:2:0 smears coloured text), ProRes / DNxHD and broadcast recorders
 * decode to 4:2:2 (yuv422p, NV16, yuv422p10le, P210), and HDMI capture cards and UVC devices hand out packed 4:2:2 (YUY2 / UYVY).
 * A matcher carries a YUV SAMPLING, the fourth component of its YUV description, set on its own; the default is
 * SLIDEO_YUV_SAMPLING_420, under which every call launches exactly what it launched before.  Under another sampling EVERY call
 * that takes a slideo_yuv420_layout reads its frames under that sampling — the match, submit / collect, changed-mask and gated
 * calls, slideo_matcher_observe_frames_yuv420[_dev], slideo_matcher_gate_reset_from_frame_yuv420[_dev], the group's forms and the
 * tap slideo_yuv420_to_bgr8.  THE NAMES KEEP THEIR `420`: the record, the calls and the tap are the YUV door, whatever the sampling.
 * Semantics: the per-pixel formula is "YUV colour description"'s, unchanged — s8 by the depth, u = U8 - 128, v = V8 - 128,
 * y = max(0, Y8 - y_offset) * CY, the three int32 sums with half = 1 << 19, >> 20, saturate, the seven integers of the matcher's
 * (matrix, range).  Only WHICH chroma sample a pixel takes, and where the samples lie, depend on the sampling:
 *   SLIDEO_YUV_SAMPLING_422, _444: the record's fields mean what they mean for 4:2:0.  Luma at the base with y_stride; U and V at
 *     u_offset / v_offset with uv_stride between chroma rows; uv_step 1 planar, 2 interleaved.  Chroma has `height` rows and width/2
 *     (422: pixel (x, y) takes chroma (x/2, y)) or width (444: pixel (x, y) takes chroma (x, y)) samples per row.  422 needs an
 *     even width (else SLIDEO_ERR_UNSUPPORTED, as an odd side is for 4:2:0) and takes any height; 444 takes any width and height.
 *     All three depths apply; with 16-bit containers the rules count two bytes per sample exactly as for 4:2:0.  The rules
 *     (SLIDEO_ERR_INVALID_ARG, named, the message carrying the sampling): uv_step 1 or 2; offsets >= 0; y_stride >= bps * width;
 *     uv_stride >= bps * chroma width * uv_step; 16-bit: even strides, offsets and frame_stride; with uv_step 2,
 *     |v_offset - u_offset| == bps; the planes (chroma of `height` rows) do not overlap; frame_stride covers the furthest byte.
 *   SLIDEO_YUV_SAMPLING_422_PACKED: ONE plane of 4-byte macropixels, two pixels each.  Rules, each SLIDEO_ERR_INVALID_ARG with the
 *     rule named: uv_step == 4; uv_stride == y_stride; y_stride >= 2 * width; (u_offset, v_offset) one of (1, 3) YUY2, (3, 1) YVYU,
 *     (0, 2) UYVY, (2, 0) VYUY.  The luma byte of pixel (x, y) is at y * y_stride + 2x + ((u_offset & 1) ^ 1); its U is at
 *     y * y_stride + u_offset + 4 * (x/2); V likewise.  The frame's span is (height-1) * y_stride + 2 * width.  Even width, any
 *     height.  The overlap rule does not apply: there is one plane.  The depth must be SLIDEO_YUV_DEPTH_8: whichever of
 *     slideo_matcher_set_yuv_sampling and slideo_matcher_set_yuv_description would complete 422_PACKED with a 10-bit depth is
 *     SLIDEO_ERR_UNSUPPORTED, and the values before stay.
 * Under the default (BT601, LIMITED, 8) a packed frame stands for the image of OpenCV's cvtColor(COLOR_YUV2BGR_YUY2 / _UYVY /
 * _YVYU) [OCV A.14: the same literals and the same SHIFT 20, recalled from color_yuv.simd.hpp and unpinned, confidence M].
 * DEPARTURE: planar 4:2:2 and 4:4:4 in this fixed point have no cvtColor counterpart: they are the library's own definition.  The
 * reference decodes everything to BGR through swscale and knows none of these doors.
 * Contract: a call under a sampling returns, bit for bit, what its *_bgr8 twin returns on that image.  Working size, frame region,
 * frame mask and scopes, the direct look-up, page sets and SIFT mode see the converted image.  A host frame is 2 * bps bytes per
 * pixel of upload and staging under both 4:2:2 forms, 3 * bps under 4:4:4; the upload's extent is the frame's span.
 * Out of scope: 4-byte BGRA / RGBA input; packed 10-bit (Y210, v210); 4:1:1 and 4:4:0; fusing the grey write into the
 * conversion.  (Chroma siting other than nearest: "YUV chroma filter" below.)
 * Kernel: csrc/yuv_sampling.hip.h yuv_sampled_to_bgr_kernel<SAMPLING, DEPTH>, launched iff the sampling is not 420. */
#define SLIDEO_YUV_SAMPLING_420         0   /* default */
#define SLIDEO_YUV_SAMPLING_422         1   /* planar or semi-planar: chroma (w/2) x h, pixel (x, y) takes chroma (x/2, y) */
#define SLIDEO_YUV_SAMPLING_444         2   /* planar or semi-planar: chroma w x h, pixel (x, y) takes chroma (x, y)       */
#define SLIDEO_YUV_SAMPLING_422_PACKED  3   /* one plane of 4-byte macropixels (YUY2, UYVY, YVYU, VYUY); 8-bit only        */
/* As slideo_matcher_set_yuv_description: before or after finalize; SLIDEO_ERR_STATE with units in flight; a value outside the
 * enumeration is SLIDEO_ERR_INVALID_ARG and the state before stays; ends the kept frames and resets the gate state to "none".
 * slideo_matcher_set_yuv_description leaves the sampling alone, and slideo_matcher_yuv_description keeps its three outputs. */
int32_t     slideo_matcher_set_yuv_sampling(slideo_matcher* m, int32_t sampling);
int32_t     slideo_matcher_yuv_sampling(const slideo_matcher* m, int32_t* sampling);
/* Validates every member before changing any; resets the group's gate state. */
int32_t     slideo_group_set_yuv_sampling(slideo_group* g, int32_t sampling);
#define SLIDEO_YUV422_I422 16   /* planar: Y, U, V */
#define SLIDEO_YUV422_YV16 17   /* planar: Y, V, U */
#define SLIDEO_YUV422_NV16 18   /* Y, then interleaved U V */
#define SLIDEO_YUV422_NV61 19   /* Y, then interleaved V U */
#define SLIDEO_YUV422_YUY2 20   /* packed Y0 U Y1 V */
#define SLIDEO_YUV422_UYVY 21   /* packed U Y0 V Y1 */
#define SLIDEO_YUV422_YVYU 22   /* packed Y0 V Y1 U */
#define SLIDEO_YUV422_VYUY 23   /* packed V Y0 U Y1 */
#define SLIDEO_YUV444_I444 24   /* planar: Y, U, V */
#define SLIDEO_YUV444_YV24 25   /* planar: Y, V, U */
#define SLIDEO_YUV444_NV24 26   /* Y, then interleaved U V */
#define SLIDEO_YUV444_NV42 27   /* Y, then interleaved V U */
/* The tight layout of `format` (SLIDEO_YUV422_* / SLIDEO_YUV444_*, numbered from 16 so that they cannot be taken for
 * SLIDEO_YUV420_*) at width x height with samples of bytes_per_sample (1 or 2) bytes: planes back to back, strides and offsets in
 * BYTES.  A packed format with bytes_per_sample 2, and an odd width of a 4:2:2 format, are SLIDEO_ERR_UNSUPPORTED. */
int32_t     slideo_yuv_layout_packed(int32_t format, int32_t width, int32_t height, int32_t bytes_per_sample, slideo_yuv420_layout* out);

/* ---- YUV chroma filter (extension: bilinear, sited chroma for 4:2:0 and 4:2:2 frames through the *_yuv420 calls) -------------------
 * Under the nearest rule — OpenCV's cvtColor, and the default — pixel (x, y) takes chroma (x/2, y/2) under 4:2:0 and (x/2, y) under
 * 4:2:2: every chroma sample is repeated over a block, and it is drawn half a luma pixel to the right of where an H.264 / HEVC /
 * MPEG-2 encoder put it.  A matcher carries a YUV CHROMA FILTER, the fifth component of its YUV description, set on its own as the
 * sampling is; the default is SLIDEO_YUV_CHROMA_NEAREST, under which every call launches exactly what it launched before.  Under
 * another filter EVERY call that takes a slideo_yuv420_layout reads the chroma of its 4:2:0 / 4:2:2 frames through a bilinear filter
 * whose phase is the filter's siting — the match, submit / collect, changed-mask and gated calls,
 * slideo_matcher_observe_frames_yuv420[_dev], slideo_matcher_gate_reset_from_frame_yuv420[_dev], the group's forms and the tap
 * slideo_yuv420_to_bgr8.  BGR calls never look at it.
 * Semantics (exact integers): the per-pixel formula is "YUV colour description"'s, unchanged; only U8 and V8 of a pixel change.
 * Let C be one chroma plane's s8 values (the depth's narrowing comes FIRST: the filter works on 8-bit values at every depth), cw
 * samples per row and chh rows, every index clamped to the plane (replicate).  Weights in quarters over the samples (k-1, k, k+1):
 *                 parity 0     parity 1
 *     co-sited    (0, 4, 0)    (0, 2, 2)
 *     centred     (1, 3, 0)    (0, 3, 1)
 *   4:2:0, k = x >> 1, j = y >> 1:   H(x, r) = sum_i wh[x & 1][i] * C[r][k - 1 + i]
 *                                    U8(x, y) = (sum_i wv[y & 1][i] * H(x, j - 1 + i) + 8) >> 4
 *   4:2:2 planar, semi-planar and 422_PACKED:   U8(x, y) = (H(x, y) + 2) >> 2   (no vertical step)
 *   SLIDEO_YUV_CHROMA_BILINEAR_LEFT: wh co-sited, wv centred; _CENTER: both centred; _TOPLEFT: both co-sited.  Under 4:2:2 LEFT and
 *   TOPLEFT coincide.  Under 4:4:4 the setting is accepted and changes nothing: the kernel launched is the sampling's.
 *   The weights sum to 16 (4:2:0) or 4 (4:2:2): the result lies in 0..255 without a clamp.
 * Layout and size rules are unchanged (4:2:0: even width and height; 4:2:2: even width), and so are the bytes of upload and staging.
 * Contract: a call under a filter returns, bit for bit, what its *_bgr8 twin returns on that image.
 * DEPARTURE: the filter is the library's own definition.  Neither cvtColor nor the reference's swscale fast path interpolates chroma.
 * Kernel: csrc/yuv_chroma.hip.h yuv_chroma_to_bgr_kernel<SAMPLING, DEPTH>, launched iff the filter is not NEAREST and the sampling
 * is not 444. */
#define SLIDEO_YUV_CHROMA_NEAREST          0   /* default: everything as before */
#define SLIDEO_YUV_CHROMA_BILINEAR_LEFT    1   /* horizontally co-sited, vertically centred (H.264 / HEVC / MPEG-2 default) */
#define SLIDEO_YUV_CHROMA_BILINEAR_CENTER  2   /* centred on both axes (JPEG, MPEG-1) */
#define SLIDEO_YUV_CHROMA_BILINEAR_TOPLEFT 3   /* co-sited on both axes (BT.2020 / UHD) */
/* As slideo_matcher_set_yuv_sampling: before or after finalize; SLIDEO_ERR_STATE with units in flight; a value outside the
 * enumeration is SLIDEO_ERR_INVALID_ARG and the state before stays; ends the kept frames and resets the gate state to "none".
 * slideo_matcher_set_yuv_description and slideo_matcher_set_yuv_sampling leave the filter alone, and
 * slideo_matcher_yuv_description keeps its three outputs. */
int32_t     slideo_matcher_set_yuv_chroma(slideo_matcher* m, int32_t filter);
int32_t     slideo_matcher_yuv_chroma(const slideo_matcher* m, int32_t* filter);
/* Validates every member before changing any; resets the group's gate state. */
int32_t     slideo_group_set_yuv_chroma(slideo_group* g, int32_t filter);
/* Pure: out12 = wh[2][3], wv[2][3] of (filter, sampling), [parity][sample k-1, k, k+1], in quarters.  An axis that is not
 * interpolated is (0, 4, 0) twice: both axes under NEAREST and under 444, wv under the 4:2:2 forms.  A value outside either
 * enumeration, or a null out12, is SLIDEO_ERR_INVALID_ARG. */
int32_t     slideo_yuv_chroma_weights(int32_t filter, int32_t sampling, int32_t* out12);

/* ---- YUV transfer (extension: HLG and PQ BT.2020 frames to SDR through the *_yuv420 calls) ----------------------------------------
 * The description above reads every frame as an SDR BT.601 / BT.709 picture and cuts 10-bit samples to their top 8 bits.  Phones
 * record HLG / BT.2020 10-bit 4:2:0, HDR screen recorders and HDMI capture write PQ / BT.2020; read as SDR a white page comes out
 * grey and the similarity test fails.  A matcher carries a YUV TRANSFER, set on its own as the sampling and the chroma filter are;
 * the default is SLIDEO_YUV_TRANSFER_SDR, under which every call launches exactly what it launched before.  Under another transfer
 * EVERY call that takes a slideo_yuv420_layout — the match, submit / collect, changed-mask and gated calls,
 * slideo_matcher_observe_frames_yuv420[_dev], slideo_matcher_gate_reset_from_frame_yuv420[_dev], the group's forms and the tap
 * slideo_yuv420_to_bgr8 — reads its frames as HLG (ARIB STD-B67 / BT.2100) or PQ (SMPTE ST 2084) signals with BT.2020 primaries
 * and the BT.2020 non-constant-luminance matrix.  The description's MATRIX IS NOT CONSULTED (the matrix is part of the transfer's
 * meaning); its range and depth are used.  BGR calls never look at it.
 * white_nits is the display light that becomes SDR white: 0 means 203, the BT.2408 reference white; any other value must be finite
 * and in 1 .. 10000; under SDR it must be 0.  slideo_matcher_yuv_transfer reports the value in force (203 for a 0; 0 under SDR).
 * Semantics (int32 arithmetic, arithmetic >>, nearest chroma exactly as the sampling defines it); a frame stands for this image:
 *   1. samples at 10 bits: s10 = sample16 >> 6 (10_MSB), min(sample16, 1023) (10_LSB).  Nothing is truncated to 8 bits.
 *   2. Y'CbCr -> R'G'B' codes: the description's rule at 10 bits, SHIFT = 18 (at 20 the sums leave int32), Kr = 0.2627,
 *      Kb = 0.0593, Kg = 1 - Kr - Kb; limited range sy = 1023/876, sc = 1023/896, y_offset = 64; full range 1, 1, 0.
 *      CY = rint(sy 2^18), CVR = rint(sc 2(1-Kr) 2^18), CUB = rint(sc 2(1-Kb) 2^18), CUG = -rint(sc 2(1-Kb) Kb/Kg 2^18),
 *      CVG = -rint(sc 2(1-Kr) Kr/Kg 2^18); u = U10 - 512, v = V10 - 512, y = max(0, Y10 - y_offset) CY, half = 1 << 17,
 *      R' = clamp((y + half + CVR v) >> 18, 0, 1023), G' = clamp((y + half + CVG v + CUG u) >> 18, 0, 1023),
 *      B' = clamp((y + half + CUB u) >> 18, 0, 1023).  Every operand fits 24 signed bits, every product (at most 2.94e8) and
 *      every sum (at most 5.82e8) int32.  coef7 = CY, CUB, CUG, CVG, CVR, y_offset, SHIFT:
 *      limited 306134, 563104, -49251, -171006, 441349, 64, 18; full 262144, 493198, -43137, -149777, 386558, 0, 18.
 *   3. linear light per channel: lin = LIN[c'], uint16 [1024], 16383 = SDR white:
 *      LIN[i] = rint(16383 min(1, nits(i / 1023) / white_nits)); PQ: nits(e) = 10000 (max(e^(1/m2) - c1, 0) / (c2 - c3
 *      e^(1/m2)))^(1/m1), the ST 2084 constants; HLG: nits(e) = 1000 E(e)^1.2, E the inverse OETF e^2 / 3 for e <= 1/2 and
 *      (exp((e - c) / a) + b) / 12 above, a = 0.17883277, b = 0.28466892, c = 0.55991073 (a nominal 1000-nit display, the system
 *      gamma per channel).  Everything above white_nits clips: a slide's white is meant to become 255.
 *   4. gamut: G = M709^-1 M2020 from the two sets of primaries and D65, float64; gamut9[r][c] = rint(G 2^14) off the diagonal, the
 *      diagonal such that every row sums to exactly 2^14 (grey stays grey): 27206 -9628 -1194 / -2041 18562 -137 / -297 -1648 18329.
 *      o_r = clamp((sum_c gamut9[r][c] lin_c + (1 << 13)) >> 14, 0, 16383); products at most 4.46e8.
 *   5. encode: OUT uint8 [4096], OUT[i] = rint(255 srgb_oetf(i / 4095)); the byte is OUT[min(4095, (o + 2) >> 2)], stored B, G, R.
 * THE LIBRARY'S TABLES ARE THE DEFINITION: the host computes them once per set call in float64 and slideo_yuv_transfer_tables
 * returns them; the kernel reads those integers.  Frame levels run after the conversion as before, for anything finer.
 * Rules between settings (SLIDEO_ERR_UNSUPPORTED; whichever set call would complete the pair is refused and the values before stay):
 * a transfer other than SDR together with SLIDEO_YUV_DEPTH_8 (which also excludes SLIDEO_YUV_SAMPLING_422_PACKED); a transfer other
 * than SDR together with a chroma filter other than NEAREST while the sampling is not 4:4:4 (bilinear chroma under a transfer is
 * out of scope).
 * Contract: a call under a transfer returns, bit for bit, what its *_bgr8 twin returns on that image.  Working size, frame region,
 * frame mask and scopes, the direct look-up, page sets, frame levels and SIFT mode see the converted image.
 * DEPARTURE: the reference knows no HDR.  The per-channel system gamma, the hard clip at white_nits and the sRGB encode are the
 * library's own definition; it is no broadcast-grade tone mapper.
 * Out of scope: bilinear chroma under a transfer; a luminance-based OOTF or any tone curve other than the clip; HDR10+ / Dolby
 * Vision metadata; BT.2020 constant luminance; an SDR BT.2020 matrix value in the description; 12-bit samples; an HDR BGR door.
 * Kernel: csrc/yuv_transfer.hip.h yuv_transfer_to_bgr_kernel<SAMPLING, DEPTH>, launched iff the transfer is not SDR. */
#define SLIDEO_YUV_TRANSFER_SDR 0   /* default: everything as before */
#define SLIDEO_YUV_TRANSFER_HLG 1   /* ARIB STD-B67 / BT.2100 HLG, BT.2020 primaries, BT.2020 non-constant-luminance matrix */
#define SLIDEO_YUV_TRANSFER_PQ  2   /* SMPTE ST 2084, BT.2020 primaries, BT.2020 NCL matrix */
/* As slideo_matcher_set_yuv_sampling: before or after finalize; SLIDEO_ERR_STATE with units in flight; a transfer outside the
 * enumeration or a white_nits outside its rule is SLIDEO_ERR_INVALID_ARG and the state before stays; ends the kept frames and resets
 * the gate state to "none".  The description's, the sampling's and the chroma filter's set calls leave the transfer alone. */
int32_t     slideo_matcher_set_yuv_transfer(slideo_matcher* m, int32_t transfer, float white_nits);
int32_t     slideo_matcher_yuv_transfer(const slideo_matcher* m, int32_t* transfer, float* white_nits);
/* Validates every member before changing any; resets the group's gate state. */
int32_t     slideo_group_set_yuv_transfer(slideo_group* g, int32_t transfer, float white_nits);
/* Pure host, no device: the whole definition as integers — coef7 (step 2), gamut9 (step 4, row-major), lin1024 (step 3), out4096
 * (step 5) of (transfer, range, white_nits); any output may be null.  SLIDEO_YUV_TRANSFER_SDR (it has no tables), a value outside
 * either enumeration or a white_nits outside the set call's rule is SLIDEO_ERR_INVALID_ARG. */
int32_t     slideo_yuv_transfer_tables(int32_t transfer, int32_t range, float white_nits, int32_t* coef7, int32_t* gamut9,
                                       uint16_t* lin1024, uint8_t* out4096);

/* ---- Frame pixel format (extension: RGB, BGRA / RGBA / ARGB / ABGR and planar RGB frames through the *_bgr8 frame calls) --------------
 * B, G, R in three bytes is OpenCV's order.  Screen-capture APIs hand out four-byte pixels (PipeWire, X11 and DXGI: BGRx; macOS and
 * browsers: RGBA), GPU decoders with a colour stage and PNG / JPEG decoders give RGB(A), every PyTorch pipeline gives uint8
 * [N, 3, H, W] planar RGB, and FFmpeg's lossless screen codecs decode to gbrp.  A matcher carries a PIXEL FORMAT, a frame setting
 * like the YUV sampling; the default is SLIDEO_PIXEL_BGR8, under which every call launches and copies exactly what it did before
 * the format existed, and device frames are still read in place.  Under another format EVERY call that takes BGR frames with a
 * stride_bytes and a frame_stride_bytes reads its frames under it: slideo_match_frames_bgr8[_dev], slideo_match_frames_submit_dev,
 * slideo_changed_mask_bgr8 (slideo_match_kept_frames then matches the kept, converted frames), slideo_match_changed_frames_bgr8[_dev],
 * slideo_match_changed_frames_submit_dev, slideo_matcher_observe_frames_bgr8[_dev], slideo_matcher_gate_reset_from_frame_bgr8[_dev],
 * slideo_match_frames_features_bgr8 and the group's forms.  THE NAMES KEEP THEIR `bgr8`, as the YUV calls kept their `420`: they are
 * the BGR door, whatever the format.  Pages (slideo_matcher_add_pages_bgr8, slideo_group_add_pages_bgr8) and the single-image taps
 * (slideo_orb_bgr8, slideo_small_image_bgr8, slideo_reduce_bgr8, slideo_rectify_bgr8, ...) stay BGR: the format is a FRAME setting.
 * This closes the first item of "YUV sampling"'s out-of-scope list (4-byte BGRA / RGBA input).
 * Layout rules, each SLIDEO_ERR_INVALID_ARG with the rule and the format named:
 *   packed formats (bpp 3 or 4 bytes per pixel): row y starts at y * stride_bytes; stride_bytes >= bpp * width; a frame spans
 *     height * stride_bytes; frame_stride_bytes >= height * stride_bytes, the rule as it stood.
 *   planar formats: stride_bytes is the row stride of EVERY plane; stride_bytes >= width; plane p starts at
 *     p * height * stride_bytes; a frame spans 3 * height * stride_bytes, which frame_stride_bytes must cover.
 *   A single frame (the gate-reset calls, the tap) has no frame stride to check.  Under the default format the rules and the
 *   message are what they were ("bad image geometry ...").
 * Semantics: a frame stands for the BGR image whose pixel (x, y) has the frame's B, G and R bytes of that pixel.  The fourth byte
 * (x below: alpha or padding) is ignored: no un-premultiplying, no blending.  Contract: a call under a format returns, bit for
 * bit, what the same call under the default returns on that image — verdicts, candidate traces, changed flags, similarities,
 * small images, gate state, gate refs, activity and content counts.  Working size, frame region, frame mask and scopes, the
 * direct look-up, page sets and SIFT mode see the converted image.  *_yuv420 calls never look at the pixel format, and *_bgr8
 * calls never look at the YUV description or sampling; the gate's "one format family" rule still tells the two doors apart only.
 * A host frame is uploaded at its span (4 bytes per pixel for the four-byte formats) and converted on the device; a device frame
 * is read from the caller's memory by the conversion, which costs the in-place read the default keeps.
 * DEPARTURE: the reference only ever sees OpenCV's BGR.
 * Out of scope: 16-bit forms (BGR48, BGRA64, gbrp10le); GRAY8; premultiplied alpha; pages in other formats; a channel order baked
 * into the ORB or re-projection kernels; fusing the grey write into the conversion.
 * Kernel: csrc/pixel_format.hip.h pixels_to_bgr_kernel<FORM>, launched iff the format is not SLIDEO_PIXEL_BGR8. */
#define SLIDEO_PIXEL_BGR8         0   /* default: B G R, 3 bytes per pixel             */
#define SLIDEO_PIXEL_RGB8         1   /* R G B, 3 bytes per pixel                      */
#define SLIDEO_PIXEL_BGRA8        2   /* B G R x  (x: alpha or padding, ignored)       */
#define SLIDEO_PIXEL_RGBA8        3   /* R G B x                                       */
#define SLIDEO_PIXEL_ARGB8        4   /* x R G B                                       */
#define SLIDEO_PIXEL_ABGR8        5   /* x B G R                                       */
#define SLIDEO_PIXEL_PLANAR_RGB8  6   /* three planes R, G, B  (torch [3, H, W])       */
#define SLIDEO_PIXEL_PLANAR_BGR8  7   /* three planes B, G, R                          */
#define SLIDEO_PIXEL_PLANAR_GBR8  8   /* three planes G, B, R  (FFmpeg gbrp)           */
/* As slideo_matcher_set_yuv_sampling: before or after finalize; SLIDEO_ERR_STATE with units in flight; a value outside the
 * enumeration is SLIDEO_ERR_INVALID_ARG and the state before stays; ends the kept frames and resets the gate state to "none". */
int32_t     slideo_matcher_set_pixel_format(slideo_matcher* m, int32_t format);
int32_t     slideo_matcher_pixel_format(const slideo_matcher* m, int32_t* format);
/* Validates every member before changing any; resets the group's gate state. */
int32_t     slideo_group_set_pixel_format(slideo_group* g, int32_t format);
/* Pure: the bytes per pixel of a row (3, 4; 1: a plane's) and the planes (1, 3) of `format`; either output may be null.  A value
 * outside the enumeration is SLIDEO_ERR_INVALID_ARG. */
int32_t     slideo_pixel_format_info(int32_t format, int32_t* bytes_per_pixel, int32_t* planes);
/* Tap: ONE host frame under the matcher's pixel format -> the BGR image it stands for, width * height * 3 bytes at stride
 * 3 * width (SLIDEO_ERR_CAPACITY when out_capacity is smaller).  Under the default format a row-by-row copy. */
int32_t     slideo_pixels_to_bgr8(slideo_matcher* m, const uint8_t* frame, int32_t width, int32_t height, int32_t stride_bytes,
                                  uint8_t* bgr_out, int64_t out_capacity);

/* ---- Frame levels (extension: a per-channel tone table in front of the pipeline, learnt from the frames' own histogram) ---------------
 * Every door and shaping step puts the right geometry and the right bytes in front of the pipeline; none touches tone.  The verdict
 * is decided by a re-projection similarity, 1 - RMS / 255 between small images, which ranks the candidates and rejects any at or
 * below min_similarity.  ORB and RANSAC survive a dim, low-contrast or colour-cast picture (a filmed projection screen, limited
 * range written into a full-range container, a washed-out capture card); that number does not: a darker look-alike wins the
 * ranking, and below about a third of the contrast every frame is lost.  One per-channel linear stretch learnt from the frames' own
 * histogram cures it (docs/EXTENSIONS.md "Frame levels" has the figures).
 * A matcher carries FRAME LEVELS, a frame setting like the pixel format: a table uint8 [3][256] (B, G, R; 768 bytes, lut[c * 256 +
 * v]), off by default, under which every call launches, copies and budgets exactly what it did before the table existed.
 * THE TABLE
 *   Under levels a frame stands for the image out[y][x][c] = lut[c][in[y][x][c]], where `in` is the unit's BGR image as it was
 *   before: after the YUV or pixel-format conversion and after the working-size reduce or the frame region's rectify.  The levels
 *   are the LAST step in front of the unit.  Contract: every call that stages frames returns, bit for bit, what the same call under
 *   the default returns on those images — slideo_match_frames_*, submit / collect, slideo_changed_mask_* with
 *   slideo_match_kept_frames (the kept frames are unit images already and are not levelled twice), the gated calls,
 *   slideo_matcher_observe_frames_*, slideo_matcher_gate_reset_from_frame_*, slideo_match_frames_features_bgr8, SIFT mode, the group's
 *   forms, both doors: verdicts, candidate traces, changed flags, similarities, small images, gate state and refs, activity and
 *   content counts.  Pages, the single-image taps (slideo_orb_bgr8, slideo_small_image_bgr8, slideo_reduce_bgr8, slideo_rectify_bgr8,
 *   the conversion taps slideo_yuv420_to_bgr8 and slideo_pixels_to_bgr8, ...) and slideo_matcher_gate_reset(small) are untouched.
 *   A device frame is never written: plain device BGR frames, which the default reads in place, are levelled out of the caller's
 *   memory into the unit's staging, which such frames then budget in gated and observing calls.
 *   The identity table is stored as off: it reports set == 0 and nothing new launches.
 * THE STRETCH TABLE  slideo_frame_levels_lut, pure:
 *   lut[c][x] = clamp(floor((510 * (x - lo[c]) + (hi[c] - lo[c])) / (2 * (hi[c] - lo[c]))), 0, 255)
 *   the rounded 255 * (x - lo) / (hi - lo) in integers.  It requires 0 <= lo[c] < hi[c] <= 255; (0, 255) gives the identity.
 * THE LEARNER  A matcher carries a LEVELS HISTOGRAM session beside the activity and the content accumulator: "none", or frames,
 *   pixels and hist[3][256] as u64 (device) — the number of samples of every value per channel of the OBSERVED IMAGES (exactly the
 *   activity map's: the BGR images the pipeline would analyse) since levels_begin, across calls.  It holds no frame size: frames of
 *   any sizes add up.  The four slideo_matcher_observe_frames_* calls feed every open session in one pass; with the levels session
 *   open alone levels_hist_kernel runs alone.  A device (HIP) error in the middle of a call ends all three.
 *   Points, per channel c with total = its samples: lo[c] is the value of the sample of ascending rank floor(total * low_ppm / 1e6),
 *   0-based; hi[c] the value of the sample of rank total - 1 - floor(total * high_ppm / 1e6) (either rank clamped into 0 .. total -
 *   1).  Computed on the host from the 768 counters, in integers, and reported as they are: slideo_frame_levels_lut is what refuses
 *   hi <= lo (a constant picture).  A table learnt on levelled frames is not the source's: levels_begin refuses while a table is
 *   set, and setting a table refuses while the session is open (SLIDEO_ERR_STATE, the rule named).  It is an estimator with an exact
 *   definition: nothing is installed and no default cut is chosen.  There is no group form of the learner: the pre-pass runs on
 *   slideo_group_member(g, 0); the table goes to slideo_group_set_frame_levels.
 * DEPARTURE: the reference analyses the frames as they are.
 * Out of scope: levels in front of the reduce or the rectify; per-call or time-varying tables; gamma estimation; levels for pages;
 * 16-bit tables; fusing the table into the converters.
 * Kernels (csrc/levels.hip.h): levels_kernel, launched iff a table is set, the last launch of the staging — in place on the staged
 * image, or out of a plain device BGR frame into the staging; levels_hist_kernel, launched iff the session is open.
 * Every call returns SLIDEO_ERR_INVALID_ARG for a null handle or a null required pointer. */
/* lut768 == NULL (or the identity table): off.  As slideo_matcher_set_pixel_format: before or after finalize; SLIDEO_ERR_STATE with
 * units in flight, and while the levels histogram is open; ends the kept frames and resets the gate state to "none". */
int32_t     slideo_matcher_set_frame_levels(slideo_matcher* m, const uint8_t* lut768);
/* *set_out = 1 with the table in lut768_out, or 0 with the identity there; lut768_out may be null. */
int32_t     slideo_matcher_frame_levels(const slideo_matcher* m, uint8_t* lut768_out, int32_t* set_out);
/* Validates every member (idle, no levels histogram open) before changing any; resets the group's gate state. */
int32_t     slideo_group_set_frame_levels(slideo_group* g, const uint8_t* lut768);
/* Pure: the stretch table of the rule above.  SLIDEO_ERR_INVALID_ARG unless 0 <= lo[c] < hi[c] <= 255 for c = 0, 1, 2 (B, G, R);
 * slideo_last_error(NULL) then names the channel. */
int32_t     slideo_frame_levels_lut(const int32_t* lo /*3*/, const int32_t* hi /*3*/, uint8_t* lut768_out);
/* Tap: ONE host BGR image (rows stride_bytes apart, height * stride_bytes readable) under the matcher's table -> width * height * 3
 * bytes at stride 3 * width (SLIDEO_ERR_CAPACITY when out_capacity is smaller), through levels_kernel as a frame's unit image goes.
 * Off: a row-by-row copy. */
int32_t     slideo_levels_bgr8(slideo_matcher* m, const uint8_t* bgr, int32_t width, int32_t height, int32_t stride_bytes, uint8_t* bgr_out,
                               int64_t out_capacity);
/* Idle matcher (SLIDEO_ERR_STATE otherwise, and while a table is set).  Afterwards the histogram is empty: frames 0, pixels 0.  May be
 * called before any page is added and before finalize. */
int32_t     slideo_matcher_levels_begin(slideo_matcher* m);
/* Idle matcher.  The state "none"; the session's device buffers are released.  Fine when the state is "none" already. */
int32_t     slideo_matcher_levels_end(slideo_matcher* m);
/* The observed frames and their pixels in all.  SLIDEO_ERR_STATE in the state "none". */
int32_t     slideo_matcher_levels_info(slideo_matcher* m, int64_t* frames, int64_t* pixels);
/* Idle matcher.  hist768[c * 256 + v] (the tap the tests hold the kernel to).  SLIDEO_ERR_STATE without an observed frame. */
int32_t     slideo_matcher_levels_histogram(slideo_matcher* m, uint64_t* hist768);
/* Idle matcher.  The points of the definition.  SLIDEO_ERR_STATE without an observed frame; SLIDEO_ERR_INVALID_ARG for low_ppm or
 * high_ppm outside 0..1000000. */
int32_t     slideo_matcher_levels_points(slideo_matcher* m, int32_t low_ppm, int32_t high_ppm, int32_t* lo /*3*/, int32_t* hi /*3*/);

/* ---- Frame shading (extension: a smooth per-cell gain field in front of the levels, for vignetting and gradients) ---------------------
 * The frame levels are ONE table per channel for the whole picture: they cannot undo a gradient across the screen.  A camera filming
 * a projection screen sees exactly that — projector hot spot, screen gain and lens falloff darken the corners of the slide by a
 * factor of two to five.  ORB and RANSAC survive it; the re-projection similarity 1 - RMS / 255 does not (docs/EXTENSIONS.md "Frame
 * shading" has the figures).
 * A matcher carries a FRAME SHADING, a frame setting like the levels: a field of Q8.8 gains on the nodes of a grid over the analysed
 * image, off by default, under which every call launches, copies and budgets exactly what it did before the field existed.
 * THE FIELD  in exact integers.  cell is 16, 32 or 64; gw = ceil(aw / cell), gh = ceil(ah / cell); node (i, j) sits at pixel (i *
 *   cell, j * cell) for 0 <= i <= gw, 0 <= j <= gh; gains is uint16 [gh + 1][gw + 1], 256 = 1.0; every gain is at least 1 (a gain of
 *   0 is refused, the node named).  For pixel (x, y):
 *     i = x / cell, j = y / cell, fx = x - i * cell, fy = y - j * cell
 *     L = g[j][i]   * (cell - fy) + g[j+1][i]   * fy
 *     R = g[j][i+1] * (cell - fy) + g[j+1][i+1] * fy
 *     G = (L * (cell - fx) + R * fx + cell * cell / 2) >> (2 * log2(cell))
 *     out[c] = min(255, (in[c] * G + 128) >> 8)          c = B, G, R: one gain for all three
 *   L * (cell - fx) + R * fx stays below 2^28 and in * G below 2^24.  An all-256 field is the identity and is stored as off: it
 *   reports set == 0 and nothing new launches.  The field is bilinear between nodes and not constant per cell: a step at a cell edge
 *   would be a FAST corner of the library's own making.  It is one gain for all channels: colour belongs to the levels table.
 * WHERE IT STANDS  after the conversion and after the reduce or the rectify, and BEFORE the levels, which stay the last step in front
 *   of the unit; everything "Frame levels" says stays true, with `in` the shaded image.  Both orders are exact for a power-law camera
 *   tone; this one is the order under which a field and then a table can be learnt from the matches ("Match tone table" sees shaded
 *   frames once a field is set, and the table it yields is applied after the field).
 *   Contract, as for the levels: every call that stages frames returns, bit for bit, what the same call under the default returns on
 *   the shaded images — verdicts, candidate traces, changed flags, similarities, small images, gate state and refs, activity,
 *   content, levels, evidence, tone and placement counts; both doors, SIFT mode, the group's forms.  The frames a mask call kept are
 *   not shaded twice.  Pages, the other single-image taps and slideo_matcher_gate_reset(small) are untouched.
 *   A device frame is never written.  A frame call whose analysed size differs from the field's fails with SLIDEO_ERR_INVALID_ARG
 *   before anything is touched, as under a frame mask.
 * Kernel (csrc/shading.hip.h): shading_kernel, launched iff a field is set, in two instances — the plain one, and with a levels table
 *   set too the fused one, which does the table look-up on the shaded bytes in the same pass: levels_kernel is then not launched.
 *   levels_kernel's thread shape, loads and stores; a thread's four pixels lie in one cell, so it reads four nodes once.
 * DEPARTURE: the reference analyses the frames as they are.
 * Limits: the field is multiplicative, so a raised black is the table's job; one gain serves all channels; a fixed camera and screen
 *   are assumed.  Out of scope: per-channel fields, a field in front of the reduce or the rectify, time-varying fields, shading pages.
 * Every call returns SLIDEO_ERR_INVALID_ARG for a null handle or a null required pointer. */
/* gains == NULL (or every node 256): off, and aw, ah, cell are not looked at.  Otherwise cell 16, 32 or 64 and 1 <= aw, ah <= 4096
 * (SLIDEO_ERR_INVALID_ARG).  As slideo_matcher_set_frame_levels: before or after finalize; SLIDEO_ERR_STATE with units in flight; ends
 * the kept frames and the evidence, tone, placement and shading sessions, and resets the gate state to "none". */
int32_t     slideo_matcher_set_frame_shading(slideo_matcher* m, int32_t aw, int32_t ah, int32_t cell, const uint16_t* gains);
/* *set_out = 1 with the field's *aw, *ah, *cell, or 0 with zeros there.  gains_out == NULL asks for those alone; otherwise the (gh +
 * 1) * (gw + 1) nodes are written, or SLIDEO_ERR_CAPACITY (with the sizes set) when capacity_elems is smaller.  Off: nothing written. */
int32_t     slideo_matcher_frame_shading(const slideo_matcher* m, uint16_t* gains_out, int64_t capacity_elems, int32_t* aw, int32_t* ah,
                                         int32_t* cell, int32_t* set_out);
/* Validates every member (idle) before changing any; resets the group's gate state. */
int32_t     slideo_group_set_frame_shading(slideo_group* g, int32_t aw, int32_t ah, int32_t cell, const uint16_t* gains);
/* Tap: ONE host BGR image of the field's size (SLIDEO_ERR_INVALID_ARG at another) -> width * height * 3 bytes at stride 3 * width
 * (SLIDEO_ERR_CAPACITY when out_capacity is smaller), through shading_kernel as a frame's unit image goes: the plain instance, or,
 * with a levels table set, the fused one (the shaded and levelled image).  No field: a row-by-row copy. */
int32_t     slideo_shading_bgr8(slideo_matcher* m, const uint8_t* bgr, int32_t width, int32_t height, int32_t stride_bytes, uint8_t* bgr_out,
                                int64_t out_capacity);
/* A pure host function in integers (no handle, no device): the field of per-cell sums cnt, sum_f, sum_p [gh][gw] — samples, the sum
 * of B + G + R over the FRAME pixels and over the PAGE-side pixels they are matched with, per cell of the analysed image.
 *   1. a cell is valid iff cnt >= min_count and sum_f >= 1; its value is r = clamp((2 * 4096 * sum_p + sum_f) / (2 * sum_f),
 *      16 * min_gain_q8, 16 * max_gain_q8) (Q12; the product in 128 bits)
 *   2. fill: in rounds, every invalid cell with at least one valid 4-neighbour gets (2 * S + n) / (2 * n) over its n valid
 *      4-neighbours' values of the previous round and becomes valid; repeated until none is invalid
 *   3. smooth: `smooth` times, every cell becomes (2 * S + 9) / 18 over its edge-clamped 3x3 neighbourhood of the previous round
 *   4. node (i, j) is the rounded mean (2 * S + n) / (2 * n) of the cells (i-1..i, j-1..j) that exist: 1, 2 or 4 cells
 *   5. gain = clamp((node + 8) >> 4, min_gain_q8, max_gain_q8)
 * gains_out: (gh + 1) * (gw + 1) nodes, what slideo_matcher_set_frame_shading takes; cells_used_out (may be null): the valid cells of
 * step 1.  SLIDEO_ERR_INVALID_ARG, and nothing written: min_count < 1; bounds outside 1 <= min_gain_q8 <= 256 <= max_gain_q8 <=
 * 65535; smooth outside 0..16; cell other than 16, 32, 64 or gw, gh outside 1..ceil(4096 / cell); a count above 2^54 or a sum above
 * 765 * cnt (no pixel sums to more); no valid cell.
 * It is an ESTIMATOR, a ratio of sums dominated by the bright background; filled cells are extrapolation; nothing is installed and no
 * parameter has a default. */
int32_t     slideo_shading_field(const uint64_t* cnt, const uint64_t* sum_f, const uint64_t* sum_p, int32_t gw, int32_t gh, int32_t cell,
                                 int64_t min_count, int32_t min_gain_q8, int32_t max_gain_q8, int32_t smooth, uint16_t* gains_out,
                                 int32_t* cells_used_out);

/* ---- Working size (extension: the reference analyses every frame at the size it arrives in) ---------------------------------
 * A matcher carries a working size (max_w, max_h); (0, 0) = none, the default.  While one is set, a frame of w x h with
 * w <= max_w and h <= max_h is untouched; any other frame STANDS FOR the image cv::resize(frame, Size(dw, dh), 0, 0, INTER_AREA)
 * [OCV A.11], reduced on the GPU in front of the pipeline (csrc/reduce.hip.h), with (dw, dh) by this rule in 64-bit integers:
 *     if (w * max_h >= h * max_w) { dw = max_w; dh = max(1, (2*h*max_w + w) / (2*w)); }      width binds
 *     else                        { dh = max_h; dw = max(1, (2*w*max_h + h) / (2*h)); }      height binds
 * (aspect kept, the free side rounded half up; dw <= max_w, dh <= max_h, dw <= w, dh <= h).  3840x2160 under 1920x1080 is
 * 1920x1080 (ResizeAreaFast's 2x2 path, (sum + 2) >> 2); 4096x2160 is 1920x1013.
 * Contract: every frame call made while a working size is set — BGR and YUV 4:2:0, host and device, sync and submit / collect,
 * the mask calls and slideo_match_kept_frames, the group's calls — returns, bit for bit, what the same call without a working
 * size returns on the reduced images: verdicts, the slideo_last_frame_candidates trace, changed flags, similarities and the last
 * small image.  COORDINATES in traces and transforms are therefore those of the REDUCED image.  The reduced image is what
 * slideo_reduce_bgr8 returns, which equals the CPU restatement (oracle/ so_resize_area_bgr8_v under the matcher's ocv.area) bit
 * for bit.  A 4:2:0 frame is converted first: the reduce reads the BGR image of "YUV 4:2:0 frames".
 * Limits apply to the reduced size (area >= small_area; sides <= 4095 in SIFT mode); the source may be up to 4096 x 4096 in
 * every mode.  Pages are never reduced.  The mask calls keep the REDUCED frames for slideo_match_kept_frames.
 * DEPARTURE: the reference never reduces a frame.  With a working size set, verdicts are those of the reduced video, as if it had
 * been encoded at that size; off by default; a front door, not another matcher. */
/* The rule as a pure host function (no device).  SLIDEO_ERR_INVALID_ARG for a non-positive argument or a null output. */
int32_t     slideo_working_size(int32_t w, int32_t h, int32_t max_w, int32_t max_h, int32_t* dw, int32_t* dh);
/* Before or after finalize, any number of times; (0, 0) clears.  SLIDEO_ERR_STATE with units in flight; SLIDEO_ERR_INVALID_ARG for
 * a negative side or exactly one zero.  Ends the kept frames of an earlier mask call. */
int32_t     slideo_matcher_set_working_size(slideo_matcher* m, int32_t max_w, int32_t max_h);
int32_t     slideo_matcher_get_working_size(const slideo_matcher* m, int32_t* max_w, int32_t* max_h);
int32_t     slideo_group_set_working_size(slideo_group* g, int32_t max_w, int32_t max_h);
/* Tap: one host image reduced to an explicit dw x dh under the matcher's ocv.area (out: stride dw * 3, out_capacity >= dw * dh * 3).
 * SLIDEO_ERR_INVALID_ARG for dw > width, dh > height or dw == width && dh == height (no upscale, no copy). */
int32_t     slideo_reduce_bgr8(slideo_matcher* m, const uint8_t* bgr, int32_t width, int32_t height, int32_t stride_bytes,
                               int32_t dw, int32_t dh, uint8_t* out, int64_t out_capacity);

/* ---- Frame region (extension: the reference analyses the whole frame) -----------------------------------------------------------
 * [OCV — recalled, unpinned, like the rest of SURVEY.md Appendix A: OpenCV 4.5.2 imgproc/imgwarp.cpp WarpPerspectiveInvoker and
 * remapBilinear, INTER_BITS 5, INTER_TAB_SIZE 32, INTER_REMAP_COEF_BITS 15.]
 * A matcher carries an optional FRAME REGION: a fixed 3x3 map M from a rectified out_w x out_h image into source frames of
 * src_w x src_h.  While one is set, a frame call whose source size is (src_w, src_h) STANDS FOR
 *     R = cv::warpPerspective(frame, M, Size(out_w, out_h), INTER_LINEAR | WARP_INVERSE_MAP, BORDER_REPLICATE)
 * made on the GPU in front of the pipeline (csrc/frame_region.hip.h).  A 4:2:0 frame is converted first ("YUV 4:2:0 frames").
 * Coordinates, for destination pixel (x, y), every product and sum rounded on its own in float64, nothing fused:
 *     bw0 = max(1, min(1024 / max(min(16, out_h), 1), out_w));  xb = (x / bw0) * bw0;  x1 = x - xb
 *     X0 = M0*xb + M1*y + M2;  Y0 = M3*xb + M4*y + M5;  W0 = M6*xb + M7*y + M8;  W = W0 + M6*x1;  W = W != 0 ? 32.0 / W : 0
 *     fX = clamp((X0 + M0*x1) * W, INT_MIN, INT_MAX);  X = (int)rint(fX);   Y likewise from Y0, M3
 * Taps: sx = X >> 5, ax = X & 31, sy = Y >> 5, ay = Y & 31; the four taps p00 p01 / p10 p11 at columns clamp(sx | sx + 1, 0, src_w - 1)
 * and rows clamp(sy | sy + 1, 0, src_h - 1); the bilinear table's weights at 1/32 steps are exact integers, so per channel
 *     R = (p00*(32-ax)*(32-ay) + p01*ax*(32-ay) + p10*(32-ax)*ay + p11*ax*ay + 512) >> 10
 * Contract: every frame call made under a region — BGR and YUV 4:2:0, host and device, sync and submit / collect, the mask calls
 * and slideo_match_kept_frames, the gated calls and slideo_matcher_gate_reset_from_frame_*, the group's calls — returns, bit for
 * bit, what the same call without a region returns on the rectified images: verdicts, the slideo_last_frame_candidates trace,
 * changed flags, similarities, the last small image and direct verdicts.  COORDINATES in traces and transforms are those of the
 * RECTIFIED image.  The rectified image is what slideo_rectify_bgr8 returns.  Pages are never rectified.
 * A frame call at another source size than (src_w, src_h) is SLIDEO_ERR_INVALID_ARG (both sizes in the message): it is not
 * silently left unrectified.  The small_area limit and SIFT's side limit apply to (out_w, out_h); a frame mask's size is
 * (out_w, out_h).  WORKING SIZE: the source frame of a rectifying call is exempt from it, and the output must fit it: a region
 * whose output exceeds a set working size, or a working size smaller than a set region's output, is SLIDEO_ERR_UNSUPPORTED at
 * whichever set call comes second (the caller chooses the output size, so nothing is lost).
 * Out of scope: uploading only the region's bounding rows of host frames; a per-call or moving region; finding a quad other than the axis-aligned content box here ("Match placement map" below learns a keystoned one from the matches); a region
 * together with a larger working size.
 * DEPARTURE: the reference never rectifies a frame.  With a region set, verdicts are those of the rectified video; off by default. */
/* M: 9 doubles, row-major, copied; NULL clears the region (the other arguments are then ignored).  Before or after finalize, any
 * number of times.  SLIDEO_ERR_STATE with units in flight.  SLIDEO_ERR_INVALID_ARG, the rule named: a non-finite M; W = M6 x + M7 y
 * + M8 zero or of two signs over the four corners of the destination rectangle; out_w or out_h outside 1..4096; a source size
 * outside 1..4096.  Ends the kept frames of an earlier mask call and resets the gate state to "none". */
int32_t     slideo_matcher_set_frame_region(slideo_matcher* m, int32_t src_w, int32_t src_h, const double* M, int32_t out_w, int32_t out_h);
/* The region as set (is_set 0: none; the sizes are then 0 and M_out the identity). */
int32_t     slideo_matcher_frame_region(const slideo_matcher* m, int32_t* src_w, int32_t* src_h, double* M_out, int32_t* out_w,
                                        int32_t* out_h, int32_t* is_set);
/* Forwards to every member and resets the group's gate state. */
int32_t     slideo_group_set_frame_region(slideo_group* g, int32_t src_w, int32_t src_h, const double* M, int32_t out_w, int32_t out_h);
/* The map of a quad, a pure host function (no device).  quad: the source coordinates (pixel centres) x, y of the slide's top-left,
 * top-right, bottom-right and bottom-left corner; M_out maps (0, 0), (out_w-1, 0), (out_w-1, out_h-1), (0, out_h-1) onto them.
 * The library's own definition (not getPerspectiveTransform's bits): an axis-aligned rectangle in closed form, M = [(x1-x0)/(out_w-1)
 * 0 x0; 0 (y1-y0)/(out_h-1) y0; 0 0 1] — an integer rectangle with out equal to its size is the crop, every ax = ay = 0 and R the
 * source sub-image byte for byte — and any other quad by Gaussian elimination with partial pivoting on the 8x8 system with M8 = 1,
 * in float64.  SLIDEO_ERR_INVALID_ARG: a null argument, out_w or out_h outside 2..4096, a degenerate (collinear) or non-convex quad. */
int32_t     slideo_frame_region_from_quad(const double* quad, int32_t out_w, int32_t out_h, double* M_out);
/* Tap: R of one host image under the matcher's region (out: stride out_w * 3, out_capacity >= out_w * out_h * 3).  No small_area
 * limit.  SLIDEO_ERR_STATE without a region; SLIDEO_ERR_INVALID_ARG at another size than the region's source. */
int32_t     slideo_rectify_bgr8(slideo_matcher* m, const uint8_t* bgr, int32_t width, int32_t height, int32_t stride_bytes, uint8_t* out,
                                int64_t out_capacity);

/* ---- Frame lens (extension: radial undistortion fused into the rectify; the reference analyses the frame as the camera saw it) ----
 * A room camera sees the projection screen through a wide-angle lens; barrel distortion is not projective, so no region's M removes
 * it.  A matcher carries an optional FRAME LENS: Brown's radial terms, in the direction initUndistortRectifyMap uses (no inversion,
 * no iteration).  A point p of the ideal, distortion-free source plane is seen by the camera at
 *     c + (p - c) * g(r2),   r2 = |p - c|^2 / f^2,   g = 1 + k1 r2 + k2 r2^2
 * c = (cx, cy) in source pixel-centre coordinates; f the normaliser in pixels (a focal length, or — the mirrors' default — half the
 * source diagonal, so that k1 is the relative displacement at the corner).  While a lens is set, a frame call whose source size is
 * (src_w, src_h) STANDS FOR its analysed image U, made on the GPU in the SAME single launch that rectifies
 * (csrc/frame_lens.hip.h); shading and levels follow it, as they follow the rectify.  Without a region U is src_w x src_h; with one
 * (of the same source size) it is out_w x out_h, and the region's quad is given in IDEAL coordinates.
 * Definition, the library's own, for destination pixel (x, y) of U; float64, every operation rounded once, nothing fused:
 *   1  the ideal point.  Without a region u = x, v = y exactly.  With a region M:
 *          N0 = (M0*x + M1*y) + M2;  N1 = (M3*x + M4*y) + M5;  W = (M6*x + M7*y) + M8;  Wi = 1.0 / W;  u = N0 * Wi;  v = N1 * Wi
 *      (no column-block term: under a lens the region's own three instances are not used; an affine or translating M takes this
 *      path too)
 *   2  the lens.  dx = u - cx;  dy = v - cy;  r2 = (dx*dx + dy*dy) * q, with q = 1.0 / (f*f) computed once on the host;
 *          t = r2 * k2;  t = k1 + t;  t = r2 * t;  g = 1.0 + t;  xd = cx + dx*g;  yd = cy + dy*g
 *   3  X = (int)rint(clamp(32.0 * xd, INT_MIN, INT_MAX));  Y likewise from yd
 *   4  taps and blend exactly the region's: sx = X >> 5, ax = X & 31, the replicate clamp, integer weights of sum 1024,
 *      (sum + 512) >> 10 per channel.
 * Rules.  SLIDEO_ERR_INVALID_ARG, the rule named, the values before staying in force: a source size outside 1..4096; a non-finite
 * argument; f <= 0; the radial map r g(r) not strictly increasing over the REACH — with R2 the largest r2 of the ideal images of the
 * four destination corners (the image of the rectangle is convex, so a corner is its farthest point), 1 + 3 k1 s + 5 k2 s^2 > 0
 * must hold at s = 0, at s = R2 and at the vertex -3 k1 / (10 k2) where that lies inside (0, R2).  The rule is evaluated at the
 * commit with the region in force, so setting either of the two can trip it.  SLIDEO_ERR_UNSUPPORTED at whichever set call comes
 * second: a lens and a region of different source sizes; a lens without a region whose analysed size src_w x src_h exceeds a set
 * working size (such a lens counts as a rectifying call: its output must fit the working size and the source is exempt, as for
 * the region).  A frame call at another source size than the lens's is SLIDEO_ERR_INVALID_ARG naming both sizes: never silently
 * left distorted.  The lens commits as the region does: it needs an idle matcher (SLIDEO_ERR_STATE), ends the kept frames, resets
 * the gate state to "none" and ends the match sessions.  small_area, SIFT's side limit, a frame mask's size and a shading field's
 * size refer to the analysed size.  Pages and the other single-image taps are untouched — slideo_rectify_bgr8 stays the tap of the
 * region alone.  A device frame is never written.
 * Contract: every call that stages frames — host and device, BGR and every YUV form, every pixel format, frame lists, submit /
 * collect, gated calls, kept frames, the observe calls, groups, SIFT mode, page sets — returns, bit for bit, what the same call
 * under the default returns on the images slideo_undistort_bgr8 gives.
 * Out of scope: tangential (decentering) terms; a learnt centre or f; fisheye models; a per-call or moving lens; undistorting
 * pages; a lens in slideo_match_frames_features_bgr8; uploading only the rows a lens reads.
 * DEPARTURE: the reference never undistorts a frame.  Off by default. */
/* k1 == 0 && k2 == 0 is stored as off, and the other arguments are then not looked at (the convention of the identity levels
 * table).  Before or after finalize, any number of times. */
int32_t     slideo_matcher_set_frame_lens(slideo_matcher* m, int32_t src_w, int32_t src_h, double cx, double cy, double f, double k1, double k2);
/* The lens as set (is_set 0: none; every value is then 0). */
int32_t     slideo_matcher_frame_lens(const slideo_matcher* m, int32_t* src_w, int32_t* src_h, double* cx, double* cy, double* f, double* k1,
                                      double* k2, int32_t* is_set);
/* Forwards to every member (validated on every member before one is touched) and resets the group's gate state. */
int32_t     slideo_group_set_frame_lens(slideo_group* g, int32_t src_w, int32_t src_h, double cx, double cy, double f, double k1, double k2);
/* A pure host function (no device, no matcher): step 2 of the definition for one ideal point (u, v), the kernel's own arithmetic.
 * k1 == 0 && k2 == 0 is the off value here too: the point itself, exactly (step 2's cx + (u - cx) would round).  SLIDEO_ERR_INVALID_ARG: a null output, a non-finite argument, f <= 0. */
int32_t     slideo_frame_lens_point(double cx, double cy, double f, double k1, double k2, double u, double v, double* xd, double* yd);
/* Tap: U of one host image under the matcher's lens, and its region if one is set (out: stride 3 * the analysed width; out_capacity
 * >= the analysed size * 3).  No small_area limit.  SLIDEO_ERR_STATE without a lens; SLIDEO_ERR_INVALID_ARG at another size than
 * the lens's source. */
int32_t     slideo_undistort_bgr8(slideo_matcher* m, const uint8_t* bgr, int32_t width, int32_t height, int32_t stride_bytes, uint8_t* out,
                                  int64_t out_capacity);

/* ---- Frame mask (cv::ORB::detectAndCompute's `mask` argument; the reference passes no_array(), mo/feature_extractor.rs:35) ----------
 * [OCV — recalled, unpinned, like the rest of SURVEY.md Appendix A: OpenCV 4.5.2 features2d/orb.cpp detectAndCompute /
 * computeKeyPoints and KeyPointsFilter::runByPixelsMask.]
 * A matcher carries an optional FRAME MASK: a u8 image of mw x mh, nonzero = "detect here".  While one is set, a frame call whose
 * ANALYSED size — the size after 4:2:0 conversion and the working-size reduce — equals (mw, mh) detects its ORB keypoints as
 * detectAndCompute(frame, mask, ...) does:
 *   mask pyramid   level 0 is the mask as given; level l > 0 is resize(level l - 1, size of image level l, INTER_LINEAR_EXACT)
 *                  followed by threshold(254, THRESH_TOZERO).  The resize is the image pyramid's own (resize_kernel and the size's
 *                  tap tables, csrc/orb.hip.h), bit-identical to what that kernel does to a u8 image, so a deeper-level pixel is
 *                  nonzero only where the interpolated value is exactly 255.  slideo_frame_mask_level returns a level.
 *   filter         a FAST candidate at integer level coordinates (x, y) of level l, after non-max suppression, is dropped iff mask
 *                  level l is 0 at (x, y) ((int)(pt + 0.5f) is the identity there).  This happens BEFORE retainBest: the level's
 *                  quota is filled from the unmasked candidates, ties kept as without a mask.  Orientation, blur and BRIEF read
 *                  the unmasked image, as in OpenCV.
 * DETECTION ONLY under the default scope: the small image, the changed-frame flags and similarities, the re-projection similarity
 * and the verdict rule see the whole frame.  The changed-frame gate can be told to ignore the masked regions too: "Frame mask
 * scope" below.  Masked re-projection: not built.  The re-projection samples the frame only where the page maps, what an inset
 * costs there is slide area it hides, which no mask recovers, and reproject_vt_kernel is at its register limit.
 * Pages are never masked, a page of the mask's size included.  A frame call whose analysed size differs from the mask's fails
 * with SLIDEO_ERR_INVALID_ARG, naming both sizes; it is not silently unmasked.  SIFT mode refuses a mask with SLIDEO_ERR_UNSUPPORTED,
 * at slideo_matcher_set_frame_mask and at slideo_matcher_use_sift.  Everything behind ORB is unchanged, so every option is picked
 * up as without a mask: matcher 1 (LSH), page sets, verify_model 1, ratio_test, the gate, the mask-call + slideo_match_kept_frames
 * pair, submit / collect, the group.  A mask of all 255 gives, bit for bit, the results of no mask; a mask of all 0 gives
 * n_keypoints 0 and page_idx -1 for every frame.
 * Where it runs (csrc/frame_mask.hip.h, csrc/stage_orb.hip): the pyramid is made once, at set time; per unit ONE more kernel,
 * mask_filter_kernel, between fast_kernel and threshold_kernel on the unit's stream: a block per (frame, level) compacts the level's
 * candidate list in place and rebuilds its score histogram and count from the survivors.  A unit re-run through the exact-size
 * path applies the mask again.  Without a mask no call launches anything it did not launch before.
 * Measured (one MI355X, 500 pages, ORB-1000, 256 device-resident 1080p frames per step, a hole of 20 % of the frame;
 * docs/EXTENSIONS.md, profiles/r10_frame_mask_*): mask_filter_kernel 0.13 ms per 256 frames (18 VGPRs, 1044 B LDS, no scratch); the
 * masked step 13.21 ms against 13.00 ms without a mask (spread 0.4 ms); on frames with a random-texture inset over that 20 %, 0.984
 * of the frames are assigned to the truth with the inset masked against 0.922 without. */
/* Idle matcher (SLIDEO_ERR_STATE with units in flight), before or after finalize, any number of times: a second mask replaces the
 * first.  mask: width x height bytes, rows stride_bytes apart, host memory; the bytes are copied.  mask == NULL clears it (the sizes
 * are then ignored).  SLIDEO_ERR_INVALID_ARG for width or height < 1 or stride_bytes < width; SLIDEO_ERR_UNSUPPORTED for a side
 * beyond 4096 and in SIFT mode.  Ends the kept frames of an earlier mask call; the gate state stays. */
int32_t     slideo_matcher_set_frame_mask(slideo_matcher* m, const uint8_t* mask, int32_t width, int32_t height, int32_t stride_bytes);
/* *is_set 1 and the mask's size, or 0 and 0 x 0.  SLIDEO_ERR_INVALID_ARG for a null argument. */
int32_t     slideo_matcher_frame_mask_info(const slideo_matcher* m, int32_t* width, int32_t* height, int32_t* is_set);
/* Forwards to every member (every member idle); ends the group's kept frames. */
int32_t     slideo_group_set_frame_mask(slideo_group* g, const uint8_t* mask, int32_t width, int32_t height, int32_t stride_bytes);
/* Tap: level `level` of the mask pyramid (out: stride *lw, out_capacity >= *lw * *lh).  SLIDEO_ERR_STATE without a mask,
 * SLIDEO_ERR_INVALID_ARG for a level outside 0 .. nlevels - 1 or a null argument, SLIDEO_ERR_CAPACITY (with *lw, *lh set).
 * The tap slideo_orb_bgr8 honours the mask for an image of the mask's size; the page-side calls and slideo_pyramid_level_bgr8 never do. */
int32_t     slideo_frame_mask_level(slideo_matcher* m, int32_t level, uint8_t* out, int64_t out_capacity, int32_t* lw, int32_t* lh);

/* ---- Frame mask scope (extension: which stages the frame mask applies to) -------------------------------------------------------
 * A matcher carries a SCOPE for its frame mask: SLIDEO_MASK_DETECT (the default: the section above, nothing else), SLIDEO_MASK_GATE,
 * or both.  The scope is the matcher's: it may be set before or after the mask, survives clearing or replacing the mask, and does
 * nothing while no mask is set.  Without the DETECT bit frame calls run no mask_filter_kernel (a GATE-only mask); the rule that a
 * frame call at another analysed size than the mask's is an error holds under either bit.
 * While a mask is set AND the scope has SLIDEO_MASK_GATE, every call that makes changed flags — slideo_changed_mask_bgr8 / _yuv420,
 * slideo_match_changed_frames_* in every form, their group forms, and what follows slideo_matcher_gate_reset* — compares small images
 * over the VALID small pixels only:
 *   validity map   B = the mask binarised (nonzero -> 255) and replicated to three channels; S = to_small_image(B), exactly what a
 *                  frame of the mask's size gets (the same small_area, ocv.area variant and small_image_kernel).  Small pixel (x, y)
 *                  is valid iff S[y, x, 0] == 255: every mask pixel it averages is nonzero.  n_valid = the number of valid pixels.
 *                  Built once, when the second of {mask, GATE scope} is set, on the matcher's stream.  If n_valid == 0 that set call
 *                  fails with SLIDEO_ERR_INVALID_ARG and the previous mask and scope stay.  slideo_frame_mask_small returns the map.
 *   similarity     ssd = the sum over the valid pixels' 3 channels of (a - b)^2; the similarity is the mask call's expression with
 *                  n_valid in place of sw * sh and nothing else changed; changed iff it is < cfg.changed_similarity.  The first
 *                  frame after the state "none" stays similarity 0.0 and changed.  On the device the decision stays integer:
 *                  ssd >= slideo_changed_ssd_threshold_n(cfg.changed_similarity, n_valid); the collect-time check of the device's
 *                  flag against the host expression stays, with n_valid.
 *   size rule      a call that makes flags fails with SLIDEO_ERR_INVALID_ARG, naming both sizes, if the frames' analysed size is
 *                  not the mask's — slideo_changed_mask_* included, which under the DETECT-only scope does not look at the mask.
 * Small images are never masked: the gate state, last_small_out, slideo_matcher_gate_last_small and slideo_matcher_gate_reset's
 * prev_small are the unmasked small image.  Rules 1 - 6 of "Changed-frame gate" hold unchanged, with "the mask call" read as the
 * mask call under the same scope, and so does the group's "equal to a single matcher for every member count" rule.  A mask of all
 * 255 under the GATE scope gives, bit for bit, the results of no mask.  With the default scope no call launches anything it did not
 * launch before.
 * Where it runs (csrc/gate.hip.h, csrc/stage_gate.hip): at set time mask_bgr_kernel, the small image, gate_valid_kernel (one byte
 * weight 0xFF / 0x00 per small-image byte; n_valid by wave ballots and LDS, one store); per call ssd_masked_kernel in place of
 * ssd_kernel: the same pairs, every image read as aligned dwords whatever its byte alignment (v_alignbyte_b32), weights ANDed in,
 * the squares as 4 x u8 dot products.  Registers, LDS and measurements: docs/EXTENSIONS.md "Frame mask scope". */
#define SLIDEO_MASK_DETECT 1u
#define SLIDEO_MASK_GATE   2u
/* Idle matcher (SLIDEO_ERR_STATE with units in flight).  scope: a non-empty combination of the two bits; 0 or an unknown bit is
 * SLIDEO_ERR_INVALID_ARG.  Like slideo_matcher_set_frame_mask it ends the kept frames of an earlier mask call and leaves the gate
 * state alone. */
int32_t     slideo_matcher_set_frame_mask_scope(slideo_matcher* m, uint32_t scope);
/* The matcher's scope (SLIDEO_MASK_DETECT unless set).  SLIDEO_ERR_INVALID_ARG for a null argument. */
int32_t     slideo_matcher_frame_mask_scope(const slideo_matcher* m, uint32_t* scope);
/* Forwards to every member (every member idle); ends the group's kept frames and leaves the group's gate state. */
int32_t     slideo_group_set_frame_mask_scope(slideo_group* g, uint32_t scope);
/* slideo_changed_ssd_threshold with the similarity normalised over n_pixels pixels: the same bisection over the same expression;
 * slideo_changed_ssd_threshold(s, w, h) == slideo_changed_ssd_threshold_n(s, (int64_t)w * h).  A pure host function.  -1 for
 * n_pixels < 1 or > INT32_MAX. */
int64_t     slideo_changed_ssd_threshold_n(float changed_similarity, int64_t n_pixels);
/* Tap: the validity map, u8 0 / 255, *sw x *sh (out: stride *sw; may be NULL to ask for the sizes), and *n_valid.  Idle matcher.
 * SLIDEO_ERR_STATE without a mask or when the scope lacks SLIDEO_MASK_GATE, SLIDEO_ERR_CAPACITY (with the sizes set),
 * SLIDEO_ERR_INVALID_ARG for a null sw, sh or n_valid. */
int32_t     slideo_frame_mask_small(slideo_matcher* m, uint8_t* out, int64_t out_capacity, int32_t* sw, int32_t* sh, int64_t* n_valid);

/* ---- Changed-frame gate (MarkSimilarIter, mo/video_capture.rs:86-98, inside the unit pipeline) ---------------------------------
 * slideo_changed_mask_* + slideo_match_kept_frames are a stop-and-go pair: host frames, an idle matcher, the flags made on the host.
 * A GATED call or unit decides on the device which of its frames changed and runs ORB / search / verify on those alone; host and
 * device frames, BGR and YUV 4:2:0, synchronous and submit / collect.
 * A matcher carries a GATE STATE: "none" (the next gated frame is changed, with similarity 0.0: video_capture.rs:92) or the small
 * image of the last gated frame, kept on the device from unit to unit.  Let f_0 .. f_{N-1} be the frames of all gated calls and
 * units since the last reset, in submission order.  They must have one size and one format family (BGR or YUV 4:2:0); another size
 * or family without a reset is SLIDEO_ERR_STATE.  Then
 *   1. changed[i] and similarity[i] equal, bit for bit, what ONE slideo_changed_mask_bgr8 (_yuv420) call over the concatenation
 *      returns with the reset's prev_small, wherever unit and call boundaries fall;
 *   2. for changed[i] == 1 the slideo_verdict equals, bit for bit, what slideo_match_frames_* of the same family returns for those
 *      frames;
 *   3. slideo_last_frame_candidates(k) is the trace of the k-th CHANGED frame of the call, or of the units collected since the
 *      matcher was last idle: the indexing slideo_match_kept_frames over the flagged frames gives;
 *   4. an unchanged frame's record is {page_idx -1, similarity 0, inliers 0, keypoints 0}; the flag tells it from a "no slide"
 *      verdict;
 *   5. the small image slideo_matcher_gate_last_small returns after the last collect is the mask call's last_small_out;
 *   6. every matcher option is picked up as by the mask + match pair under the same option: the selected page set (recorded per
 *      unit at submission), the working size (the small image is the reduced image's), verify_model 1, ratio_test, SIFT mode,
 *      matcher 1.  Plain units may be in flight beside gated ones and do not touch the gate state.
 * The flag does not depend on device floating point: the mask call tests sim = 1 - (float)sqrt((double)ssd) / max_error against
 * cfg.changed_similarity, which is monotone in the integer SSD, so the device compares ssd >= T in 64-bit integers, with T from
 * slideo_changed_ssd_threshold.  The similarities returned are computed on the host, by the mask call's own expression, from the
 * SSDs read back.  Where it runs (csrc/stage_gate.hip, csrc/gate.hip.h): small images and SSDs of all n frames of a unit on the
 * unit's stream, pair 0 and the write of the new state ordered behind the previous gated unit's by an event; gate_kernel (flags,
 * kept list, count); gather_frames_kernel packs the kept frames; the kept count reaches the host in ONE short wait inside the
 * submit, and the unchanged pipeline runs for the kept frames only.  A unit without a changed frame runs no pipeline.
 * A size, format or argument error leaves the gate state untouched.  slideo_matcher_set_working_size resets it.
 *
 * The N-device group's form.  A group carries ONE gate state: "none", or a small image.  For any sequence of slideo_group_gate_reset
 * and slideo_group_match_changed_frames_* calls, changed_out, similarity_out, verdicts_out, the small image
 * slideo_group_gate_last_small returns and the trace slideo_group_last_frame_candidates(g, k, ...) returns after a gated group call
 * (k: the k-th CHANGED frame of that call, rule 3) equal, bit for bit, what a single slideo_matcher of the same config, pages and
 * options returns for the same sequence of slideo_matcher_gate_reset and slideo_match_changed_frames_* calls — for every member
 * count, more members than frames included, and wherever the shard boundaries fall.  Rules 1 - 6 hold unchanged; the call's
 * arguments are checked once, before any member is touched, so a size, format or argument error leaves the state untouched.
 * How (under the default group gate order, SLIDEO_GROUP_GATE_HALO; SLIDEO_GROUP_GATE_CHAIN hands the whole state from shard to
 * shard instead: "Group gate order"): the call is cut into the group's contiguous shards; member 0 continues the group's state, and every later non-empty shard
 * [lo, hi) first sets its member's state from frame lo - 1 (slideo_matcher_gate_reset_from_frame_*: the one-frame halo of
 * slideo_group_changed_mask_bgr8 as a gate state, one extra frame upload per member and call), then runs the gated call over its
 * block.  After the call the state is the last non-empty shard's member's; the next call moves it to member 0 through a host copy of
 * at most 3 * small_area bytes.  Page sets, the working size, verify_model 1, ratio_test and SIFT mode are the members' own, set
 * through the group's calls; slideo_group_set_working_size resets the state.  n_frames == 0 is a no-op.  Progress counts the n
 * frames of the call (a halo frame is not counted).  If a member fails in the middle of a call the group's state becomes "none", and
 * the message says so.  Calling a member's own gated entry points (through slideo_group_member) between gated group calls is
 * undefined.  Shards are contiguous: a run of changed frames loads one member (no re-deal of the kept frames). */
/* The smallest SSD of two small_w x small_h small images that counts as changed under changed_similarity: found by bisection over
 * the mask call's host expression itself.  INT64_MAX: no SSD (0 .. 255^2 * 3 * small_w * small_h) does.  A pure host function (no
 * device).  -1 for a non-positive size. */
int64_t     slideo_changed_ssd_threshold(float changed_similarity, int32_t small_w, int32_t small_h);
/* Idle matcher.  prev_small: a small_w x small_h small image (3 bytes per pixel, as last_small_out / slideo_matcher_gate_last_small
 * return it) the next gated frame compares against; NULL (the sizes are then ignored): the state "none".  A small image whose size
 * is not the next gated frames' is SLIDEO_ERR_STATE at that call. */
int32_t     slideo_matcher_gate_reset(slideo_matcher* m, const uint8_t* prev_small, int32_t small_w, int32_t small_h);
/* Idle matcher.  The gate state's small image; *sw, *sh its size (out may be NULL).  SLIDEO_ERR_STATE when the state is "none". */
int32_t     slideo_matcher_gate_last_small(slideo_matcher* m, uint8_t* out, int64_t out_capacity, int32_t* sw, int32_t* sh);
/* Idle matcher.  The gate state from a FRAME: afterwards the state is exactly what slideo_matcher_gate_reset(m, S, sw, sh) leaves,
 * S being the last_small_out of a one-frame slideo_changed_mask_* call on that frame under the matcher's working size
 * (slideo_matcher_gate_last_small returns S bit for bit; the next gated frame is compared against S).  The frame is staged as a gated
 * unit stages its frames (upload, 4:2:0 conversion, reduce; plain device BGR is read in place).  Argument, size and layout errors
 * are those of a gated call and leave the state untouched.  hip_stream: the stream the device frame was produced on (may be NULL). */
int32_t     slideo_matcher_gate_reset_from_frame_bgr8(slideo_matcher* m, const uint8_t* frame, int32_t width, int32_t height,
                                                      int32_t stride_bytes);
int32_t     slideo_matcher_gate_reset_from_frame_yuv420(slideo_matcher* m, const uint8_t* frame, int32_t width, int32_t height,
                                                        const slideo_yuv420_layout* layout);
int32_t     slideo_matcher_gate_reset_from_frame_bgr8_dev(slideo_matcher* m, const uint8_t* frame_dev, int32_t width, int32_t height,
                                                          int32_t stride_bytes, void* hip_stream);
int32_t     slideo_matcher_gate_reset_from_frame_yuv420_dev(slideo_matcher* m, const uint8_t* frame_dev, int32_t width, int32_t height,
                                                            const slideo_yuv420_layout* layout, void* hip_stream);
/* The synchronous forms (idle matcher): the call is cut into units and pipelined through the slots as slideo_match_frames_* is;
 * host frames in short units through the ordered copy stream, so that unit u + 1 uploads and gates while unit u matches.
 * changed_out [n] and verdicts_out [n] are required, similarity_out [n] may be NULL. */
int32_t     slideo_match_changed_frames_bgr8(slideo_matcher* m, int32_t n_frames, const uint8_t* frames, int32_t width, int32_t height,
                                             int32_t stride_bytes, int64_t frame_stride_bytes, uint8_t* changed_out, float* similarity_out,
                                             slideo_verdict* verdicts_out);
int32_t     slideo_match_changed_frames_yuv420(slideo_matcher* m, int32_t n_frames, const uint8_t* frames, int32_t width, int32_t height,
                                               const slideo_yuv420_layout* layout, int64_t frame_stride_bytes, uint8_t* changed_out,
                                               float* similarity_out, slideo_verdict* verdicts_out);
int32_t     slideo_match_changed_frames_bgr8_dev(slideo_matcher* m, int32_t n_frames, const uint8_t* frames_dev, int32_t width, int32_t height,
                                                 int32_t stride_bytes, int64_t frame_stride_bytes, uint8_t* changed_out, float* similarity_out,
                                                 slideo_verdict* verdicts_out, void* hip_stream);
int32_t     slideo_match_changed_frames_yuv420_dev(slideo_matcher* m, int32_t n_frames, const uint8_t* frames_dev, int32_t width, int32_t height,
                                                   const slideo_yuv420_layout* layout, int64_t frame_stride_bytes, uint8_t* changed_out,
                                                   float* similarity_out, slideo_verdict* verdicts_out, void* hip_stream);
/* The streaming forms.  Tickets share the sequence and the in-order collect rule of slideo_match_frames_submit_dev; a gated ticket
 * is collected by slideo_match_changed_frames_collect alone and a plain one by slideo_match_frames_collect[_dev] alone (the other
 * is SLIDEO_ERR_STATE, and the unit stays in flight).  The frames must stay valid until the unit is collected. */
int32_t     slideo_match_changed_frames_submit_dev(slideo_matcher* m, int32_t n_frames, const uint8_t* frames_dev, int32_t width, int32_t height,
                                                   int32_t stride_bytes, int64_t frame_stride_bytes, void* hip_stream, int64_t* ticket_out);
int32_t     slideo_match_changed_frames_submit_yuv420_dev(slideo_matcher* m, int32_t n_frames, const uint8_t* frames_dev, int32_t width,
                                                          int32_t height, const slideo_yuv420_layout* layout, int64_t frame_stride_bytes,
                                                          void* hip_stream, int64_t* ticket_out);
int32_t     slideo_match_changed_frames_collect(slideo_matcher* m, int64_t ticket, uint8_t* changed_out, float* similarity_out,
                                                slideo_verdict* verdicts_out);
/* The group's gated calls ("The N-device group's form" above): host frames, every member idle.  slideo_group_gate_reset and
 * slideo_group_gate_last_small are slideo_matcher_gate_reset / _gate_last_small on the group's one state. */
int32_t     slideo_group_gate_reset(slideo_group* g, const uint8_t* prev_small, int32_t small_w, int32_t small_h);
int32_t     slideo_group_gate_last_small(slideo_group* g, uint8_t* out, int64_t out_capacity, int32_t* sw, int32_t* sh);
int32_t     slideo_group_match_changed_frames_bgr8(slideo_group* g, int32_t n_frames, const uint8_t* frames, int32_t width, int32_t height,
                                                   int32_t stride_bytes, int64_t frame_stride_bytes, uint8_t* changed_out,
                                                   float* similarity_out, slideo_verdict* verdicts_out);
int32_t     slideo_group_match_changed_frames_yuv420(slideo_group* g, int32_t n_frames, const uint8_t* frames, int32_t width, int32_t height,
                                                     const slideo_yuv420_layout* layout, int64_t frame_stride_bytes, uint8_t* changed_out,
                                                     float* similarity_out, slideo_verdict* verdicts_out);

/* ---- Gate reference (extension: which frame a gated frame is compared with) -------------------------------------------------------
 * MarkSimilarIter compares frame i with frame i - 1.  The reference samples one frame every five seconds, where "the frame before"
 * is another picture after any slide change.  Fed every decoded frame — what the gate exists to make affordable — a change spread
 * over several frames (a cross-fade, a slide transition, an animated build, slow scrolling) never crosses the threshold in one step:
 * no frame of it is flagged, and the stream after it returns "unchanged" although it shows another slide.
 * A matcher carries a GATE REFERENCE:
 *   SLIDEO_GATE_PREVIOUS (default)  everything under "Changed-frame gate" above, as before.
 *   SLIDEO_GATE_ANCHOR              the gate state is "none" or the small image of the ANCHOR: the last frame that was flagged, and
 *                                   therefore matched.  Every unflagged frame is then within cfg.changed_similarity of a frame that
 *                                   got a verdict.
 * Under SLIDEO_GATE_ANCHOR, with f_0 .. f_{N-1} the frames of all gated calls and units since the last reset, in submission order:
 *   similarity    ssd_i is the SSD of small(f_i) against the anchor in force BEFORE f_i is decided — under SLIDEO_MASK_GATE with a mask
 *                 set over the valid small pixels, normalised over n_valid, exactly as "Frame mask scope" defines —, and
 *                 similarity[i] is the mask call's host expression of ssd_i;
 *   flag          changed[i] = similarity[i] < cfg.changed_similarity; on the device ssd_i >= slideo_changed_ssd_threshold[_n], as
 *                 under PREVIOUS;
 *   anchor        a changed frame becomes the anchor, an unchanged frame leaves it alone;
 *   state "none"  f_0 has similarity 0.0, is changed and becomes the anchor;
 *   independence  the result depends neither on where unit and call boundaries fall nor on how many units are in flight.
 * Rules 2, 3, 4 and 6 of "Changed-frame gate" hold word for word.  Rule 5 becomes: slideo_matcher_gate_last_small returns the
 * anchor's small image, unmasked; slideo_matcher_gate_reset and slideo_matcher_gate_reset_from_frame_* set the anchor.  Rule 1 is
 * replaced by the definition above (tests/gate_anchor_ref.py restates it in numpy).  The definition is exact and in integers.
 * The mask + kept pair: slideo_changed_mask_* takes prev_small explicitly and stays MarkSimilarIter, whatever the gate reference is.
 * The direct page look-up works as before on the changed frames; it never depended on the flags.
 * The reference is a frame setting: it changes on an idle matcher only (SLIDEO_ERR_STATE), an unknown value is
 * SLIDEO_ERR_INVALID_ARG and the value before stays, and a change resets the gate state (the state means another frame).
 * Group: a group of one member forwards the call and returns what the single matcher returns.  With more members SLIDEO_GATE_ANCHOR
 * is SLIDEO_ERR_UNSUPPORTED and no member is changed: a shard's anchor depends on every flag before the shard, which the one-frame
 * halo that primes a shard cannot supply.  SLIDEO_GATE_PREVIOUS is always accepted.  (That is the default group gate order,
 * SLIDEO_GROUP_GATE_HALO; under SLIDEO_GROUP_GATE_CHAIN a shard receives its predecessor's whole state and SLIDEO_GATE_ANCHOR is
 * accepted for every member count: "Group gate order".)
 * Where it runs (csrc/gate_anchor.hip.h, csrc/stage_gate_anchor.hip; gate_unit_submit's one branch): the rule is sequential — a flag
 * decides what the next frame is compared with — so a unit of n frames computes every pair it could need at once: the frames'
 * centred operand (direct_centre_kernel, its weighted instance under the gate's weights), frame_gram_kernel — <a'_i, a'_j>
 * for i < j on v_mfma_i32_32x32x32_i8, page_ssd_kernel's symmetric case, SSD = |a'_i|^2 + |a'_j|^2 - 2 <a'_i, a'_j> exact in
 * integers —, the n SSDs against the carried anchor (gate_carried_ssd_kernel, every pair cut across several blocks; the only step
 * that waits for the previous unit's state), gate_settle_kernel at a cap of 0 — the walk "Gate settle" shares: one wave walks the
 * table, one table read per step, and writes what gate_kernel writes — and gate_settle_state_kernel, which copies the last anchor's
 * small image into the state.  A unit that also looks pages up builds the operand twice.  The operand
 * takes 3 sw sh bytes (padded to 128) per frame and the table 8 n^2 bytes; a gated unit is capped at 1024 frames (a synchronous
 * call is cut accordingly, a longer submitted unit is SLIDEO_ERR_CAPACITY).  Every allocation happens before the first write of the
 * gate state, so an error leaves the state as it was. */
#define SLIDEO_GATE_PREVIOUS 0u  /* default: a gated frame is compared with the frame before it (MarkSimilarIter) */
#define SLIDEO_GATE_ANCHOR   1u  /* ... with the last frame that was flagged */
/* Idle matcher (SLIDEO_ERR_STATE otherwise).  Resets the gate state, also when the value does not change. */
int32_t     slideo_matcher_set_gate_reference(slideo_matcher* m, uint32_t ref);
/* The matcher's gate reference (SLIDEO_GATE_PREVIOUS unless set).  SLIDEO_ERR_INVALID_ARG for a null argument. */
int32_t     slideo_matcher_gate_reference(const slideo_matcher* m, uint32_t* ref);
/* Every member idle.  More than one member: SLIDEO_GATE_ANCHOR is SLIDEO_ERR_UNSUPPORTED (above) unless the group gate order is
 * SLIDEO_GROUP_GATE_CHAIN.  Resets the group's gate state. */
int32_t     slideo_group_set_gate_reference(slideo_group* g, uint32_t ref);
/* Tap: frame_gram_kernel and the operand kernels on their own.  small: n small images of sw x sh (3 bytes per pixel, back to back, host
 * memory); ssd_out [n * n]: ssd_out[i * n + j] = the SSD of images i and j over whole images (symmetric, 0 on the diagonal), or,
 * use_valid != 0, over the valid pixels of the matcher's current validity map: SLIDEO_ERR_STATE without a map in force,
 * SLIDEO_ERR_INVALID_ARG when (sw, sh) is not the map's size.  Idle matcher; needs no pages.  n <= 1024, sw * sh <= small_area. */
int32_t     slideo_small_gram_ssd(slideo_matcher* m, const uint8_t* small, int32_t n, int32_t sw, int32_t sh, int32_t use_valid,
                                  uint64_t* ssd_out);

/* ---- Gate settle (extension: match a changed frame only once the picture stands still) -----------------------------------------
 * Under SLIDEO_GATE_ANCHOR a cross-fade sends about every second frame of the fade through the pipeline, and every one of those
 * verdicts is for a blend of two slides, which is no page at all.  A settle rule matches only the frame at which the change ends.
 * A matcher carries a GATE SETTLE (settle_similarity, max_defer).  settle_similarity == 0 is off: the default, everything as
 * before.  Otherwise 0 < settle_similarity <= 1 and 0 <= max_defer <= INT32_MAX; anything else is SLIDEO_ERR_INVALID_ARG and the
 * value before stays.  Settle is meaningful under SLIDEO_GATE_ANCHOR only.  Everything is exact and in integers.
 * The gate state under settle is "none", or three things: the anchor's small image, the previous gated frame's small image, and a
 * deferral count d.  With f_0 .. f_{N-1} the frames of all gated calls and units since the last reset, in submission order, let
 * T_c = slideo_changed_ssd_threshold[_n](cfg.changed_similarity, .) and T_s the same function of settle_similarity, both over the
 * valid small pixels and n_valid under SLIDEO_MASK_GATE, exactly as ANCHOR does.
 *   state "none"  f_0 has similarity 0.0, changed = 1, and becomes anchor and previous; d = 0.
 *   otherwise     ssd_a is the SSD against the anchor in force before f_i is decided, ssd_p the SSD against the frame before it (for
 *                 the first frame after a reset: the state's previous image); away = ssd_a >= T_c, still = ssd_p < T_s.
 *                   !away:                                changed = 0, d = 0;
 *                   away && (still || d >= max_defer):    changed = 1, the frame becomes the anchor, d = 0;
 *                   away otherwise:                       changed = 0, d = min(d + 1, max_defer): the frame is DEFERRED.
 *                 The frame becomes the previous frame in every case.
 *   similarity    similarity[i] is the mask call's host expression of ssd_a, as under ANCHOR.  A deferred frame is therefore the one
 *                 with changed == 0 && similarity < cfg.changed_similarity: no new output value, no new array.  changed_out stays
 *                 0 / 1 and means "went through the pipeline and has a verdict".
 *   records       a deferred frame's record is the unchanged record {-1, 0, 0, 0}; the kept list, the traces' indexing and the
 *                 direct look-up see changed == 1 frames only.  Rules 2, 3, 4 and 6 of "Changed-frame gate" hold word for word.
 *   independence  the result depends neither on unit or call boundaries nor on the number of units in flight.
 *   state calls   slideo_matcher_gate_reset(S) and slideo_matcher_gate_reset_from_frame_* set anchor = previous = that image, d = 0;
 *                 slideo_matcher_gate_last_small returns the anchor; anything that resets the gate state resets all three.
 * Consequences.  With max_defer == 0 the rule is ANCHOR, bit for bit.  A change of any length gets a verdict at most max_defer
 * frames after it began.  A hard cut is matched on the SECOND frame of the new hold (the first frame is away but not still), or
 * on its first when max_defer == 0.  A stream sampled so sparsely that holds are one frame long never stands still: every verdict
 * then comes max_defer frames late — such a stream wants settle off.  (tests/gate_settle_ref.py restates the rule in numpy.)
 * The settle is part of the gate-reference frame setting: it changes on an idle matcher only (SLIDEO_ERR_STATE) and a change resets
 * the gate state, also when the values do not change.  settle_similarity > 0 with a gate reference other than SLIDEO_GATE_ANCHOR is
 * SLIDEO_ERR_UNSUPPORTED, whichever call would complete the combination — slideo_matcher_set_gate_settle under PREVIOUS, or
 * slideo_matcher_set_gate_reference(PREVIOUS) while a settle is on —, and the values before stay in force.
 * Group: a group of one member forwards the call.  With more members settle on is SLIDEO_ERR_UNSUPPORTED, checked before any member
 * is touched; setting it off is always accepted.
 * Where it runs (csrc/gate_anchor.hip.h, csrc/stage_gate_anchor.hip: ANCHOR's one unit and gate_unit_submit's one branch — plain
 * ANCHOR is this path with a cap of 0 and no previous-frame state): the unit's pair table, whose sub-diagonal gives ssd_p of frames
 * 1 .. n - 1 for nothing; gate_carried_ssd_kernel — ONE launch behind the wait on the previous gated unit for the n SSDs against the
 * carried anchor and frame 0's against the carried previous frame, every pair cut across several blocks that add their partial sums
 * with one 64-bit atomic each —; gate_settle_kernel — one wave, two ballots per 64 frames: away, and from it every lane's deferral
 * count, then the first matched lane; with max_defer == 0 it reads neither the carried count nor ssd_p —; gate_settle_state_kernel,
 * which copies the unit's last anchor (if any) and its last frame into the state and stores d.  Every allocation happens before the
 * first write of the gate state. */
/* Idle matcher (SLIDEO_ERR_STATE otherwise).  Resets the gate state, also when the values do not change. */
int32_t     slideo_matcher_set_gate_settle(slideo_matcher* m, float settle_similarity, int32_t max_defer);
/* The matcher's gate settle (0, 0 unless set).  SLIDEO_ERR_INVALID_ARG for a null argument. */
int32_t     slideo_matcher_gate_settle(const slideo_matcher* m, float* settle_similarity, int32_t* max_defer);
/* Every member idle.  More than one member: settle_similarity > 0 is SLIDEO_ERR_UNSUPPORTED (above) unless the group gate order is
 * SLIDEO_GROUP_GATE_CHAIN ("Group gate order").  Resets the group's gate state. */
int32_t     slideo_group_set_gate_settle(slideo_group* g, float settle_similarity, int32_t max_defer);
/* Tap: gate_carried_ssd_kernel on its own.  anchor_small, prev_small: one small image of sw x sh each; small: n of them back to back
 * (host memory; uploaded back to back behind the two, so odd sizes put the images at every byte alignment).  ssd_out [n + 1]:
 * ssd_out[i] = the SSD of anchor_small and image i, ssd_out[n] = the SSD of prev_small and image 0 — over whole images, or,
 * use_valid != 0, over the valid pixels of the matcher's current validity map (SLIDEO_ERR_STATE without one in force,
 * SLIDEO_ERR_INVALID_ARG at another size).  prev_small == NULL: the n pairs alone, as plain ANCHOR launches them; ssd_out[0 .. n)
 * alone is written.  Idle matcher; needs no pages.  1 <= n <= 1024, sw * sh <= small_area. */
int32_t     slideo_small_carried_ssd(slideo_matcher* m, const uint8_t* anchor_small, const uint8_t* prev_small, const uint8_t* small, int32_t n,
                                     int32_t sw, int32_t sh, int32_t use_valid, uint64_t* ssd_out);
/* Tap: gate_settle_kernel — the walk of ANCHOR with and without a settle — on its own inputs.  dot [n * n]: <a'_i, a'_j>, read for i < j alone; norm [n]: |a'_i|^2; carried [n + 1]: the
 * SSDs against the carried anchor, then frame 0's against the carried previous frame; thr_c, thr_s: T_c and T_s; d_in: the carried
 * deferral count (0 <= d_in <= max_defer); none != 0: the state "none" (nothing carried is read).  changed_out [n], ssd_out [n] (ssd_a
 * per frame), *anchor_out: the last matched frame or -1, *d_out: the count behind the unit.  Idle matcher.  1 <= n <= 1024. */
int32_t     slideo_gate_settle_walk(slideo_matcher* m, const uint64_t* dot, const int64_t* norm, const uint64_t* carried, int32_t n, int64_t thr_c,
                                    int64_t thr_s, int32_t max_defer, int32_t d_in, int32_t none, uint8_t* changed_out, uint64_t* ssd_out,
                                    int32_t* anchor_out, int32_t* d_out);

/* ---- Gate state record (extension: the whole gate state as bytes) ------------------------------------------------------------------
 * slideo_matcher_gate_last_small + slideo_matcher_gate_reset move the anchor alone: under a gate settle the previous frame and the
 * deferral count d are lost (the reset sets previous = anchor, d = 0).  The record moves all of it.
 * Layout, little-endian: a header of eight 32-bit words (32 bytes) —
 *     0 magic 0x54534753 ("SGST")   1 version 1   2 has (0: "none", 1)   3 gate reference (SLIDEO_GATE_*)   4 settle (0: off, 1: on)
 *     5 sw   6 sh   7 d (the deferral count; 0 without a settle)
 * — then, has == 1: the anchor's small image, 3 * sw * sh bytes (under SLIDEO_GATE_PREVIOUS: the last small image) and, settle == 1,
 * the previous frame's small image, 3 * sw * sh bytes.  has == 0: the header alone, sw = sh = d = 0.
 * Definition: after slideo_matcher_gate_state_import(B, export of A) into a matcher B with A's config, pages and settings, every
 * later gated call on B returns, bit for bit, what it would have returned on A, and so does slideo_matcher_gate_last_small.  (The
 * record does not hold the size and format family of the frames gated so far: like slideo_matcher_gate_reset the import forgets
 * them, and a small image whose size is not the next gated frames' is SLIDEO_ERR_STATE at that call.)
 * Import refuses, with SLIDEO_ERR_INVALID_ARG, the rule named and B's state as it was: a size that is not the one its header
 * describes (or shorter than a header); a bad magic or version; a record made under another gate reference, or with the settle on
 * where B's is off or the other way round; sw x sh outside what slideo_matcher_gate_reset accepts (sw, sh >= 1, sw * sh <=
 * small_area); d beyond B's max_defer.  A record of "none" imports as slideo_matcher_gate_reset(m, NULL, 0, 0).
 * All three calls need an idle matcher (SLIDEO_ERR_STATE with units in flight). */
/* The size of the record slideo_matcher_gate_state_export would write now. */
int32_t     slideo_matcher_gate_state_bytes(slideo_matcher* m, int64_t* bytes);
/* *bytes = the record's size, always; SLIDEO_ERR_CAPACITY when it exceeds `capacity` or out is NULL. */
int32_t     slideo_matcher_gate_state_export(slideo_matcher* m, uint8_t* out, int64_t capacity, int64_t* bytes);
int32_t     slideo_matcher_gate_state_import(slideo_matcher* m, const uint8_t* rec, int64_t bytes);

/* ---- Group gate order (extension: how a gated group call hands the gate state from shard to shard) -----------------------------------
 * It extends "The N-device group's form" of "Changed-frame gate".
 *   SLIDEO_GROUP_GATE_HALO   the default, and what that section describes: every later non-empty shard [lo, hi) primes its member from
 *                            frame lo - 1.  One frame carries neither an anchor nor a settle's state, so with more than one member
 *                            SLIDEO_GATE_ANCHOR and a gate settle that is on are SLIDEO_ERR_UNSUPPORTED.
 *   SLIDEO_GROUP_GATE_CHAIN  the shards of a gated group call are decided in order: each non-empty shard's member receives the complete
 *                            gate state its predecessor left after its last frame.  SLIDEO_GATE_ANCHOR and a gate settle are accepted
 *                            for every member count.
 * Definition.  Under CHAIN, for every gate reference, with or without a settle, a frame mask under SLIDEO_MASK_GATE, the direct
 * look-up or a page set, a sequence of group resets and gated group calls returns, bit for bit, what a single matcher returns for
 * the same sequence: flags, similarities and verdicts, the trace of the k-th pipelined frame, slideo_group_gate_last_small and
 * slideo_group_gate_state_export — for every member count, more members than frames included, and wherever the shard boundaries
 * fall.  Under SLIDEO_GATE_PREVIOUS that is also what HALO returns.
 * The setter needs every member idle (SLIDEO_ERR_STATE); an unknown value is SLIDEO_ERR_INVALID_ARG and the value before stays; a
 * successful set resets the group's gate state to "none".  With more than one member, HALO together with SLIDEO_GATE_ANCHOR or a
 * settle that is on is SLIDEO_ERR_UNSUPPORTED at whichever of the three set calls — slideo_group_set_gate_order,
 * slideo_group_set_gate_reference, slideo_group_set_gate_settle — would complete the combination, checked before any member is
 * touched; the values before stay.  A group of one member forwards its calls as before and never chains.
 * How (csrc/capi_group.hip, csrc/gate_baton.h): the call is validated once and cut into the same contiguous shards; every member
 * runs the single matcher's gated call over its shard on a thread of its own.  A later member knows on the host that it will hold
 * a state of the call's small size, so it submits its first unit at once: staging, small images, the operand and the pair table of
 * all members run side by side.  Where that unit would wait for the previous gated unit's write of the state it waits for its
 * predecessor instead: behind its last unit's state write the predecessor copies the three state buffers (anchor, previous image,
 * d) into a pinned record the group owns and publishes a baton; the successor's thread, released, queues the copy from that record
 * on its unit's stream.  Only the carried SSDs, the walk and the state write are chained.  No kernel reads a peer's memory, so
 * members on one device and on distinct devices take the same path.  A member that fails before it has published fails its
 * successor's baton: every thread ends, the lowest member's error is reported and the group's state becomes "none".
 * Between calls the group moves its state to member 0 as a record (slideo_matcher_gate_state_export / _import), not as a small image.
 * A limit, by construction: a member's pipeline blocks at its first unit until its predecessor has decided its last frame, so a call
 * whose shards span many units serialises the members' uploads.  One unit per shard — 64 frames per device, what the mirrors feed — is
 * what the order is made for. */
#define SLIDEO_GROUP_GATE_HALO 0u
#define SLIDEO_GROUP_GATE_CHAIN 1u
int32_t     slideo_group_set_gate_order(slideo_group* g, uint32_t order);
/* The group's gate order (SLIDEO_GROUP_GATE_HALO unless set).  SLIDEO_ERR_INVALID_ARG for a null argument. */
int32_t     slideo_group_gate_order(const slideo_group* g, uint32_t* order);
/* slideo_matcher_gate_state_export / _import on the group's one state (every member idle), under either order.  A reset's small
 * image exports as anchor = previous = that image, d = 0, as a single matcher's does. */
int32_t     slideo_group_gate_state_export(slideo_group* g, uint8_t* out, int64_t capacity, int64_t* bytes);
int32_t     slideo_group_gate_state_import(slideo_group* g, const uint8_t* rec, int64_t bytes);
/* Measurement: the seconds member `member` (1 .. members - 1) blocked on the host for its predecessor's gate state in the last
 * chained gated call (0 when it did not run).  SLIDEO_ERR_INVALID_ARG for a null argument or a member outside that range. */
int32_t     slideo_group_gate_chain_waited(const slideo_group* g, int32_t member, double* seconds);

/* ---- Direct page look-up (extension: the reference never decides without keypoints) ---------------------------------------------
 * In a screen recording the frame IS the slide, full screen, plus codec noise.  The reference's final score for a candidate is
 * compute_similarity(to_small(warp(frame)), page.small); for such a frame the warp is the identity up to scale, so
 * compute_similarity(to_small(frame), page.small) is the same quantity without keypoints, search or RANSAC.
 * A matcher carries a DIRECT SIMILARITY t.  0 means off and is the default; valid values are 0 < t <= 1.  While t > 0, in every
 * GATED frame call (slideo_match_changed_frames_* in every form: host or device frames, BGR or 4:2:0, synchronous or submit /
 * collect, and slideo_group_match_changed_frames_*), for a frame i whose flag is changed:
 *   eligible pages   the pages of the selected page set (set 0 = the deck) whose small size (sw_p, sh_p) equals the frame's (sw, sh);
 *   distance         ssd_i(p) = the sum over all 3 sw sh bytes of (small_i - page_small_p)^2, in integers;
 *   best page        best_i = the smallest ssd_i(p) over the eligible pages, page_i = the lowest deck page index that attains it;
 *   similarity       s_i = the mask call's host expression 1 - (float)sqrt((double)best_i) / max_error over sw sh pixels
 *                    (compute_similarity, image_utils.rs:22-27);
 *   direct verdict   if there is an eligible page and s_i >= t, frame i is DIRECT: its verdict is {page_i, s_i, inliers 0,
 *                    n_keypoints 0}, and it does NOT go through ORB, search or verify.  A direct verdict is recognisable as
 *                    page_idx >= 0 && inliers == 0: the normal path never produces that (a verdict needs a rating above 50).
 * Every other changed frame gets exactly what it gets today, bit for bit, verdict and trace; an unchanged frame stays {-1, 0, 0, 0}
 * and is never looked up; flags, similarities, the gate state and slideo_matcher_gate_last_small do not depend on t.
 * slideo_last_frame_candidates(k) (and the group's form) is the trace of the k-th frame THAT WENT THROUGH THE PIPELINE, i.e. changed
 * and not direct; with t = 0 that is rule 3's k-th changed frame.  Under a working size the small image is the reduced frame's.
 * SIFT mode, matcher 1, verify_model 1 and ratio_test need nothing: the look-up sits in front of the unit pipeline.  The group
 * equals a single matcher for every member count, as for the gate.
 * The device decides in integers: best_i <= slideo_direct_ssd_threshold(t, sw sh), the largest SSD whose host similarity is >= t,
 * found by bisection over that very expression.  At collect the host recomputes s_i from the SSD read back and checks the device's
 * decision against the host expression (a mismatch is an internal error, as for the gate's flag).
 * The plain calls (slideo_match_frames_*) and the mask + kept pair do NOT look up: their units have no small images, no kept list
 * and no host wait to ride on.
 * Departure from the reference: a direct verdict's similarity is the identity warp's, not a verified transform's, and no keypoint
 * was matched for it.  No default t is chosen here; tools/direct_rate.py reports what a user needs to choose one.
 * Refused: t > 0 together with a frame mask under the SLIDEO_MASK_GATE scope is SLIDEO_ERR_UNSUPPORTED at whichever of
 * slideo_matcher_set_direct_similarity, slideo_matcher_set_frame_mask and slideo_matcher_set_frame_mask_scope would complete the
 * combination; the state before stays in force.  SLIDEO_MASK_DETECT alone is fine.  That is the default DIRECT SCOPE,
 * SLIDEO_DIRECT_WHOLE; under SLIDEO_DIRECT_VALID the combination is allowed ("Direct look-up scope" below).
 * Where it runs (csrc/direct.hip.h, csrc/stage_direct.hip): the page operand is built at the first use with t > 0 after finalize
 * (a matcher that never turns the feature on allocates and launches nothing new): per small-size class of the deck the pages'
 * small images centred to i8 (x ^ 0x80) in the MFMA's tile order, zero padded to the K granule, |b'|^2 per page as i64 and the
 * class's ascending page list; a page set selects through a per-set eligible list cached with the set.  Per gated unit, on the
 * slot's stream: stage, small images, gate SSDs, direct_centre_kernel (the frames' aligned centred copy and |a'|^2),
 * page_ssd_kernel over all n frames (v_mfma_i32_32x32x32_i8, split over K, i64 partial sums by non-returning vector atomics),
 * direct_best_kernel, gate_kernel, direct_gate_kernel (the direct frames leave the kept list in place), the unit's ONE host wait
 * (it reads the reduced count), gather, the pipeline of the remaining frames.  Registers, LDS and measurements:
 * docs/EXTENSIONS.md "Direct page look-up". */
/* Idle matcher (SLIDEO_ERR_STATE with units in flight).  t < 0, t > 1 or NaN is SLIDEO_ERR_INVALID_ARG. */
int32_t     slideo_matcher_set_direct_similarity(slideo_matcher* m, float t);
/* The matcher's direct similarity (0 unless set).  SLIDEO_ERR_INVALID_ARG for a null argument. */
int32_t     slideo_matcher_direct_similarity(const slideo_matcher* m, float* t);
/* Forwards to every member; validated once (the value, every member idle, the refusal above), before any member is touched. */
int32_t     slideo_group_set_direct_similarity(slideo_group* g, float t);
/* The largest SSD of two small images of n_pixels pixels whose similarity is >= t.  A pure host function (no device).  -1 for
 * t outside (0, 1], NaN, n_pixels < 1 or > INT32_MAX, and where no SSD qualifies. */
int64_t     slideo_direct_ssd_threshold(float t, int64_t n_pixels);
/* Tap: n host small images of sw x sh (3 bytes per pixel, back to back) against the deck: ssd_out[i * page_count + p] = ssd_i(p) for
 * every deck page p, UINT64_MAX for a page of another small size.  The same kernels and the same page operand as the gated path
 * (it builds the operand if no gated call has).  Finalized, idle matcher; sw * sh at most cfg.small_area. */
int32_t     slideo_page_small_ssd(slideo_matcher* m, const uint8_t* small, int32_t n, int32_t sw, int32_t sh, uint64_t* ssd_out);
/* Direct look-up scope.  A screen share with a speaker thumbnail on top needs both the gate's mask scope and the look-up; a
 * matcher therefore carries a DIRECT SCOPE, additive at the unchanged ABI:
 *   SLIDEO_DIRECT_WHOLE (default)  everything above, the refusal included.
 *   SLIDEO_DIRECT_VALID            the refusal is lifted (no set call raises it), and WHILE A VALIDITY MAP IS IN FORCE - a frame mask
 *                    is set and the mask scope has SLIDEO_MASK_GATE: the very map slideo_frame_mask_small returns, with its n_valid -
 *                    every gated call looks up over the valid pixels: ssd_i(p) = the sum over the valid small pixels' three channels
 *                    of (small_i - page_small_p)^2, in integers; best_i and page_i as above (the smallest SSD, the lowest deck page
 *                    that attains it among the eligible pages); s_i = the host expression over n_valid pixels; the frame is direct
 *                    iff s_i >= t; the device decides best_i <= slideo_direct_ssd_threshold(t, n_valid), and the collect-time check
 *                    of that decision against the host expression stays.  A direct verdict is {page_i, s_i, 0, 0}.
 * With no map in force (no mask, or SLIDEO_MASK_DETECT alone) SLIDEO_DIRECT_VALID behaves as SLIDEO_DIRECT_WHOLE, bit for bit; under an
 * all-255 mask with DETECT | GATE every result equals the result of no mask under WHOLE, bit for bit.  Everything else of the
 * definition holds unchanged: unchanged frames are never looked up; flags, similarities, the gate state and
 * slideo_matcher_gate_last_small depend neither on t nor on the direct scope; a frame that is not direct gets what it gets with t = 0
 * under the same mask and mask scope; page sets, working size (the mask is then of the reduced size), host and device frames, BGR and
 * 4:2:0, synchronous and submit / collect calls, and the group for every member count.
 * Where it runs: the deck's page operand is NOT rebuilt and not copied.  With a'_m = a' at the valid bytes and 0 elsewhere, the sum
 * over the valid bytes of a' b' is <a'_m, b'> against the unmasked page operand, so page_ssd_kernel, direct_best_kernel and
 * direct_gate_kernel run unchanged; direct_centre_kernel's weighted instance (csrc/ssd_table.hip.h; written as
 * direct_centre_valid_kernel, since merged into the one template) writes the frames' operand as (x ^ 0x80) & w under
 * the gate's byte weights with the norm over the valid bytes, and its store-less instance makes the pages' masked norms, one i64 per
 * page of the class, built in front of any change to the gate state at the first look-up (or tap) under a map and cached with the
 * class until the map changes (slideo_matcher_set_frame_mask, _set_frame_mask_scope, _set_working_size).  docs/EXTENSIONS.md "Direct
 * look-up scope". */
#define SLIDEO_DIRECT_WHOLE 0u   /* default: the look-up compares whole small images (and is refused beside SLIDEO_MASK_GATE, as today) */
#define SLIDEO_DIRECT_VALID 1u   /* the look-up compares what the gate compares: the valid pixels of the gate's validity map */
/* Idle matcher (SLIDEO_ERR_STATE with units in flight).  A value other than the two above is SLIDEO_ERR_INVALID_ARG.  Going back to
 * SLIDEO_DIRECT_WHOLE while t > 0 and a mask is set under SLIDEO_MASK_GATE is SLIDEO_ERR_UNSUPPORTED (the fourth set call that can
 * complete the refused combination); the state before stays in force. */
int32_t     slideo_matcher_set_direct_scope(slideo_matcher* m, uint32_t scope);
/* The matcher's direct scope (SLIDEO_DIRECT_WHOLE unless set).  SLIDEO_ERR_INVALID_ARG for a null argument. */
int32_t     slideo_matcher_direct_scope(const slideo_matcher* m, uint32_t* scope);
/* Forwards to every member; validated once (the value, every member idle, the refusal), before any member is touched. */
int32_t     slideo_group_set_direct_scope(slideo_group* g, uint32_t scope);
/* Tap: slideo_page_small_ssd with the masked SSDs under the matcher's current validity map, whatever t and the direct scope are.
 * SLIDEO_ERR_STATE without a map in force; SLIDEO_ERR_INVALID_ARG for (sw, sh) other than the map's; UINT64_MAX for a page of another
 * small size.  The kernels and the masked page norms of the gated path (it builds the norms if no gated call has). */
int32_t     slideo_page_small_ssd_valid(slideo_matcher* m, const uint8_t* small, int32_t n, int32_t sw, int32_t sh, uint64_t* ssd_out);

/* ---- Frame activity map (extension: the measurement a frame mask can be made from) --------------------------------------------------
 * The frame mask, its GATE scope and the direct look-up's VALID scope need a mask, and the caller had to know it beforehand.  An
 * inset (a speaker, a clock) gives itself away: it changes on almost every sampled frame, a slide pixel only at slide transitions.
 * A matcher carries an ACTIVITY ACCUMULATOR, off by default.  Its state is "none", or: an analysed size (aw, ah), not fixed until
 * the first frame has been observed; a delta; the last observed image (device); `pairs`; count[ah][aw] as u32 (device).
 *   observed image   of a frame: the BGR image the pipeline would analyse — the frame after the 4:2:0 conversion under the matcher's
 *                    YUV description, then after the frame region's rectify or, failing that, the working-size reduce: exactly the
 *                    images slideo_yuv420_to_bgr8, slideo_rectify_bgr8 and slideo_reduce_bgr8 return.  The frame mask, its scope, the
 *                    direct settings, the page set and the deck are not looked at.
 *   moved            for consecutive observed images a, b, pixel (x, y) moved iff |a.B-b.B| + |a.G-b.G| + |a.R-b.R| > delta, in
 *                    integers; delta in 0..765.
 *   count, pairs     over all frames observed since activity_begin, in submission order across calls: count[y][x] = the number of
 *                    consecutive pairs in which (x, y) moved, pairs = the number of consecutive pairs.  The first frame after begin
 *                    forms no pair; the last frame of a call pairs with the first frame of the next call.
 *   active           count[y][x] * 1000000 > max_share_ppm * pairs, in unsigned 64-bit integers (strict: equality is not active).
 *   mask             mask[y][x] = 0 iff some active pixel (x', y') of the image has |x'-x| <= grow && |y'-y| <= grow, else 255; grow in
 *                    0..64.  n_active = the active pixels, n_masked = the zeros of the mask.
 * It is an estimator with an exact definition, not a detector with a claim: no default delta, share or grow is chosen here
 * (docs/EXTENSIONS.md "Frame activity map" says on what content it was tried).  The mask is never installed: the caller looks at
 * n_masked and hands the bytes to slideo_matcher_set_frame_mask.  There is no group form: the pre-pass runs on one member,
 * slideo_group_member(g, 0), and the result goes to slideo_group_set_frame_mask.
 * Observing touches nothing else: the frames a mask call kept stay valid, the gate state and every setting stay, and a setter called
 * between observes does not reset the accumulator (an analysed size that no longer fits is SLIDEO_ERR_STATE at the next observe).
 * Where it runs (csrc/stage_activity.hip, csrc/activity.hip.h): the frames are staged as every frame call stages them (upload,
 * 4:2:0 conversion, rectify or reduce; plain device BGR is read in the caller's memory), in blocks of at most 256 MiB of staging and 4096 frames,
 * into a buffer of the accumulator's own; activity_kernel once per block on slot 0's stream — a thread owns 4 pixels of a row, walks
 * the block's frames with the previous pixels and its counts in registers, one v_sad_u8 per pixel and frame, and ends with one
 * read-modify-write of its counts and one store into the carried image: no atomic, no LDS —; one synchronise at the end.  The mask
 * is made at read-out by activity_rows_kernel and activity_cols_kernel.
 * Every call returns SLIDEO_ERR_INVALID_ARG for a null handle or a null required pointer. */
/* Idle matcher (SLIDEO_ERR_STATE otherwise).  delta outside 0..765 is SLIDEO_ERR_INVALID_ARG and the state before stays.  Afterwards
 * the accumulator is empty: no size, pairs 0.  May be called before any page is added and before finalize. */
int32_t     slideo_matcher_activity_begin(slideo_matcher* m, int32_t delta);
/* Idle matcher.  The state "none"; the accumulator's device buffers are released.  Fine when the state is "none" already. */
int32_t     slideo_matcher_activity_end(slideo_matcher* m);
/* Synchronous; idle matcher; neither pages nor finalize are needed.  The argument rules of a frame source apply (the layout rules
 * under the YUV description, image geometry, frame stride, the frame region's source-size rule).  SLIDEO_ERR_STATE without a begin,
 * when the analysed size differs from the accumulator's (the message names both), and when pairs would pass INT32_MAX.  n_frames == 0
 * is a no-op.  Sizes are refused as a frame call refuses them (SLIDEO_ERR_UNSUPPORTED): an analysed image, or the source of a frame the
 * working size reduces, wider or higher than 4096.  An argument, size or state error leaves the counts, pairs and the last image as
 * they were.  A device (HIP) error in the middle of a call may have counted some of its blocks: it ends the accumulator (the state
 * "none", SLIDEO_ERR_STATE until the next begin).  hip_stream: the stream the device frames were produced on (may be NULL). */
int32_t     slideo_matcher_observe_frames_bgr8(slideo_matcher* m, int32_t n_frames, const uint8_t* frames, int32_t width, int32_t height,
                                               int32_t stride_bytes, int64_t frame_stride_bytes);
int32_t     slideo_matcher_observe_frames_yuv420(slideo_matcher* m, int32_t n_frames, const uint8_t* frames, int32_t width, int32_t height,
                                                 const slideo_yuv420_layout* layout, int64_t frame_stride_bytes);
int32_t     slideo_matcher_observe_frames_bgr8_dev(slideo_matcher* m, int32_t n_frames, const uint8_t* frames_dev, int32_t width, int32_t height,
                                                   int32_t stride_bytes, int64_t frame_stride_bytes, void* hip_stream);
int32_t     slideo_matcher_observe_frames_yuv420_dev(slideo_matcher* m, int32_t n_frames, const uint8_t* frames_dev, int32_t width,
                                                     int32_t height, const slideo_yuv420_layout* layout, int64_t frame_stride_bytes,
                                                     void* hip_stream);
/* The accumulator's analysed size (*aw == 0 before the first frame), pairs and delta.  SLIDEO_ERR_STATE in the state "none". */
int32_t     slideo_matcher_activity_info(slideo_matcher* m, int32_t* aw, int32_t* ah, int32_t* pairs, int32_t* delta);
/* Idle matcher.  The counts, ah rows of aw elements (the tap the tests hold the kernel to).  SLIDEO_ERR_STATE without an observed
 * frame; SLIDEO_ERR_CAPACITY (with *aw, *ah, *pairs set) when aw * ah > capacity_elems; out == NULL asks for the sizes only. */
int32_t     slideo_matcher_activity_counts(slideo_matcher* m, uint32_t* out, int64_t capacity_elems, int32_t* aw, int32_t* ah, int32_t* pairs);
/* Idle matcher.  The mask of the definition, tight (aw bytes per row), with n_active and n_masked.  SLIDEO_ERR_STATE while pairs == 0;
 * SLIDEO_ERR_INVALID_ARG for max_share_ppm outside 0..1000000 or grow outside 0..64; SLIDEO_ERR_CAPACITY (with *aw, *ah set) when
 * aw * ah > capacity. */
int32_t     slideo_matcher_activity_mask(slideo_matcher* m, int32_t max_share_ppm, int32_t grow, uint8_t* out, int64_t capacity, int32_t* aw,
                                         int32_t* ah, int64_t* n_active, int64_t* n_masked);

/* ---- Frame content box (extension: the measurement a frame region can be made from) ---------------------------------------------------
 * The frame region needs a quad, and the caller had to know it in pixels.  The most common case in which the slide does not fill the
 * frame is mechanical: 4:3 slides pillarboxed in a 16:9 recording, 16:10 letterboxed in 16:9, a windowboxed capture.  The slide's box
 * is static and its surroundings are black up to codec noise.  With the exact crop as a region the rectify is the clamped-copy
 * instance, the small sizes of frame and page agree, and the direct page look-up applies.
 * A matcher carries a CONTENT ACCUMULATOR, off by default and independent of the activity accumulator.  Its state is "none", or: a
 * level; an analysed size (aw, ah), fixed by the first observed frame; `frames`; lit[ah][aw] as u32 (device).
 *   observed image   of a frame: exactly the activity map's — the BGR image the pipeline would analyse, after the 4:2:0 conversion
 *                    under the matcher's YUV description, then the frame region's rectify or, failing that, the working-size reduce.
 *   lit              pixel (x, y) of an observed image is lit iff max(B, G, R) > level, in integers; level in 0..254.
 *   lit[y][x], frames  lit[y][x] = the number of observed frames since content_begin, across calls, in which (x, y) is lit; frames =
 *                    the number of observed frames.  frames may not pass INT32_MAX (SLIDEO_ERR_STATE).
 *   content pixel    lit[y][x] * 1000000 > min_share_ppm * frames, in unsigned 64-bit integers (strict); min_share_ppm in 0..1000000.
 *   row_fill, col_fill  row_fill[y] = the content pixels of row y, col_fill[x] = the content pixels of column x, n_content = their total.
 *   content row      row_fill[y] * 1000000 > min_fill_ppm * aw, in unsigned 64-bit integers (strict); content column: col_fill[x] *
 *                    1000000 > min_fill_ppm * ah; min_fill_ppm in 0..1000000.
 *   box              {x0, y0, x1, y1}: x0 = the first content column, x1 = the last content column + 1; y0, y1 the same from the
 *                    content rows.  Without a content row or without a content column the box is {0, 0, 0, 0}, and the call still
 *                    returns SLIDEO_OK.
 * It is an estimator with an exact definition, not a detector: no default level, share or fill is chosen here, and nothing is
 * installed.  It finds an axis-aligned box on dark surroundings only: not a keystoned screen, not a sub-window on a background that is
 * not black ("Match evidence map" below learns that one from the matches), and a dark-theme slide whose rows are mostly unlit needs a low min_fill or is not found (docs/EXTENSIONS.md "Frame
 * content box" says on what content it was tried).  There is no group form: the pre-pass runs on slideo_group_member(g, 0), as the
 * activity map's does; the box goes through slideo_frame_region_from_quad (corners at the pixel centres (x0, y0), (x1 - 1, y0),
 * (x1 - 1, y1 - 1), (x0, y1 - 1), the output x1 - x0 by y1 - y0) to slideo_matcher_set_frame_region / slideo_group_set_frame_region.
 * Observing: there is no observe call of its own.  The four slideo_matcher_observe_frames_* calls feed EVERY open accumulator.  With
 * only an activity session open they launch exactly what they launched before; with neither open they return SLIDEO_ERR_STATE;
 * with only a content session open content_kernel runs alone (no carried image, `pairs` untouched); with both open every check of
 * both (the analysed size against each accumulator's, the pairs and the frames limits) comes before the first write, the message
 * names the accumulator that refused, and an argument, size or state error leaves both as they were.  A device (HIP) error in the
 * middle of a call ends both.  The two sessions begin and end independently; the staging buffer they share is released when the
 * last of them ends.
 * Where it runs (csrc/stage_content.hip, csrc/content.hip.h): content_kernel once per staged block on slot 0's stream, directly
 * behind or in place of activity_kernel on the same staged frames — a thread owns 4 pixels of a row, walks the block's frames with
 * its four counts in registers and ends with one read-modify-write of them: no atomic, no LDS —; the read-out is
 * content_fill_kernel (a thread owns a column over a strip of rows; wave ballots, integer atomics) and a host scan of the two fill
 * arrays.
 * Every call returns SLIDEO_ERR_INVALID_ARG for a null handle or a null required pointer. */
/* Idle matcher (SLIDEO_ERR_STATE otherwise).  level outside 0..254 is SLIDEO_ERR_INVALID_ARG and the state before stays.  Afterwards
 * the accumulator is empty: no size, frames 0.  May be called before any page is added and before finalize. */
int32_t     slideo_matcher_content_begin(slideo_matcher* m, int32_t level);
/* Idle matcher.  The state "none"; the accumulator's device buffers are released.  Fine when the state is "none" already. */
int32_t     slideo_matcher_content_end(slideo_matcher* m);
/* The accumulator's analysed size (*aw == 0 before the first frame), frames and level.  SLIDEO_ERR_STATE in the state "none". */
int32_t     slideo_matcher_content_info(slideo_matcher* m, int32_t* aw, int32_t* ah, int32_t* frames, int32_t* level);
/* Idle matcher.  The lit counts, ah rows of aw elements (the tap the tests hold the kernel to).  SLIDEO_ERR_STATE without an observed
 * frame; SLIDEO_ERR_CAPACITY (with *aw, *ah, *frames set) when aw * ah > capacity_elems; out == NULL asks for the sizes only. */
int32_t     slideo_matcher_content_counts(slideo_matcher* m, uint32_t* out, int64_t capacity_elems, int32_t* aw, int32_t* ah, int32_t* frames);
/* Idle matcher.  The box of the definition (4 values) and n_content; fill_out, when not NULL, receives the ah row fills, then the aw
 * column fills.  SLIDEO_ERR_STATE while frames == 0; SLIDEO_ERR_INVALID_ARG for min_share_ppm or min_fill_ppm outside 0..1000000;
 * SLIDEO_ERR_CAPACITY when fill_out is given and ah + aw > fill_capacity_elems. */
int32_t     slideo_matcher_content_box(slideo_matcher* m, int32_t min_share_ppm, int32_t min_fill_ppm, int32_t* box /*4*/,
                                       int64_t* n_content, uint32_t* fill_out /*nullable: ah row fills, then aw column fills*/,
                                       int64_t fill_capacity_elems);

/* ---- Gate memory (extension: recall the verdict of an earlier matched frame) --------------------------------------------------------
 * Under SLIDEO_GATE_ANCHOR the gate knows ONE earlier picture, the anchor.  A lecture recording returns to pictures it has shown
 * before — a cut back from the speaker camera to the slide, a flip back two slides, a toggled build, a recurring agenda slide —, and
 * every such return is "away from the anchor": it goes through the pipeline and gets a verdict the library already computed for a
 * frame of the same picture, within the threshold the gate already trusts.  The second verdict need not even equal the first.
 * A matcher carries a GATE MEMORY capacity M.  0 is off: the default, everything as before.  1 <= M <= SLIDEO_GATE_MEMORY_MAX (64:
 * one lane per entry); anything else is SLIDEO_ERR_INVALID_ARG and the value before stays.  It is meaningful under
 * SLIDEO_GATE_ANCHOR only, with or without a gate settle.  Everything is exact and in integers.
 * The gate state is then "none", or: an ordered list E of at most M ENTRIES, oldest first — each the small image of a frame that
 * was matched, plus that frame's ORDINAL —; which entry is the ANCHOR; the previous gated frame's small image and the deferral count
 * d, as under a settle.  A frame's ordinal is its position among the frames of all gated calls and units since the last reset, from
 * 0, as int64.  Frame f with ordinal t is decided as follows; T_c, T_s, ssd_a, ssd_p, away and still are exactly as in "Gate
 * settle" (over the valid small pixels and n_valid under SLIDEO_MASK_GATE):
 *   state "none"  f is matched: changed = 1, similarity 0.0; E = [(f, t)], it is the anchor and the previous frame, d = 0, ref = t.
 *   !away         changed = 0, d = 0, ref = the anchor's ordinal.
 *   away          let ssd_e be the SSD of f against each entry e of E and r the entry with the smallest ssd_e, ties to the greatest
 *                 ordinal.  If ssd_r < T_c, f is RECALLED: changed = 0, the anchor becomes r, d = 0, ref = r's ordinal.  No test
 *                 excludes the anchor: it cannot qualify, being away.
 *                 Nothing recalled: the rule in force decides.  f is MATCHED if there is no settle, or if still, or if d >=
 *                 max_defer: changed = 1 and (f, t) is appended to E — when E already holds M entries the oldest is dropped first
 *                 (FIFO: a recall does not refresh an entry) —, f is the anchor, d = 0, ref = t.  Otherwise f is DEFERRED:
 *                 changed = 0, d = min(d + 1, max_defer), ref = SLIDEO_GATE_REF_DEFERRED.
 *   In every case f becomes the previous frame and the next ordinal is t + 1.
 *   similarity    similarity[i] is the mask call's host expression of ssd_a, against the anchor in force BEFORE the frame is
 *                 decided, as under ANCHOR.  A recalled frame, like a deferred one, has changed == 0 && similarity <
 *                 cfg.changed_similarity; ref tells them apart (slideo_matcher_last_gate_refs).
 *   records       a recalled frame's record is the unchanged record {-1, 0, 0, 0}; the kept list, the traces' indexing and the
 *                 direct look-up see changed == 1 frames only.  Rules 2, 3, 4 and 6 of "Changed-frame gate" hold word for word.
 *   independence  the result depends neither on unit and call boundaries nor on the number of units in flight.
 *   state calls   slideo_matcher_gate_reset(S) and slideo_matcher_gate_reset_from_frame_* leave E = [(S, SLIDEO_GATE_REF_RESET)],
 *                 S as anchor and previous frame, d = 0, the next ordinal 0; a reset to "none" leaves the next ordinal 0;
 *                 slideo_matcher_gate_last_small returns the anchor's small image, unmasked; everything that resets the gate state
 *                 resets the memory.
 * Consequences.  With M = 1, flags, similarities, verdicts, traces and the last small image equal those of the same stream without
 * a memory, bit for bit.  Every frame with ref >= 0 is within cfg.changed_similarity of the frame with that ordinal, which got a
 * verdict.  A recall stands behind the verdict that frame got under whatever page set was selected then.  (tests/gate_memory_ref.py
 * restates the rule in numpy.)
 * The capacity is part of the gate-reference frame setting: it changes on an idle matcher only (SLIDEO_ERR_STATE) and a set call
 * resets the gate state, also when the value does not change.  M > 0 with a gate reference other than SLIDEO_GATE_ANCHOR is
 * SLIDEO_ERR_UNSUPPORTED, whichever call would complete the combination — slideo_matcher_set_gate_memory under PREVIOUS, or
 * slideo_matcher_set_gate_reference(PREVIOUS) while a memory is on —, and the values before stay in force.
 * Refused by name, the state before kept: a group of more than one member refuses M > 0 with SLIDEO_ERR_UNSUPPORTED, checked before
 * any member is touched (the chain's baton carries three buffers, not a ring); a group of one member forwards.  While M > 0,
 * slideo_matcher_gate_state_bytes / _export / _import and the group forms return SLIDEO_ERR_UNSUPPORTED: record version 1 holds no
 * memory, and with M = 0 everything about it stays as it is.  LRU refresh, capacities above 64 and the memory in the record are
 * follow-ups.
 * Where it runs (csrc/gate_anchor.hip.h, csrc/stage_gate_anchor.hip; gate_unit_submit's one branch into gate_anchor_unit, which with
 * M == 0 launches exactly what it launched before).  With M > 0 a unit of n frames: its operand, norms and pair table as before;
 * then, behind the wait on the previous gated unit, the memory's centred operand and norms (direct_centre_kernel over the memory's
 * WHOLE small images under the gate weights in force now, rebuilt per unit: a frame-mask change keeps the gate state), the table
 * mdot[j * M + c] = <a'_j, e'_c> (page_ssd_kernel, the engine as it is) and, under a settle, frame 0's SSD against the carried
 * previous frame (gate_carried_ssd_kernel); gate_recall_kernel — one wave, no LDS: lane l < M holds slot l's occupant, a carried
 * entry or a frame of this unit; the 64 lanes test frames i .. i + 63 against the anchor, one ballot gives away, the lanes below the
 * first away frame j are unchanged; for j every lane computes its occupant's SSD, a wave reduction on (SSD, then greater ordinal)
 * finds r, and j is recalled, matched (slot head := j, head = (head + 1) % M) or deferred; the walk continues at j + 1, so a unit
 * with more than M matches evicts inside the walk —; gate_memory_state_kernel copies every slot whose occupant is a frame of this
 * unit into the memory with its ordinal, the previous frame, d, head, count and the anchor slot.  The memory takes M small images,
 * its operand 64 rows, the table 8 n M bytes and the refs 8 n; every allocation happens before the first write of the gate state. */
#define SLIDEO_GATE_MEMORY_MAX 64
#define SLIDEO_GATE_REF_RESET (-1)      /* ref: the frame stands behind the image of slideo_matcher_gate_reset[_from_frame_*] */
#define SLIDEO_GATE_REF_DEFERRED (-2)   /* ref: the frame is deferred and stands behind no verdict */
/* Idle matcher (SLIDEO_ERR_STATE otherwise).  Resets the gate state, also when the value does not change. */
int32_t     slideo_matcher_set_gate_memory(slideo_matcher* m, int32_t capacity);
/* The matcher's gate memory capacity (0 unless set).  SLIDEO_ERR_INVALID_ARG for a null argument. */
int32_t     slideo_matcher_gate_memory(const slideo_matcher* m, int32_t* capacity);
/* Every member idle.  More than one member: capacity > 0 is SLIDEO_ERR_UNSUPPORTED (above).  Resets the group's gate state. */
int32_t     slideo_group_set_gate_memory(slideo_group* g, int32_t capacity);
/* The ref of every frame of the last synchronous gated call (all its units, in order) or of the last collected gated ticket: the
 * ordinal of the matched frame it stands behind (its own when it was matched), SLIDEO_GATE_REF_RESET or SLIDEO_GATE_REF_DEFERRED.
 * *n is always set.  SLIDEO_ERR_CAPACITY when n > capacity or refs_out is NULL; SLIDEO_ERR_STATE when M == 0 or no gated call was
 * made since the setting.  Units may be in flight (a collect leaves them). */
int32_t     slideo_matcher_last_gate_refs(slideo_matcher* m, int64_t* refs_out, int64_t capacity, int64_t* n);
/* A group of one member: its matcher's.  More members hold no memory: SLIDEO_ERR_STATE. */
int32_t     slideo_group_last_gate_refs(slideo_group* g, int64_t* refs_out, int64_t capacity, int64_t* n);
/* Tap, idle matcher: the entries, oldest first — *count of them, their ordinals in ordinals_out [64] — and the anchor's index among
 * them.  The state "none": *count = 0, *anchor = -1.  SLIDEO_ERR_STATE when M == 0. */
int32_t     slideo_matcher_gate_memory_entries(slideo_matcher* m, int32_t* count, int32_t* anchor, int64_t* ordinals_out /*64*/);
/* Tap, idle matcher: the small image of entry `entry` (0: the oldest), unmasked.  *sw, *sh always set when entries exist;
 * SLIDEO_ERR_INVALID_ARG for an entry outside 0 .. count - 1, SLIDEO_ERR_CAPACITY when it takes more than `capacity` bytes. */
int32_t     slideo_matcher_gate_memory_small(slideo_matcher* m, int32_t entry, uint8_t* out, int64_t capacity, int32_t* sw, int32_t* sh);
/* Tap: gate_recall_kernel on its own inputs.  dot [n * n], norm [n]: the unit's, as slideo_gate_settle_walk takes them; mdot [n * M]:
 * mdot[j * M + c] = <a'_j, e'_c>, mnorm [M]: |e'_c|^2 of the carried slots; ordinals [M], count, head, anchor_slot: the carried ring
 * (slots 0 .. count - 1 are occupied, head is the slot the next match overwrites; with count < M head == count); prev_ssd0: frame 0's
 * SSD against the carried previous frame; thr_c, thr_s, max_defer (0 without a settle), d_in (0 <= d_in <= max_defer); none != 0:
 * the state "none" (nothing carried is read); t0: frame 0's ordinal; 1 <= M <= 64; 1 <= n <= 1024.
 * -> changed_out [n], ssd_out [n] (ssd_a per frame), refs_out [n], occupants_out [64] (per slot the frame of this unit that occupies
 * it behind the unit, -1: what it carried, or nothing), *head_out, *count_out, *anchor_out (a slot), *d_out.  Idle matcher. */
int32_t     slideo_gate_recall_walk(slideo_matcher* m, const uint64_t* dot, const int64_t* norm, const uint64_t* mdot, const int64_t* mnorm,
                                    const int64_t* ordinals, int32_t count, int32_t head, int32_t anchor_slot, uint64_t prev_ssd0, int32_t n,
                                    int32_t M, int64_t thr_c, int64_t thr_s, int32_t max_defer, int32_t d_in, int32_t none, int64_t t0,
                                    uint8_t* changed_out, uint64_t* ssd_out, int64_t* refs_out, int32_t* occupants_out /*64*/,
                                    int32_t* head_out, int32_t* count_out, int32_t* anchor_out, int32_t* d_out);

/* ---- Match evidence map (extension: the measurement a frame mask and a frame region can be made from, out of the matches) ----------
 * The activity map finds what moves, the content box what stands on black.  A filmed or composited lecture has neither: the slide is
 * a sub-window, and the rest of the frame — the room, a lectern, a window's chrome, a logo strip — is static and textured.  Its
 * keypoints take part of each pyramid level's retainBest quota and vote for arbitrary pages.  What tells slide from clutter exists
 * after the verdicts and only on the device: where the keypoints of matched frames fall, and which of them the winning page's
 * transform explains.
 * A matcher carries an EVIDENCE SESSION, off by default.  Its state is "none", or: a cell (16, 32 or 64), min_inliers >= 0, an
 * analysed size (aw, ah), not fixed until the first counted call; the grid gw = ceil(aw / cell), gh = ceil(ah / cell); seen[gh][gw]
 * and hit[gh][gw] as u32 (device); frames_through and frames_counted.
 * The session counts during MATCH calls (the observe calls never look at it).  Every call form that runs the verify stage counts:
 * synchronous calls and submit / collect, host and device frames, the BGR and the YUV door, gated calls, slideo_match_kept_frames,
 * slideo_match_frames_features_bgr8, and the group's forms through their members.  The first counted call fixes (aw, ah): the size
 * of the image the pipeline analyses (after the frame region's rectify or the working-size reduce).  A later call at another
 * analysed size is SLIDEO_ERR_INVALID_ARG (the message names both sizes), before anything runs.
 *   contributes      a frame contributes iff it went through the pipeline and its verdict has page_idx >= 0 && inliers >=
 *                    min_inliers.  Unchanged, deferred, recalled and direct frames of a gated call never went through it.
 *                    frames_through counts the frames that went through, frames_counted those that contribute.
 * For a contributing frame with winning page p, and M the transform of p's candidate slot exactly as slideo_last_frame_candidates
 * returns it:
 *   cell             keypoint q at (X, Y) (the slideo_keypoint floats) lies in cell ((int)X / cell, (int)Y / cell).  A keypoint
 *                    outside [0, aw) x [0, ah) (only a caller's own features can hold one) has no cell and counts nowhere.
 *   seen             seen[cell] += 1 for every keypoint of the frame.
 *   hit              q is a hit iff some vote (q, t) of the frame with train_page[t] == p has dx*dx + dy*dy <= ransac_threshold^2
 *                    IN FLOAT64, with (x, y) = page_xy[t] (the page keypoint's floats):
 *                      verify_model 0: dx = M0 x + M1 y + M2 - X, dy = M3 x + M4 y + M5 - Y;
 *                      verify_model 1: w = M6 x + M7 y + M8; w == 0: not a hit; else dx = (M0 x + M1 y + M2) / w - X, dy likewise.
 *                    Products and sums are evaluated left to right, each rounded once (no fused multiply-add).
 *                    hit[cell] += 1 per hit keypoint, once, however many of its votes pass.
 * This is the library's own definition under the FINAL (refined) transform of the winner.  It is NOT RANSAC's inlier mask: that
 * mask belongs to the sampled model before the refinement, lives in the kernel's LDS and is not kept; the sum of hit over a frame
 * need not equal the verdict's `inliers`.
 * Counters are u32 and a session holds at most 2^20 counted frames: a call that could take frames_counted past 2^20 (its frames
 * and those of the units in flight counted as if all contributed) is refused with SLIDEO_ERR_INVALID_ARG and nothing runs.  (2^20
 * frames of fewer than 4096 keypoints each cannot wrap a counter.)
 * Installing nothing: the session changes no verdict, no trace and no setting; verdict bytes are identical with and without it.
 * The caller reads the counts out, makes a mask or a box with the two pure functions below, looks at it, and hands it to
 * slideo_matcher_set_frame_mask / slideo_frame_region_from_quad + slideo_matcher_set_frame_region.  No threshold has a default:
 * they depend on the content (docs/EXTENSIONS.md "Match evidence map" says on what content it was tried).
 * What ends a session with the state "none": slideo_matcher_evidence_end; a setter that ends the kept frames AND resets the gate
 * (working size, frame region, YUV description, sampling, chroma, transfer, pixel format, levels: the analysed image is another);
 * a counted call, submit or collect that fails after its first unit was submitted (a HIP error, an overflow that cannot be served),
 * which may have counted a unit whose verdicts are never returned.  (The activity and content
 * accumulators survive a setter and refuse at the next observe; an evidence session cannot, its grid is fixed.)  The frame mask, its
 * scope, the direct settings, the gate reference and page sets leave the session open: a session may span a mask change.
 * SIFT mode is out of scope: begin in SIFT mode and slideo_matcher_use_sift under an open session are SLIDEO_ERR_UNSUPPORTED.
 * matcher 1, ratio_test, page sets (page_idx and train_page are deck indices), working size, frame region, pixel formats and levels
 * run the same verify stage and need nothing of their own.
 * Where it runs (csrc/evidence.hip.h, launched by csrc/stage_verify.hip unit_verify behind verdict_kernel on the unit's stream, only
 * while a session is open): evidence_kernel, one block of 256 threads per frame — the verdict and the winner's slot, the slot's votes
 * at qofs[f] * k + ofs[slot] tested in f64 into an LDS bitset (windows of 2048 keypoints), then the keypoints' adds, integer global
 * atomics whose result is not read.  Integer adds commute: the four units in flight share one accumulator.  A unit that is run
 * again (the RNG stream grew, a frame overflowed the keypoint capacity) raised its flag before verdict_kernel; the kernel reads the
 * unit's flags word and leaves without counting, so only the run whose verdicts are returned counts.  The kernel's per-frame body
 * is a host + device function (tools/evidence_hostcheck.cpp runs it on the CPU).
 * Every call returns SLIDEO_ERR_INVALID_ARG for a null handle or a null required pointer. */
/* Idle matcher, no session open (SLIDEO_ERR_STATE otherwise); cell other than 16, 32, 64 or min_inliers < 0: SLIDEO_ERR_INVALID_ARG;
 * SIFT mode: SLIDEO_ERR_UNSUPPORTED.  Afterwards the session is empty: no size, every count 0.  May be called before finalize. */
int32_t     slideo_matcher_evidence_begin(slideo_matcher* m, int32_t cell, int32_t min_inliers);
/* Idle matcher.  The state "none"; the device buffer is released.  Fine when the state is "none" already. */
int32_t     slideo_matcher_evidence_end(slideo_matcher* m);
/* The session's values (*aw, *ah, *gw, *gh are 0 before the first counted call); the frame counts are those of the collected units.
 * SLIDEO_ERR_STATE in the state "none". */
int32_t     slideo_matcher_evidence_info(slideo_matcher* m, int32_t* cell, int32_t* min_inliers, int32_t* aw, int32_t* ah, int32_t* gw, int32_t* gh,
                                         int64_t* frames_through, int64_t* frames_counted);
/* Idle matcher (SLIDEO_ERR_STATE with units in flight, and in the state "none").  seen_out, hit_out: gh rows of gw elements each;
 * both NULL asks for the sizes and frame counts only.  Before the first counted call *gw == *gh == 0 and nothing is written.
 * SLIDEO_ERR_CAPACITY (with the sizes set) when gw * gh > capacity_elems. */
int32_t     slideo_matcher_evidence_counts(slideo_matcher* m, uint32_t* seen_out, uint32_t* hit_out, int64_t capacity_elems, int32_t* gw,
                                           int32_t* gh, int64_t* frames_through, int64_t* frames_counted);
/* The group forms: begin and end start and end EVERY member's session (validated on every member before one is touched); info and
 * counts return the members' element-wise sums (a member whose shards were all empty has counted nothing and fixes no size).  The
 * frames limit holds per member; a summed counter that would pass UINT32_MAX is SLIDEO_ERR_CAPACITY (read the members one by one). */
int32_t     slideo_group_evidence_begin(slideo_group* g, int32_t cell, int32_t min_inliers);
int32_t     slideo_group_evidence_end(slideo_group* g);
int32_t     slideo_group_evidence_info(slideo_group* g, int32_t* cell, int32_t* min_inliers, int32_t* aw, int32_t* ah, int32_t* gw, int32_t* gh,
                                       int64_t* frames_through, int64_t* frames_counted);
int32_t     slideo_group_evidence_counts(slideo_group* g, uint32_t* seen_out, uint32_t* hit_out, int64_t capacity_elems, int32_t* gw, int32_t* gh,
                                         int64_t* frames_through, int64_t* frames_counted);
/* Two pure host functions over count arrays (no handle, no device).  seen, hit: gh rows of gw elements, gw == ceil(aw / cell) and
 * gh == ceil(ah / cell), cell 16, 32 or 64, 1 <= aw, ah <= 4096; anything else, a ppm outside 0..1000000, a negative count or one
 * above UINT32_MAX, grow outside 0..256 or stride_bytes < aw is SLIDEO_ERR_INVALID_ARG and nothing is written (SLIDEO_ERR_CAPACITY: no host memory for the grid).
 *   mask   a cell is CLUTTER iff seen >= min_seen && hit * 1000000 < min_hit_ppm * seen (unsigned 64-bit); every other cell is kept;
 *          a cell within `grow` cells (Chebyshev) of a kept cell is kept too; pixel (x, y) gets 255 if cell (x / cell, y / cell) is
 *          kept, else 0.  mask_out: ah rows of aw bytes, stride_bytes apart: what slideo_matcher_set_frame_mask takes.
 *   box    the bounding box of the cells with hit >= min_hits && hit * 1000000 >= min_hit_ppm * seen, in pixels, clipped to
 *          (aw, ah): {x0, y0, x1, y1}, x1 and y1 exclusive; all -1 when no cell qualifies.  Axis-aligned: a keystoned screen needs
 *          a quad, which "Match placement map" below learns from the matches (a similarity transform of verify_model 0 cannot express one). */
int32_t     slideo_evidence_mask(const uint32_t* seen, const uint32_t* hit, int32_t gw, int32_t gh, int32_t cell, int32_t aw, int32_t ah,
                                 int64_t min_seen, int32_t min_hit_ppm, int32_t grow, uint8_t* mask_out, int64_t stride_bytes);
int32_t     slideo_evidence_box(const uint32_t* seen, const uint32_t* hit, int32_t gw, int32_t gh, int32_t cell, int32_t aw, int32_t ah,
                                int64_t min_hits, int32_t min_hit_ppm, int32_t* box_out4);
/* Tap: the length of the pre-drawn cv::RNG stream now: SLIDEO_RNG_STREAM_LEN at creation, larger once a unit outran it and was run again. */
int32_t     slideo_matcher_rng_stream_len(const slideo_matcher* m, int64_t* len);

/* ---- Match tone table (extension: the measurement a frame levels table can be made from, out of the matches) ------------------------
 * The levels histogram ("Frame levels") is blind: it reads every pixel of the frame and stretches each channel between two
 * percentile points.  On a filmed or composited lecture the histogram is the room's, not the slide's, and a stretch is linear per
 * channel where a projector's raised black, gamma and colour cast are not.  After a match the device holds what relates the tones
 * directly: a candidate's transform, the page's small image, the analysed frame, the votes and the keypoints.
 * A matcher carries a TONE SESSION, off by default, beside the evidence session and built like it.  Its state is "none", or:
 * min_inliers >= 0, min_hits >= 1, flat in 0..255; the accumulators cnt[3][256] and sum[3][256] (u64, channel B, G, R by frame
 * value) and frames_counted (u64), all on the device; frames_through.
 * The session counts during MATCH calls.  Every call form that runs the verify stage counts, the evidence map's list: synchronous
 * calls and submit / collect, host and device frames, the BGR and the YUV door, gated calls, slideo_match_kept_frames,
 * slideo_match_frames_features_bgr8, and the group's forms through their members.  Unchanged, deferred, recalled and direct frames
 * of a gated call never went through the pipeline and never count.  frames_through counts the frames that went through.
 *   the contributor  NOT the verdict (its similarity test is what a bad tone breaks).  Of the frame's candidate slots, as
 *                    slideo_last_frame_candidates returns them, keep those whose model was found (transform not all zero) and whose
 *                    inliers >= min_inliers; the contributor is the one with the most inliers, ties to the first slot.  A frame
 *                    with no such slot does not contribute.
 * With the contributor's page p and transform M:
 *   hits             a vote (q, t) of the contributor's run is a hit under the evidence map's rule, unchanged: dx*dx + dy*dy <=
 *                    ransac_threshold^2 in float64, verify_model 0 and 1, w == 0 is no hit, left to right, no fused multiply-add.
 *                    Fewer than min_hits hits: the frame does not contribute.  The HIT BOX, in PAGE coordinates, over the hits'
 *                    page_xy[t]: bx0 = floor(min x), bx1 = ceil(max x), by0 = floor(min y), by1 = ceil(max y).
 *   samples          with (w, h) the page's size and (sw, sh) its small image's: for every pixel (i, j) of the small image, its
 *                    centre's page coordinate is x = ((i + 0.5) * w) / sw - 0.5, y = ((j + 0.5) * h) / sh - 0.5, in float64.  The
 *                    pixel is sampled iff  bx0 <= x <= bx1 && by0 <= y <= by1;  its four edge-clamped neighbours in the small image
 *                    differ from it by at most `flat` in every channel;  and (Xi, Yi) = (floor(X + 0.5), floor(Y + 0.5)) lies in
 *                    [0, aw) x [0, ah), where (X, Y) is M applied to (x, y) with the hit test's arithmetic (verify_model 1: w == 0
 *                    is no sample) and aw x ah is the analysed frame: the image the pipeline analyses, levels included.
 *                    For each channel c, with fv = frame[Yi][Xi][c] and pv = small[j][i][c]:  cnt[c][fv] += 1; sum[c][fv] += pv.
 *   frames_counted   += 1 for a frame with a contributor and at least min_hits hits.
 * Integer adds commute: the units in flight and the group's members share or sum accumulators, and no order enters.  A unit that is
 * run again counts once (the evidence kernel's flags-word rule).
 * A session holds at most 2^31 frames through (u64 cannot overflow below that): a call that could pass it (its frames and those
 * of the units in flight included) is refused with SLIDEO_ERR_INVALID_ARG and nothing runs.
 * Installing nothing: the session changes no verdict, no trace and no setting; verdict bytes are identical with and without it.
 * The caller reads the counts out, makes a table with slideo_tone_lut, looks at it, and hands it to slideo_matcher_set_frame_levels
 * (which, like every setter that changes the analysed image, ends the session).  No parameter has a default.
 * Whatever ends an evidence session ends a tone session (see there: the setters that change the analysed image, a counted call
 * that fails after its first unit was submitted), and slideo_matcher_tone_end.  The frame mask, its scope, the direct settings, the
 * gate reference and page sets leave it open.  A tone session and an evidence session may be open together; each one's results are
 * what they are alone.  SIFT mode: begin in SIFT mode and slideo_matcher_use_sift under an open session are SLIDEO_ERR_UNSUPPORTED.
 * Where it runs (csrc/tone.hip.h, launched by csrc/stage_verify.hip unit_verify behind verdict_kernel, and behind evidence_kernel
 * when both sessions are open, on the unit's stream, only while a session is open): tone_kernel, one block of 256 threads per frame
 * — the votes with the hit box through LDS min / max, then the samples into per-block LDS bins, a thread walking 32 consecutive
 * pixels of a small-image row and adding a run only when the bin changes; the block's nonzero bins go to the u64 arrays with 64-bit
 * atomics whose result is not read.  The per-frame body is host + device functions (tools/tone_hostcheck.cpp runs it on the CPU).
 * Limits: the table is a conditional mean — at text edges the area-averaged page pixel and the point-sampled frame pixel disagree,
 * and `flat` trades samples for cleanliness; a speaker in front of the slide pollutes bins in proportion to the area covered; one
 * table per channel cannot undo vignetting or a gradient; frames so dark that RANSAC finds no model teach nothing.
 * Every call returns SLIDEO_ERR_INVALID_ARG for a null handle or a null required pointer. */
/* Idle matcher, no tone session open (SLIDEO_ERR_STATE otherwise); min_inliers < 0, min_hits < 1 or flat outside 0..255:
 * SLIDEO_ERR_INVALID_ARG; SIFT mode: SLIDEO_ERR_UNSUPPORTED.  Afterwards every count is 0.  May be called before finalize. */
int32_t     slideo_matcher_tone_begin(slideo_matcher* m, int32_t min_inliers, int32_t min_hits, int32_t flat);
/* Idle matcher.  The state "none"; the device buffer is released.  Fine when the state is "none" already. */
int32_t     slideo_matcher_tone_end(slideo_matcher* m);
/* The session's settings and the frames of the collected units.  SLIDEO_ERR_STATE in the state "none". */
int32_t     slideo_matcher_tone_info(slideo_matcher* m, int32_t* min_inliers, int32_t* min_hits, int32_t* flat, int64_t* frames_through);
/* Idle matcher (SLIDEO_ERR_STATE with units in flight, and in the state "none").  cnt_out, sum_out: 3 x 256 elements each. */
int32_t     slideo_matcher_tone_counts(slideo_matcher* m, uint64_t* cnt_out /*[3][256]*/, uint64_t* sum_out /*[3][256]*/, int64_t* frames_through,
                                       int64_t* frames_counted);
/* The group forms: begin and end start and end EVERY member's session (validated on every member before one is touched); info and
 * counts return the members' sums.  The frames limit holds per member. */
int32_t     slideo_group_tone_begin(slideo_group* g, int32_t min_inliers, int32_t min_hits, int32_t flat);
int32_t     slideo_group_tone_end(slideo_group* g);
int32_t     slideo_group_tone_info(slideo_group* g, int32_t* min_inliers, int32_t* min_hits, int32_t* flat, int64_t* frames_through);
int32_t     slideo_group_tone_counts(slideo_group* g, uint64_t* cnt_out /*[3][256]*/, uint64_t* sum_out /*[3][256]*/, int64_t* frames_through,
                                     int64_t* frames_counted);
/* A pure host function in integers (no handle, no device): the levels table of the counts, what slideo_matcher_set_frame_levels
 * takes.  Per channel:  the ANCHORS are the values v with cnt[v] >= min_count;  mean[v] = (2 * sum[v] + cnt[v]) / (2 * cnt[v]);
 * m[v] is the running maximum of mean over the anchors up to v (the table is monotone);  lut[x] = m[first anchor] for x below the
 * first anchor and m[last anchor] above the last;  between neighbouring anchors a < x < b:
 * lut[x] = (2 * (m[a] * (b - x) + m[b] * (x - a)) + (b - a)) / (2 * (b - a)).
 * SLIDEO_ERR_INVALID_ARG, and nothing written: min_count < 1, a channel without an anchor, a cnt above 2^48 or a sum[v] above
 * 255 * cnt[v] (no session gives either). */
int32_t     slideo_tone_lut(const uint64_t* cnt /*[3][256]*/, const uint64_t* sum /*[3][256]*/, int64_t min_count, uint8_t* lut_out /*[3][256]*/);

/* ---- Frame lists (extension: a batch given as per-frame plane pointers) -----------------------------------------------------------
 * Every frame call above takes one base pointer and one frame_stride_bytes: frames equally spaced in one allocation, every plane of a
 * YUV frame at a fixed offset from its frame's base.  Frame sources hand out something else — one cv::Mat per sampled frame, an
 * AVFrame with data[0..2] / linesize[0..2] out of buffer pools, decoder surfaces out of a pool of allocations — and had to be copied
 * into a batch buffer first.  A FRAME LIST describes a batch by per-frame plane addresses instead; one list form of every frame-call
 * family takes it, for host and device memory, through both doors and under every frame setting the matcher carries.
 *
 * Contract: a list call returns, bit for bit, what the contiguous call of the same family returns for frames holding the same samples
 * (verdicts and candidate traces, changed flags and similarities, gate state and refs, small images, activity / content / levels /
 * evidence / tone counts).  The ABI stays 7; no existing record changes.
 *
 * The record.  `door` says how the frames are read: SLIDEO_FRAME_LIST_BGR like the *_bgr8 calls (under the matcher's pixel format),
 * SLIDEO_FRAME_LIST_YUV like the *_yuv420 calls (description, sampling, chroma filter, transfer).  `planes` is a HOST array of
 * n_frames x 3 addresses, frame i's at planes[3i .. 3i + 2]; the addresses are host or device memory by `on_device`.  stride[k] is
 * the bytes between rows of the plane at planes[3i + k], the same for every frame.  By sample address (bps, the bytes per sample, and
 * the chroma plane's size come from the matcher's depth and sampling):
 *   YUV door, planar and semi-planar   Y (x, y) at planes[3i] + y * stride[0] + x * bps;  U (cx, cy) at planes[3i + 1] + cy * stride[1]
 *                                      + cx * uv_step * bps;  V the same from planes[3i + 2] and stride[2].  uv_step 1: planar, 2:
 *                                      interleaved (planes[3i + 2] - planes[3i + 1] == +-bps, stride[1] == stride[2])
 *   YUV door, packed 4:2:2             planes[3i] is the frame's first byte, planes[3i + 1] and planes[3i + 2] are planes[3i] plus one
 *                                      of the four (u_offset, v_offset) pairs of "YUV sampling"; uv_step 4, the three strides equal
 *   BGR door, packed pixel formats     planes[3i] is the frame, stride[0] its row stride; the other two addresses are NULL (stride[1],
 *                                      stride[2] are not read)
 *   BGR door, planar RGB / BGR / GBR   three planes in the order the [N, 3, H, W] form has them; uv_step is not read through this door
 * Rules (SLIDEO_ERR_INVALID_ARG, each with a message naming it, unless stated otherwise): a NULL record or array, a needed plane
 * that is NULL and an unneeded plane that is not are refused; so are a door or an on_device outside the values above and a negative
 * n_frames; stride[k] is at least the plane's row bytes (a negative stride is refused); in 16-bit containers every address and stride
 * is even; an interleaved or packed list keeps the relations above; a uv_step the sampling does not have is refused.  The size rules
 * are the door's, with their codes (even sizes under 4:2:0, even width under the 4:2:2 forms, the image limits).  Frames and planes
 * may alias or repeat: nothing is written, there is no overlap rule.  The record and the `planes` array are copied at the call: a
 * submit form needs only the frames themselves to stay valid until collect.  Sizes and strides are the list's, not a frame's: per-frame
 * sizes, flipped (negative) strides and pages by list are not part of this.
 *
 * Where it runs.  A list is one more source form in front of the one place that stages a call's frames.  HOST lists: every plane of
 * every frame is copied into the slot's upload buffer in a tight staged layout (rows packed; planar chroma U then V; interleaved
 * chroma as one plane in the list's U / V order; packed and BGR planes row-tight) — one asynchronous copy per plane whose stride is
 * its row bytes, one 2-D copy per pitched plane; through the ordered copy stream iff every frame's first plane is page-locked.
 * DEVICE lists: one kernel (csrc/frame_list.hip.h frame_gather_kernel) gathers the planes into the same staged layout, out of a
 * pointer table uploaded with the unit.  From the staged layout on a list unit IS a host-frame unit after its upload: the
 * converters, the reduce, the rectify, the levels, the gate staging and the observe driver run as they do for host frames, and the
 * unit sizes count a device list as they count a host frame.  So a device list gives up the read-in-place shortcut of contiguous
 * device BGR8 frames: its frames are gathered into the unit's image (one extra read and write of every byte).
 *
 * Error codes and state rules (idle matcher, tickets in order, kept frames ended by an upload) are those of the contiguous twin;
 * arguments behind `list` are the twin's.  slideo_match_frames_submit_list and slideo_match_changed_frames_submit_list take device
 * lists (a host list: SLIDEO_ERR_INVALID_ARG, as the contiguous submit has no host form); the existing collect calls collect them.
 * slideo_matcher_gate_reset_from_frame_list takes a list of one.  The group forms take host lists; shards are sub-ranges of the
 * array, and a later shard is primed from the list entry before its block.  The tap returns the BGR image at source size (without
 * working size, region or levels) of every frame, back to back at row stride 3 * width: the list counterpart of
 * slideo_yuv420_to_bgr8 / slideo_pixels_to_bgr8. */
#define SLIDEO_FRAME_LIST_BGR 0   /* read like the *_bgr8 calls: under the matcher's pixel format */
#define SLIDEO_FRAME_LIST_YUV 1   /* read like the *_yuv420 calls: description, sampling, chroma filter, transfer */
typedef struct slideo_frame_list {
    int32_t door, on_device, n_frames, width, height, uv_step;
    int64_t stride[3];               /* bytes between rows of the plane at planes[3i+k] */
    const void* const* planes;       /* HOST array of n_frames x 3 addresses (host or device memory by on_device) */
} slideo_frame_list;                 /* 56 bytes */

int32_t     slideo_match_frames_list(slideo_matcher* m, const slideo_frame_list* list, slideo_verdict* verdicts_out, void* hip_stream);
int32_t     slideo_match_frames_submit_list(slideo_matcher* m, const slideo_frame_list* list, void* hip_stream, int64_t* ticket_out);
int32_t     slideo_match_changed_frames_list(slideo_matcher* m, const slideo_frame_list* list, uint8_t* changed_out, float* similarity_out,
                                             slideo_verdict* verdicts_out, void* hip_stream);
int32_t     slideo_match_changed_frames_submit_list(slideo_matcher* m, const slideo_frame_list* list, void* hip_stream, int64_t* ticket_out);
int32_t     slideo_changed_mask_list(slideo_matcher* m, const slideo_frame_list* list, const uint8_t* prev_small, uint8_t* last_small_out,
                                     uint8_t* changed_out, float* similarity_out);
int32_t     slideo_matcher_observe_frames_list(slideo_matcher* m, const slideo_frame_list* list, void* hip_stream);
int32_t     slideo_matcher_gate_reset_from_frame_list(slideo_matcher* m, const slideo_frame_list* list, void* hip_stream);
int32_t     slideo_group_match_frames_list(slideo_group* g, const slideo_frame_list* list, slideo_verdict* verdicts_out);
int32_t     slideo_group_match_changed_frames_list(slideo_group* g, const slideo_frame_list* list, uint8_t* changed_out, float* similarity_out,
                                                   slideo_verdict* verdicts_out);
int32_t     slideo_group_changed_mask_list(slideo_group* g, const slideo_frame_list* list, const uint8_t* prev_small, uint8_t* last_small_out,
                                           uint8_t* changed_out, float* similarity_out);
/* Tap: out_capacity >= n_frames * width * height * 3. */
int32_t     slideo_frame_list_to_bgr8(slideo_matcher* m, const slideo_frame_list* list, uint8_t* bgr_out, int64_t out_capacity);

/* ---- Match placement map (extension: the measurement a keystoned frame region can be made from, out of the matches) -----------------
 * The frame region ("Frame region") rectifies a fixed quadrilateral of every frame: a camera at the back of the room filming the
 * projection screen.  It needs the quad in pixels.  Under the default similarity model (verify_model 0) a candidate's transform has
 * four degrees of freedom and cannot express a keystone; what can is the pooled point correspondences of many matched frames: each
 * keypoint's frame position against where its page point lies on the slide.  They exist only on the device, per unit.
 * A matcher carries a PLACEMENT SESSION, off by default, beside the evidence and tone sessions and built like the evidence session.
 * Its state is "none", or: a cell (16, 32 or 64), min_inliers >= 0, reach (a finite double > 0, pixels of the analysed image), an
 * analysed size (aw, ah), not fixed until the first counted call; the grid gw = ceil(aw / cell), gh = ceil(ah / cell); five sums
 * n, sfx, sfy, su, sv [gh][gw] and frames_counted, all u64 on the device; frames_through.
 * The evidence map's rules hold unchanged wherever this text does not say otherwise: the call forms that count (every form that
 * runs the verify stage; unchanged, deferred, recalled and direct frames of a gated call never count), the first counted call
 * fixing (aw, ah) and the SLIDEO_ERR_INVALID_ARG of a later call at another analysed size (the message names both sizes), what
 * ends a session (slideo_matcher_placement_end, the setters that change the analysed image, a counted call that fails after its
 * first unit was submitted) and what leaves it open, the idle and state rules, SIFT mode (SLIDEO_ERR_UNSUPPORTED in either order),
 * and a unit that is run again counting once through the unit's flags word.  Any combination of the three sessions may be open at
 * once; each one's results are what they are alone.
 *   the contributor  the tone table's, NOT the verdict's winner (an unrectified keystone is exactly what pushes the re-projection
 *                    similarity under min_similarity and removes the verdict): of the frame's candidate slots, as
 *                    slideo_last_frame_candidates returns them, those whose model was found (transform not all zero) and whose
 *                    inliers >= min_inliers; the one with the most inliers, ties to the first slot.  A frame with no such slot
 *                    does not contribute.  frames_counted += 1 for a frame with a contributor.
 * With the contributor's page p of full size (pw, ph) and its transform M:
 *   residual         for each vote (q, t) of the contributor's run, d2 = dx*dx + dy*dy as the evidence map computes it, under both
 *                    verify_model values: in float64, left to right, each operation rounded once, no fused multiply-add; w == 0 or
 *                    a non-finite d2: the vote does not pass.  The vote PASSES iff d2 <= reach * reach.  reach is the session's own
 *                    radius and may exceed ransac_threshold: under a keystone the similarity fits only part of the screen within
 *                    3 px, and the correspondences further out are the ones the fit needs.
 *   one per keypoint a keypoint q with at least one passing vote contributes once, through its passing vote of smallest d2, ties to
 *                    the smallest train row t.  The order in which the votes are stored does not matter.
 *   coordinates      the keypoint's floats (X, Y) and (x, y) = page_xy[t].  A keypoint outside [0, aw) x [0, ah), a page point
 *                    outside [0, pw - 1] x [0, ph - 1], and a page with pw < 2 or ph < 2 contribute nothing.
 *   sums             otherwise, into cell ((int)X / cell, (int)Y / cell):  n += 1;  sfx += rint(X * 16);  sfy += rint(Y * 16);
 *                    su += rint(x / (double)(pw - 1) * 1048576.0);  sv += rint(y / (double)(ph - 1) * 1048576.0), in float64 with
 *                    round-half-even.  (su, sv) / n / 2^20 is the position on the UNIT SLIDE whose corners are the page's corner
 *                    pixel centres — the convention of slideo_frame_region_from_quad —, so pages of different sizes share one
 *                    accumulator.
 * A session holds at most 2^20 frames through: a call that could pass it (its frames and those of the units in flight included) is
 * refused with SLIDEO_ERR_INVALID_ARG and nothing runs.  Bound: 2^20 frames of fewer than 4096 keypoints each adding at most 2^20
 * keep every sum below 2^52, far inside u64 and exact in a double.
 * Installing nothing: the session changes no verdict, no trace and no setting; verdict bytes are identical with and without it.  The
 * caller reads the sums out, fits a quad with slideo_placement_quad, looks at it, and hands it to slideo_frame_region_from_quad +
 * slideo_matcher_set_frame_region.  No threshold has a default.
 * Where it runs (csrc/placement.hip.h, launched by csrc/stage_verify.hip unit_verify behind verdict_kernel, and behind
 * evidence_kernel and tone_kernel when those sessions are open, on the unit's stream, only while a session is open):
 * placement_kernel, one block of 256 threads per frame, by windows of 2048 keypoints — the votes' d2 patterns into LDS with a 64-bit
 * unsigned min (the pattern of a non-negative finite double orders as the double does), the rows of the votes at the minimum with a
 * 32-bit min, then per keypoint with a winner five 64-bit global atomic adds whose result is not read.  24 KB of LDS, no
 * compare-and-swap loop.  The per-frame body is host + device functions (tools/placement_hostcheck.cpp runs it on the CPU).
 * Limits: the estimator assumes a FIXED camera and screen over the session; a moving camera smears the cells.  SIFT mode, weighting
 * the cells, a geometric refinement of the fit and installing the region are out of scope.
 * Every call returns SLIDEO_ERR_INVALID_ARG for a null handle or a null required pointer. */
/* Idle matcher, no placement session open (SLIDEO_ERR_STATE otherwise); cell other than 16, 32, 64, min_inliers < 0, or a reach that
 * is not above 0 or whose square is not finite: SLIDEO_ERR_INVALID_ARG; SIFT mode: SLIDEO_ERR_UNSUPPORTED.  Afterwards the session
 * is empty: no size, every sum 0.  May be called before finalize. */
int32_t     slideo_matcher_placement_begin(slideo_matcher* m, int32_t cell, int32_t min_inliers, double reach);
/* Idle matcher.  The state "none"; the device buffer is released.  Fine when the state is "none" already. */
int32_t     slideo_matcher_placement_end(slideo_matcher* m);
/* The session's values (*aw, *ah, *gw, *gh are 0 before the first counted call) and the frames of the collected units.
 * SLIDEO_ERR_STATE in the state "none". */
int32_t     slideo_matcher_placement_info(slideo_matcher* m, int32_t* cell, int32_t* min_inliers, double* reach, int32_t* aw, int32_t* ah, int32_t* gw,
                                          int32_t* gh, int64_t* frames_through);
/* Idle matcher (SLIDEO_ERR_STATE with units in flight, and in the state "none").  The five arrays: gh rows of gw elements each; all
 * five NULL asks for the sizes and frame counts only (some NULL: SLIDEO_ERR_INVALID_ARG).  Before the first counted call *gw == *gh
 * == 0 and nothing is written.  SLIDEO_ERR_CAPACITY (with the sizes set) when gw * gh > capacity_elems. */
int32_t     slideo_matcher_placement_sums(slideo_matcher* m, uint64_t* n_out, uint64_t* sfx_out, uint64_t* sfy_out, uint64_t* su_out, uint64_t* sv_out,
                                          int64_t capacity_elems, int32_t* gw, int32_t* gh, int64_t* frames_through, int64_t* frames_counted);
/* The group forms: begin and end start and end EVERY member's session (validated on every member before one is touched); info and
 * sums return the members' element-wise sums (a member whose shards were all empty fixes no size).  The frames limit holds per member. */
int32_t     slideo_group_placement_begin(slideo_group* g, int32_t cell, int32_t min_inliers, double reach);
int32_t     slideo_group_placement_end(slideo_group* g);
int32_t     slideo_group_placement_info(slideo_group* g, int32_t* cell, int32_t* min_inliers, double* reach, int32_t* aw, int32_t* ah, int32_t* gw, int32_t* gh,
                                        int64_t* frames_through);
int32_t     slideo_group_placement_sums(slideo_group* g, uint64_t* n_out, uint64_t* sfx_out, uint64_t* sfy_out, uint64_t* su_out, uint64_t* sv_out,
                                        int64_t capacity_elems, int32_t* gw, int32_t* gh, int64_t* frames_through, int64_t* frames_counted);
/* A pure host function in float64 (no handle, no device): the quad of the sums.  The grid is validated as slideo_evidence_box
 * validates its own (gw == ceil(aw / cell), gh == ceil(ah / cell), cell 16, 32 or 64, 1 <= aw, ah <= 4096); min_count >= 1,
 * trim_px finite and > 0, rounds in 0..8; a count above 2^32 or a sum above its count times 2^16 (sfx, sfy) or 2^20 (su, sv): no
 * session gives them.
 *   points   every cell with n >= min_count is ONE point, unweighted: (u, v) = (su / n / 2^20, sv / n / 2^20), (X, Y) = (sfx / n
 *            / 16, sfy / n / 16).  The cell mean is an ESTIMATOR: the mean of images is not the image of the mean under a
 *            homography; the difference is second-order over a cell.  It assumes a fixed camera and screen.
 *   fit      H = [[h0 h1 h2] [h3 h4 h5] [h6 h7 1]] mapping (u, v) to (X, Y) / s, s = max(aw, ah): the least-squares solution of
 *            two linear equations per point,  h0 u + h1 v + h2 - xh u h6 - xh v h7 = xh  and  h3 u + h4 v + h5 - yh u h6 - yh v h7
 *            = yh,  with (xh, yh) = (X, Y) / s; by a Householder QR with column pivoting.  Rank deficient: a diagonal entry of R
 *            at or below 1e-10 of the first.
 *   trim     at most `rounds` times: a point's residual is the pixel distance between s * H(u, v) and (X, Y); the points of the
 *            current set with a residual above trim_px (or none, w == 0) are dropped; if none was, stop; otherwise refit.
 *   outputs  quad_out8: s * H applied to (0,0), (1,0), (1,1), (0,1) — top-left, top-right, bottom-right, bottom-left as x, y pairs,
 *            exactly what slideo_frame_region_from_quad takes; H_out9 row-major; cells_used, the points of the last fit; rms_px,
 *            the root mean square of their residuals.
 * SLIDEO_ERR_INVALID_ARG, and nothing written: a bad argument, fewer than 4 points at any stage, a rank-deficient system, a corner
 * that does not come out finite.  SLIDEO_ERR_CAPACITY: no host memory for the system. */
int32_t     slideo_placement_quad(const uint64_t* n, const uint64_t* sfx, const uint64_t* sfy, const uint64_t* su, const uint64_t* sv, int32_t gw,
                                  int32_t gh, int32_t cell, int32_t aw, int32_t ah, int64_t min_count, double trim_px, int32_t rounds,
                                  double* quad_out8, double* H_out9, int32_t* cells_used, double* rms_px);

/* ---- Placement lens (extension: the frame lens and the quad learnt jointly from the placement session's sums) ------------------------
 * Under lens distortion a homography fits only a patch of the screen, and slideo_placement_quad's trim drops exactly the outer cells
 * that carry the signal.  slideo_placement_lens fits H and the radial terms of "Frame lens" JOINTLY to the sums a placement session
 * gives when it ran with NO lens and NO region set.  A pure host function in float64 (no handle, no device); it installs nothing.
 * Arguments: the grid, min_count, trim_px and rounds as slideo_placement_quad validates them; cx, cy finite, f > 0 (the lens's centre
 * and normaliser, GIVEN, not learnt); order 1 (k1) or 2 (k1 and k2); iters in 1..1000.
 *   points   slideo_placement_quad's: a cell with n >= min_count is one unweighted correspondence (u, v) -> (X, Y).
 *   model    P = s * H(u, v), s = max(aw, ah), H = [[h0 h1 h2] [h3 h4 h5] [h6 h7 1]] — the ideal pixel of the unit-slide point —,
 *            D(P) = c + (P - c) (1 + k1 r2 + k2 r2^2), r2 = |P - c|^2 / f^2; the residual of a point is D(P) - (X, Y), in pixels.
 *            Parameters: h0 .. h7 (scaled by s as slideo_placement_quad scales them), k1 and, at order 2, k2 (0 at order 1).
 *   start    slideo_placement_quad's linear fit over ALL points, WITHOUT trimming; k = 0.
 *   iterate  at most `iters` damped Gauss-Newton steps with the analytic Jacobian J: with A = J^T J and g = J^T r, the step solves
 *            (A + lambda diag(A)) d = -g (Cholesky on the system scaled to a unit diagonal); lambda starts at 1e-3 on every run
 *            of the iteration.  A step that lowers the cost C = |r|^2 is taken and lambda becomes max(lambda / 10, 1e-12); the
 *            iteration stops when the taken step lowered C by no more than 1e-12 C, or when C is 0.  A step that does not lower C
 *            (or leaves a point without a finite image) is not taken and lambda becomes 10 lambda; the iteration stops when lambda
 *            exceeds 1e8.  Either kind of step counts towards `iters`.  After the iteration the UNDAMPED A at the result must have
 *            full rank: a Cholesky pivot of the unit-diagonal A at or below 1e-12 refuses.
 *   trim     at most `rounds` times: the points further than trim_px from the joint fit (or without an image) are dropped; if none
 *            was, stop; otherwise the iteration runs again from the current parameters.
 *   outputs  k_out2 = (k1, k2); H_out9 row-major, mapping the unit slide to IDEAL pixels (rows 0 and 1 multiplied by s); quad_out8
 *            its images of (0,0), (1,0), (1,1), (0,1) in ideal coordinates — exactly what slideo_frame_region_from_quad takes while
 *            that lens is set —; cells_used and rms_px of the last fit.
 * SLIDEO_ERR_INVALID_ARG, and nothing written: a bad argument; fewer than 4 + order points at any stage; a rank-deficient or
 * non-finite step; a result whose radial map is not strictly increasing (the rule of "Frame lens") up to the largest r2 of the kept
 * cells' ideal points.  SLIDEO_ERR_CAPACITY: no host memory. */
int32_t     slideo_placement_lens(const uint64_t* n, const uint64_t* sfx, const uint64_t* sfy, const uint64_t* su, const uint64_t* sv, int32_t gw,
                                  int32_t gh, int32_t cell, int32_t aw, int32_t ah, int64_t min_count, double cx, double cy, double f, int32_t order,
                                  double trim_px, int32_t rounds, int32_t iters, double* k_out2, double* quad_out8, double* H_out9,
                                  int32_t* cells_used, double* rms_px);

/* ---- Match shading map (extension: the measurement a frame shading can be made from, out of the matches) ------------------------------
 * The frame shading ("Frame shading") needs its gains.  What can give them is what the tone table is learnt from — the pixel pairs
 * (frame pixel, page small-image pixel) that a matched frame's contributing candidate puts in correspondence — binned by WHERE they
 * lie in the analysed frame instead of by their value: the ratio of the page side's sum to the frame side's sum over a cell is the
 * gain that cell wants.
 * A matcher carries a SHADING SESSION, off by default, beside the evidence, tone and placement sessions and built like the placement
 * session.  Its state is "none", or: a cell (16, 32 or 64), min_inliers >= 0, min_hits >= 1, flat in 0..255, an analysed size (aw,
 * ah), not fixed until the first counted call; the grid gw = ceil(aw / cell), gh = ceil(ah / cell); three sums cnt, sum_f, sum_p
 * [gh][gw] and frames_counted, all u64 on the device; frames_through.
 * Everything up to the sample is the tone table's ("Match tone table"), unchanged: the contributor (the candidate slot with a model
 * and the most inliers, at least min_inliers, ties to the first slot), its hits by the evidence map's float64 test (at least
 * min_hits of them), the hit box in page coordinates, and the sample test — a small-image pixel (i, j) is a sample iff its centre lies
 * in the box, its four edge-clamped neighbours differ from it by at most `flat` in every channel, and (Xi, Yi) = (floor(X + 0.5),
 * floor(Y + 0.5)) lies in the analysed frame.  For a sample, with k = (Yi / cell) * gw + Xi / cell:
 *   cnt[k] += 1;  sum_f[k] += B + G + R of the frame pixel (Xi, Yi);  sum_p[k] += B + G + R of the small-image pixel (i, j)
 * and frames_counted += 1 per contributing frame.
 * The placement map's rules hold unchanged wherever this text does not say otherwise: the call forms that count, the first counted
 * call fixing (aw, ah) and the SLIDEO_ERR_INVALID_ARG of a later call at another analysed size (the message names both sizes), what
 * ends a session (slideo_matcher_shading_end, the setters that change the analysed image — the frame shading's and the levels' own
 * among them —, a counted call that fails after its first unit was submitted), the idle and state rules, SIFT mode
 * (SLIDEO_ERR_UNSUPPORTED in either order), and a unit that is run again counting once.  Any combination of the four sessions may be
 * open at once; each one's results are what they are alone.  Verdict bytes are identical with and without a session.
 * Its own rules: begin is refused with SLIDEO_ERR_STATE while a frame shading is set (a field learnt on shaded frames is not the
 * source's) and while a frame levels table is set (a gain learnt behind the table cannot be installed in front of it: learn the field
 * first and the table second).  A grid of more than 4096 cells is refused at the first counted call with SLIDEO_ERR_UNSUPPORTED, the
 * next cell size named (1080p at cell 32 and 4K at cell 64 have 2040).  A session holds at most 2^20 frames through.
 * Installing nothing: the caller reads the sums out, makes a field with slideo_shading_field ("Frame shading"), looks at it, and hands
 * it to slideo_matcher_set_frame_shading.  No parameter has a default.
 * Where it runs (csrc/shading.hip.h, launched by csrc/stage_verify.hip unit_verify behind verdict_kernel and the other sessions'
 * kernels, on the unit's stream, only while a session is open): shading_map_kernel, one block of 256 threads per frame; the tone
 * kernel's phase 1; work items of 32 consecutive small-image pixels whose thread keeps one cell index with a run count and two run
 * sums and adds to the block's u32 bins [3][cells] in LDS (at most 48 KB) only when the cell changes; row tiles of at most 2^22
 * pixels; the nonzero bins go to the u64 arrays with 64-bit atomics whose result is not read.
 * Limits: the estimator is a ratio of sums, dominated by the bright background; a speaker or an occluder biases the cells it covers;
 * clipped highlights bias low; a FIXED camera and screen are assumed; cell 16 needs more frames than cell 32.
 * Every call returns SLIDEO_ERR_INVALID_ARG for a null handle or a null required pointer. */
/* Idle matcher, no shading session open, no frame shading and no frame levels set (SLIDEO_ERR_STATE otherwise); cell other than 16,
 * 32, 64, min_inliers < 0, min_hits < 1 or flat outside 0..255: SLIDEO_ERR_INVALID_ARG; SIFT mode: SLIDEO_ERR_UNSUPPORTED.  Afterwards
 * the session is empty: no size, every sum 0.  May be called before finalize. */
int32_t     slideo_matcher_shading_begin(slideo_matcher* m, int32_t cell, int32_t min_inliers, int32_t min_hits, int32_t flat);
/* Idle matcher.  The state "none"; the device buffer is released.  Fine when the state is "none" already. */
int32_t     slideo_matcher_shading_end(slideo_matcher* m);
/* The session's values (*aw, *ah, *gw, *gh are 0 before the first counted call) and the frames of the collected units.
 * SLIDEO_ERR_STATE in the state "none". */
int32_t     slideo_matcher_shading_info(slideo_matcher* m, int32_t* cell, int32_t* min_inliers, int32_t* min_hits, int32_t* flat, int32_t* aw,
                                        int32_t* ah, int32_t* gw, int32_t* gh, int64_t* frames_through);
/* Idle matcher (SLIDEO_ERR_STATE with units in flight, and in the state "none").  The three arrays: gh rows of gw elements each; all
 * three NULL asks for the sizes and frame counts only (some NULL: SLIDEO_ERR_INVALID_ARG).  Before the first counted call *gw == *gh
 * == 0 and nothing is written.  SLIDEO_ERR_CAPACITY (with the sizes set) when gw * gh > capacity_elems. */
int32_t     slideo_matcher_shading_sums(slideo_matcher* m, uint64_t* cnt_out, uint64_t* sum_f_out, uint64_t* sum_p_out, int64_t capacity_elems,
                                        int32_t* gw, int32_t* gh, int64_t* frames_through, int64_t* frames_counted);
/* The group forms: begin and end start and end EVERY member's session (validated on every member before one is touched); info and
 * sums return the members' element-wise sums (a member whose shards were all empty fixes no size).  The frames limit holds per member. */
int32_t     slideo_group_shading_begin(slideo_group* g, int32_t cell, int32_t min_inliers, int32_t min_hits, int32_t flat);
int32_t     slideo_group_shading_end(slideo_group* g);
int32_t     slideo_group_shading_info(slideo_group* g, int32_t* cell, int32_t* min_inliers, int32_t* min_hits, int32_t* flat, int32_t* aw, int32_t* ah,
                                      int32_t* gw, int32_t* gh, int64_t* frames_through);
int32_t     slideo_group_shading_sums(slideo_group* g, uint64_t* cnt_out, uint64_t* sum_f_out, uint64_t* sum_p_out, int64_t capacity_elems, int32_t* gw,
                                      int32_t* gh, int64_t* frames_through, int64_t* frames_counted);

#ifdef __cplusplus
}
#endif
#endif /* SLIDEO_AMD_H */
