// capi_group.hip — slideo_group_*: one matcher per device behind ONE handle (include/slideo_amd.h, "N-device group").
//
// The reference fans a video's frames out over every core of the machine (rayon: one task per changed frame,
// crates/matching-opencv/src/lib.rs:174,213) and its pages over the same pool (lib.rs:45-47).  The N-device counterpart: the
// page database is REPLICATED on every device (0.45 GB at 1000 pages against 288 GB of HBM), a call's
// frames are cut into contiguous shards, one per device, each shard runs through its device's matcher on a host thread of its
// own, and every shard's verdict records land in the caller's array at the shard's offset — the gather of the in-process
// form is the D2H copy each device makes anyway, so there is no collective here (one process per GPU, where every rank wants
// the whole timeline, is bench.py / slideo_amd/distributed.py: ONE RCCL all-gather of the 16-byte records).
// Page analysis is sharded the same way (ProcessedImage::compute is independent per page): device d analyses its share of a
// call's pages and every member appends the whole call, in page order, from the host records.
//
// No kernel lives in this unit; it only drives the members through the functions of runtime.hpp.
#include "runtime.hpp"
#include "gate_baton.h"

#include <thread>

using namespace slideo;

struct slideo_group {
    std::vector<slideo_matcher*> members;
    std::string err;
    slideo_progress_fn progress = nullptr;
    void* progress_user = nullptr;
    // progress of a sharded call: the members report their own (done, total); the group reports the sum
    struct Tramp { slideo_group* g = nullptr; uint64_t last = 0; };
    std::vector<Tramp> tramps;
    // (reports are serialised: one member thread at a time advances `done` and calls the sink, so a sink sees a monotonic count
    // and is never entered twice at once — what a single matcher's caller gets)
    std::mutex progress_mutex;
    uint64_t done = 0;
    uint64_t total = 0;
    const char* msg_override = nullptr;
    // shards of the last match call (trace lookup) and of the last changed-mask call (kept frames)
    std::vector<int> match_lo;           // n + 1 bounds
    struct KeptShard { int read_lo = 0, lo = 0, hi = 0; };
    std::vector<KeptShard> kept;
    bool kept_valid = false;
    // the group's ONE gate state (include/slideo_amd.h "Changed-frame gate", the group's form).  Its small image lives in the gate
    // state of member gate_owner (the last non-empty shard's member of the last gated call), or, gate_owner -1, in gate_small (a
    // reset's prev_small); the next gated call moves it to member 0, where the call's first frame is compared.
    slideo_matcher::GateState gate;
    int gate_owner = -1;
    std::vector<uint8_t> gate_small;
    // group gate order (include/slideo_amd.h "Group gate order").  Under CHAIN link r carries the gate state member r leaves behind
    // its last frame to member r + 1: a pinned record {d | anchor | previous image} of the group's and the baton that says it is there.
    uint32_t gate_order = SLIDEO_GROUP_GATE_HALO;
    struct GateLink {
        GateBaton baton;
        void* rec = nullptr;
        size_t cap = 0;
        double waited_s = 0.0;                // how long member r + 1 blocked on the baton in the last chained call
        ~GateLink() { if (rec) (void)hipHostFree(rec); }
        void reserve(size_t bytes) {
            if (bytes <= cap) return;
            if (rec) (void)hipHostFree(rec);
            rec = nullptr; cap = 0;
            HIP_CHECK(hipHostMalloc(&rec, bytes, hipHostMallocPortable));      // (read by the next member's device, written by this one's)
            cap = bytes;
        }
    };
    std::vector<std::unique_ptr<GateLink>> gate_links;      // members - 1
    std::vector<uint8_t> gate_rec;                          // the state on its way to member 0, as a record
};

namespace {

std::string g_group_create_error;
std::mutex g_group_err_mutex;

void set_group_err(slideo_group* g, const char* what) {
    if (g) g->err = what;
    else { std::lock_guard<std::mutex> lk(g_group_err_mutex); g_group_create_error = what; }
}

// contiguous block [lo, hi) of member r (block sizes differ by at most one): slideo_amd/distributed.py shard_range
void shard_range(int n, int r, int world, int& lo, int& hi) {
    const int base = n / world, rem = n % world;
    lo = r * base + std::min(r, rem);
    hi = lo + base + (r < rem ? 1 : 0);
}

void group_progress_tramp(void* user, uint64_t done, uint64_t total, const char* msg) {
    auto* t = static_cast<slideo_group::Tramp*>(user);
    slideo_group* g = t->g;
    (void)total;
    if (!g->progress || done <= t->last) { t->last = std::max(t->last, done); return; }
    const uint64_t d = done - t->last;
    t->last = done;
    std::lock_guard<std::mutex> lk(g->progress_mutex);
    g->done += d;
    g->progress(g->progress_user, std::min(g->done, g->total), g->total, g->msg_override ? g->msg_override : msg);
}

// fn(member index) on one host thread per member; the first failure (lowest member) is rethrown on the caller's thread
template <class F>
void for_each_member(slideo_group* g, F fn) {
    const int n = (int)g->members.size();
    std::vector<int32_t> code((size_t)n, SLIDEO_OK);
    std::vector<std::string> what((size_t)n);
    auto body = [&](int r) {
        try { fn(r); }
        catch (const slideo::Error& e) { code[r] = e.code; what[r] = e.what(); }
        catch (const std::exception& e) { code[r] = SLIDEO_ERR_HIP; what[r] = e.what(); }
        catch (...) { code[r] = SLIDEO_ERR_HIP; what[r] = "unknown error"; }
    };
    if (n == 1) body(0);
    else {
        std::vector<std::thread> th;
        th.reserve((size_t)n);
        try {
            for (int r = 0; r < n; ++r) th.emplace_back(body, r);
        } catch (...) {                                     // (a thread could not be started: the members it would have driven run here)
            for (int r = (int)th.size(); r < n; ++r) body(r);
        }
        for (auto& t : th) t.join();
    }
    for (int r = 0; r < n; ++r)
        if (code[r] != SLIDEO_OK) fail(code[r], "device member %d (device %d): %s", r, g->members[r]->device, what[r].c_str());
}

void check_member_call(slideo_matcher* m, int32_t rc) {
    if (rc != SLIDEO_OK) fail(rc, "%s", slideo_last_error(m));
}

void begin_progress(slideo_group* g, uint64_t total, const char* msg_override) {
    g->done = 0; g->total = total; g->msg_override = msg_override;
    for (auto& t : g->tramps) t.last = 0;
}

// slideo_group_match_frames_bgr8 / _yuv420
void group_match_impl(slideo_group* g, int32_t n_frames, const FrameSrc& src, slideo_verdict* verdicts_out) {
    if (n_frames < 0 || (n_frames > 0 && (!src.p || !verdicts_out))) fail(SLIDEO_ERR_INVALID_ARG, "null frames/verdicts");
    const int N = (int)g->members.size();
    begin_progress(g, (uint64_t)n_frames, nullptr);
    g->match_lo.assign((size_t)N + 1, 0);
    for (int r = 0; r < N; ++r) { int lo, hi; shard_range(n_frames, r, N, lo, hi); g->match_lo[r] = lo; g->match_lo[r + 1] = hi; }
    g->kept_valid = false;
    for_each_member(g, [&](int r) {
        const int lo = g->match_lo[r], hi = g->match_lo[r + 1];
        // (an empty shard still runs the call's checks: every member reports a matcher that was never finalized, say)
        match_frames_impl(g->members[r], hi - lo, src.from(lo), verdicts_out + lo, nullptr);
    });
}

// slideo_group_changed_mask_bgr8 / _yuv420 (every member's kept frames are the BGR images of its block)
void group_mask_impl(slideo_group* g, int32_t n_frames, const FrameSrc& src, const uint8_t* prev_small, uint8_t* last_small_out,
                     uint8_t* changed_out, float* similarity_out) {
    if (n_frames < 0 || (n_frames > 0 && (!src.p || !changed_out))) fail(SLIDEO_ERR_INVALID_ARG, "null frames/changed");
    g->kept_valid = false;
    if (n_frames == 0) return;
    const int N = (int)g->members.size();
    // MarkSimilarIter compares every sampled frame with the one before it (video_capture.rs:86-98): a shard reads ONE frame
    // before its block (the halo; slideo_amd/distributed.py halo_range) and drops that frame's own flag.
    g->kept.assign((size_t)N, slideo_group::KeptShard{});
    int last_r = 0;
    for (int r = 0; r < N; ++r) {
        int lo, hi;
        shard_range(n_frames, r, N, lo, hi);
        g->kept[r] = slideo_group::KeptShard{(lo > 0 && hi > lo) ? lo - 1 : lo, lo, hi};
        if (hi > lo) last_r = r;
    }
    for_each_member(g, [&](int r) {
        const slideo_group::KeptShard k = g->kept[r];
        if (k.hi <= k.lo) return;
        const int cnt = k.hi - k.read_lo, halo = k.lo - k.read_lo;
        std::vector<uint8_t> ch((size_t)cnt);
        std::vector<float> sim((size_t)cnt);
        changed_mask_impl(g->members[r], cnt, src.from(k.read_lo), r == 0 ? prev_small : nullptr, r == last_r ? last_small_out : nullptr,
                          ch.data(), sim.data());
        for (int i = halo; i < cnt; ++i) {
            changed_out[k.read_lo + i] = ch[i];
            if (similarity_out) similarity_out[k.read_lo + i] = sim[i];
        }
    });
    g->kept_valid = true;
}

void group_gate_none(slideo_group* g) {
    g->gate = slideo_matcher::GateState{};
    g->gate_owner = -1;
}

// Group gate order CHAIN: the hand-over of one gated call over members 0 .. last_r (the non-empty shards), small images of sw x sh.
// Link r's record: {d u32, 12 bytes unused | anchor sb | previous image sb}.  Member r > 0 is told on the host that it holds a state
// of that size — its predecessor, a non-empty shard, always leaves one —, so its first unit reserves the state buffers and is
// submitted at once; where that unit waits for the state (runtime.hpp gate_chain_receive) its thread blocks on the baton and then
// queues the record's copy on the unit's stream.  Member r < last_r copies its state out behind its last unit's write of it
// (Slot::ev_gate) and publishes.  The links' records are reserved here, before any member is touched.
void gate_chain_arm(slideo_group* g, int last_r, int sw, int sh) {
    const size_t sb = (size_t)sw * sh * 3;
    for (int r = 0; r < last_r; ++r) {
        slideo_group::GateLink& L = *g->gate_links[r];
        L.reserve(16 + 2 * sb);
        L.baton.reset();
        L.waited_s = 0.0;
    }
    for (int r = 0; r <= last_r; ++r) {
        slideo_matcher* m = g->members[r];
        if (r > 0) {
            slideo_group::GateLink* in = g->gate_links[r - 1].get();
            m->gate = slideo_matcher::GateState{};
            m->gate.has = true; m->gate.sw = sw; m->gate.sh = sh;
            m->gate_receive = [m, in, sb](hipStream_t st) {
                in->waited_s = in->baton.await();
                uint8_t* p = static_cast<uint8_t*>(in->rec);
                gate_state_write(m, sb, p + 16, p + 16 + sb, reinterpret_cast<const uint32_t*>(p), st);
            };
        }
        if (r < last_r) {
            slideo_group::GateLink* out = g->gate_links[r].get();
            m->gate_publish = [m, out, sb](Slot& S) {
                uint8_t* p = static_cast<uint8_t*>(out->rec);
                gate_state_read(m, S.ev_gate, sb, p + 16, p + 16 + sb, reinterpret_cast<uint32_t*>(p));
                out->baton.publish();
            };
        }
    }
}

// slideo_group_match_changed_frames_bgr8 / _yuv420: member 0 continues the group's gate state; every later non-empty shard [lo, hi)
// primes its member from frame lo - 1 (the one-frame halo of group_mask_impl, as a gate state) and runs the single matcher's gated
// call over its block.  The pairs compared, the small images and the pipeline of the changed frames are the single matcher's.
// Under the group gate order CHAIN (gate_chain_arm above) no shard is primed: every later member receives its predecessor's whole
// state where its first unit waits for it, and the state travels to member 0 between calls as a record.
void group_gated_impl(slideo_group* g, int32_t n_frames, const FrameSrc& src, uint8_t* changed_out, float* similarity_out,
                      slideo_verdict* verdicts_out) {
    const int N = (int)g->members.size();
    slideo_matcher* m0 = g->members[0];
    // the whole call's checks once, before any member is touched: an error leaves the gate state as it was
    if (n_frames > 0 && !changed_out) fail(SLIDEO_ERR_INVALID_ARG, "null changed_out");
    FrameSrc checked = src;
    validate_frames(checked, m0, n_frames, verdicts_out);
    gate_check(g->gate, checked);
    for (slideo_matcher* m : g->members) require_idle(m);
    if (n_frames == 0) return;                      // a no-op: the state, the last call's traces and a mask call's kept frames stay
    g->match_lo.assign((size_t)N + 1, 0);
    g->kept_valid = false;
    begin_progress(g, (uint64_t)n_frames, nullptr);
    // (a group of one never chains: it forwards)
    const bool chain = g->gate_order == SLIDEO_GROUP_GATE_CHAIN && N > 1;
    // whatever happens, no member keeps a hook of this call
    struct Unhook {
        slideo_group* g;
        ~Unhook() { for (slideo_matcher* m : g->members) { m->gate_receive = nullptr; m->gate_publish = nullptr; } }
    } unhook{g};
    try {
        // the state to member 0
        if (g->gate_owner != 0) {
            if (!g->gate.has) check_member_call(m0, slideo_matcher_gate_reset(m0, nullptr, 0, 0));
            else if (chain && g->gate_owner > 0) {
                // the whole state, as a record: under a settle the previous frame and the deferral count travel too
                slideo_matcher* o = g->members[g->gate_owner];
                int64_t bytes = 0;
                check_member_call(o, slideo_matcher_gate_state_bytes(o, &bytes));
                g->gate_rec.resize((size_t)bytes);
                check_member_call(o, slideo_matcher_gate_state_export(o, g->gate_rec.data(), bytes, &bytes));
                check_member_call(m0, slideo_matcher_gate_state_import(m0, g->gate_rec.data(), bytes));
                if (!m0->gate.has || m0->gate.sw != g->gate.sw || m0->gate.sh != g->gate.sh)
                    fail(SLIDEO_ERR_STATE, "member %d holds a %dx%d gate state (%d), the group's is %dx%d (a member was gated directly)", g->gate_owner,
                         m0->gate.sw, m0->gate.sh, (int)m0->gate.has, g->gate.sw, g->gate.sh);
            } else {
                if (g->gate_owner > 0) {
                    slideo_matcher* o = g->members[g->gate_owner];
                    int32_t sw = 0, sh = 0;
                    g->gate_small.resize((size_t)g->gate.sw * g->gate.sh * 3);
                    check_member_call(o, slideo_matcher_gate_last_small(o, g->gate_small.data(), (int64_t)g->gate_small.size(), &sw, &sh));
                    if (sw != g->gate.sw || sh != g->gate.sh)
                        fail(SLIDEO_ERR_STATE, "member %d holds a %dx%d small image, the group's is %dx%d (a member was gated directly)", g->gate_owner,
                             sw, sh, g->gate.sw, g->gate.sh);
                }
                check_member_call(m0, slideo_matcher_gate_reset(m0, g->gate_small.data(), g->gate.sw, g->gate.sh));
            }
            g->gate_owner = 0;
        }
        int last_r = 0;
        for (int r = 0; r < N; ++r) { int lo, hi; shard_range(n_frames, r, N, lo, hi); if (hi > lo) last_r = r; }
        if (chain) gate_chain_arm(g, last_r, checked.plan.sw, checked.plan.sh);
        for_each_member(g, [&](int r) {
            int lo, hi;
            shard_range(n_frames, r, N, lo, hi);
            if (hi <= lo) return;               // (the empty shards are the trailing ones: the chain ends at last_r)
            slideo_matcher* m = g->members[r];
            if (chain) {
                // dropped unpublished — this member threw before its last unit's state was handed over — it releases the successor
                GateBatonGuard owed(r < last_r ? &g->gate_links[r]->baton : nullptr);
                match_frames_impl(m, hi - lo, src.from(lo), verdicts_out + lo, nullptr, true, changed_out + lo,
                                  similarity_out ? similarity_out + lo : nullptr);
                return;
            }
            if (r > 0) {
                FrameSrc halo = src.from(lo - 1);
                if (halo.yuv) halo.frame_stride = -1;           // (a single frame: no stride to check)
                gate_prime(m, halo, nullptr);
            }
            match_frames_impl(m, hi - lo, src.from(lo), verdicts_out + lo, nullptr, true, changed_out + lo,
                              similarity_out ? similarity_out + lo : nullptr);
        });
        g->gate = g->members[last_r]->gate;
        g->gate_owner = last_r;
    } catch (const slideo::Error& e) {
        group_gate_none(g);
        fail(e.code, "%s (the group's gate state is now \"none\")", e.what());
    } catch (const std::exception& e) {
        group_gate_none(g);
        fail(SLIDEO_ERR_HIP, "%s (the group's gate state is now \"none\")", e.what());
    }
    // the trace lookup counts the frames that went through the pipeline — changed and not direct (page_idx >= 0 with 0 inliers:
    // include/slideo_amd.h "Direct page look-up"): member r's are [match_lo[r], match_lo[r + 1])
    for (int r = 0; r < N; ++r) {
        int lo, hi, k = 0;
        shard_range(n_frames, r, N, lo, hi);
        for (int i = lo; i < hi; ++i) k += changed_out[i] != 0 && !(verdicts_out[i].page_idx >= 0 && verdicts_out[i].inliers == 0);
        g->match_lo[r + 1] = g->match_lo[r] + k;
    }
}

}  // namespace

#define GROUP_TRY try {
#define GROUP_CATCH(g)                                                        \
    }                                                                         \
    catch (const slideo::Error& e) { set_group_err(g, e.what()); return e.code; }   \
    catch (const std::exception& e) { set_group_err(g, e.what()); return SLIDEO_ERR_HIP; } \
    catch (...) { set_group_err(g, "unknown error"); return SLIDEO_ERR_HIP; } \
    return SLIDEO_OK;

// The one path of the group's six frame setters, as the entry point's return code.  propose: frame_settings.h propose_* on a member's
// settings.  Validated before any member is touched — the arguments, every member idle, the rules between settings on every
// member —, then every member's commit, then the group's half of what the setting ends.
template <class Propose>
int32_t group_set(slideo_group* g, Setting what, Propose propose, const uint8_t* mask = nullptr, int stride = 0) {
    if (!g) return SLIDEO_ERR_INVALID_ARG;
    GROUP_TRY
    std::vector<FrameSettings> next;
    for (slideo_matcher* m : g->members) next.push_back(propose(m->fs));
    for (slideo_matcher* m : g->members) require_idle(m);
    for (size_t r = 0; r < next.size(); ++r) frame_settings_rules(next[r], what, g->members[r]->sift_on);
    for (size_t r = 0; r < next.size(); ++r) settings_commit(g->members[r], what, next[r], mask, stride);
    if (SETTING_ENDS[what].kept) g->kept_valid = false;
    if (SETTING_ENDS[what].gate) group_gate_none(g);
    GROUP_CATCH(g)
}

extern "C" {

int32_t slideo_device_list(int32_t* ordinals_out, int32_t capacity) {
    int ndev = 0, n = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess) { (void)hipGetLastError(); return 0; }
    for (int d = 0; d < ndev; ++d) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, d) == hipSuccess && std::string(prop.gcnArchName).find("gfx950") != std::string::npos) {
            if (ordinals_out && n < capacity) ordinals_out[n] = d;
            ++n;
        }
    }
    return n;
}

int32_t slideo_device_count(void) { return slideo_device_list(nullptr, 0); }

int32_t slideo_group_create(const slideo_config* cfg, int32_t n_devices, const int32_t* devices, slideo_group** out) {
    slideo_group* none = nullptr;
    GROUP_TRY
    if (!cfg || !out) fail(SLIDEO_ERR_INVALID_ARG, "null cfg/out");
    *out = nullptr;
    // n_devices 0 (devices may be null): every gfx950 device of the node, by its own HIP ordinal — a device of another
    // architecture at a lower ordinal shifts nothing (the count alone would name ordinals 0 .. n-1)
    std::vector<int32_t> all;
    if (n_devices == 0) {
        all.resize(64);
        const int32_t n = slideo_device_list(all.data(), 64);
        if (n < 1) fail(SLIDEO_ERR_NO_DEVICE, "no gfx950 device visible (this library has no CPU fallback)");
        all.resize((size_t)std::min(n, 64));
        devices = all.data(); n_devices = (int32_t)all.size();
    }
    if (!devices) fail(SLIDEO_ERR_INVALID_ARG, "null devices with n_devices > 0");
    if (n_devices < 1 || n_devices > 64) fail(SLIDEO_ERR_INVALID_ARG, "n_devices must be 0 (all) or 1..64");
    std::unique_ptr<slideo_group> g(new slideo_group());
    struct Guard { slideo_group* g; ~Guard() { if (g) for (slideo_matcher* m : g->members) slideo_matcher_destroy(m); } } guard{g.get()};
    for (int i = 0; i < n_devices; ++i) {
        slideo_matcher* m = nullptr;
        const int32_t rc = slideo_matcher_create(cfg, devices[i], &m);
        if (rc != SLIDEO_OK) fail(rc, "member %d (device %d): %s", i, devices[i], slideo_last_error(nullptr));
        g->members.push_back(m);
    }
    for (int i = 1; i < n_devices; ++i) g->gate_links.emplace_back(new slideo_group::GateLink());
    g->tramps.resize((size_t)n_devices);
    for (auto& t : g->tramps) t.g = g.get();
    guard.g = nullptr;
    *out = g.release();
    GROUP_CATCH(none)
}

void slideo_group_destroy(slideo_group* g) {
    if (!g) return;
    for (slideo_matcher* m : g->members) slideo_matcher_destroy(m);
    delete g;
}

const char* slideo_group_last_error(const slideo_group* g) {
    if (g) return g->err.c_str();
    std::lock_guard<std::mutex> lk(g_group_err_mutex);
    static thread_local std::string copy;
    copy = g_group_create_error;
    return copy.c_str();
}

int32_t slideo_group_device_count(const slideo_group* g) { return g ? (int32_t)g->members.size() : 0; }

slideo_matcher* slideo_group_member(slideo_group* g, int32_t i) {
    return (g && i >= 0 && i < (int)g->members.size()) ? g->members[i] : nullptr;
}

int32_t slideo_group_set_progress(slideo_group* g, slideo_progress_fn fn, void* user) {
    if (!g) return SLIDEO_ERR_INVALID_ARG;
    g->progress = fn; g->progress_user = user;
    for (size_t r = 0; r < g->members.size(); ++r)
        slideo_matcher_set_progress(g->members[r], fn ? group_progress_tramp : nullptr, fn ? &g->tramps[r] : nullptr);
    return SLIDEO_OK;
}

int32_t slideo_group_use_sift(slideo_group* g, const slideo_sift_config* cfg, float ratio) {
    if (!g) return SLIDEO_ERR_INVALID_ARG;
    GROUP_TRY
    for (slideo_matcher* m : g->members) check_member_call(m, slideo_matcher_use_sift(m, cfg, ratio));
    GROUP_CATCH(g)
}

int32_t slideo_group_set_working_size(slideo_group* g, int32_t max_w, int32_t max_h) {
    return group_set(g, SET_WORKING_SIZE, [&](const FrameSettings& s) { return propose_working_size(s, max_w, max_h); });
}
int32_t slideo_group_set_frame_region(slideo_group* g, int32_t src_w, int32_t src_h, const double* M, int32_t out_w, int32_t out_h) {
    return group_set(g, SET_FRAME_REGION, [&](const FrameSettings& s) { return propose_frame_region(s, src_w, src_h, M, out_w, out_h); });
}
int32_t slideo_group_set_frame_lens(slideo_group* g, int32_t src_w, int32_t src_h, double cx, double cy, double f, double k1, double k2) {
    return group_set(g, SET_FRAME_REGION, [&](const FrameSettings& s) { return propose_frame_lens(s, src_w, src_h, cx, cy, f, k1, k2); });
}
int32_t slideo_group_set_frame_mask(slideo_group* g, const uint8_t* mask, int32_t width, int32_t height, int32_t stride_bytes) {
    return group_set(g, SET_FRAME_MASK, [&](const FrameSettings& s) { return propose_frame_mask(s, mask != nullptr, width, height, stride_bytes); }, mask,
                     stride_bytes);
}
int32_t slideo_group_set_frame_mask_scope(slideo_group* g, uint32_t scope) {
    return group_set(g, SET_FRAME_MASK_SCOPE, [&](const FrameSettings& s) { return propose_frame_mask_scope(s, scope); });
}
int32_t slideo_group_set_direct_similarity(slideo_group* g, float t) {
    return group_set(g, SET_DIRECT_SIMILARITY, [&](const FrameSettings& s) { return propose_direct_similarity(s, t); });
}
int32_t slideo_group_set_direct_scope(slideo_group* g, uint32_t scope) {
    return group_set(g, SET_DIRECT_SCOPE, [&](const FrameSettings& s) { return propose_direct_scope(s, scope); });
}

int32_t slideo_group_set_yuv_description(slideo_group* g, int32_t matrix, int32_t range, int32_t depth) {
    return group_set(g, SET_YUV_DESCRIPTION, [&](const FrameSettings& s) { return propose_yuv_description(s, matrix, range, depth); });
}
int32_t slideo_group_set_yuv_sampling(slideo_group* g, int32_t sampling) {
    return group_set(g, SET_YUV_DESCRIPTION, [&](const FrameSettings& s) { return propose_yuv_sampling(s, sampling); });
}
int32_t slideo_group_set_yuv_chroma(slideo_group* g, int32_t filter) {
    return group_set(g, SET_YUV_DESCRIPTION, [&](const FrameSettings& s) { return propose_yuv_chroma(s, filter); });
}
int32_t slideo_group_set_yuv_transfer(slideo_group* g, int32_t transfer, float white_nits) {
    return group_set(g, SET_YUV_DESCRIPTION, [&](const FrameSettings& s) { return propose_yuv_transfer(s, transfer, white_nits); });
}
int32_t slideo_group_set_pixel_format(slideo_group* g, int32_t format) {
    return group_set(g, SET_YUV_DESCRIPTION, [&](const FrameSettings& s) { return propose_pixel_format(s, format); });
}
// (a member whose levels histogram is open refuses, before any member changes)
int32_t slideo_group_set_frame_levels(slideo_group* g, const uint8_t* lut768) {
    bool open = false;
    if (g) for (const slideo_matcher* m : g->members) open |= m->levels.on;
    return group_set(g, SET_YUV_DESCRIPTION, [&](const FrameSettings& s) { return propose_frame_levels(s, lut768, open); });
}
int32_t slideo_group_set_frame_shading(slideo_group* g, int32_t aw, int32_t ah, int32_t cell, const uint16_t* gains) {
    return group_set(g, SET_YUV_DESCRIPTION, [&](const FrameSettings& s) { return propose_frame_shading(s, aw, ah, cell, gains); });
}

// (the group's own rule first: ANCHOR needs a group of one member or the gate order CHAIN, and a refused call changes no member)
int32_t slideo_group_set_gate_reference(slideo_group* g, uint32_t ref) {
    return group_set(g, SET_GATE_REFERENCE, [&](const FrameSettings& s) {
        gate_reference_group_rule((int)g->members.size(), ref, g->gate_order);
        return propose_gate_reference(s, ref);
    });
}

// Group gate order (include/slideo_amd.h "Group gate order"): the group's own value, beside the members' frame settings.  Validated
// before anything changes: the value, every member idle, the rule against the members' gate reference and settle.
int32_t slideo_group_set_gate_order(slideo_group* g, uint32_t order) {
    if (!g) return SLIDEO_ERR_INVALID_ARG;
    GROUP_TRY
    const uint32_t next = propose_group_gate_order(order);
    for (slideo_matcher* m : g->members) require_idle(m);
    const FrameSettings& fs = g->members[0]->fs;        // (the group's setters keep every member's alike)
    group_gate_order_rule((int)g->members.size(), next, fs.gate_ref, fs.settle_similarity);
    g->gate_order = next;
    group_gate_none(g);
    GROUP_CATCH(g)
}

int32_t slideo_group_gate_order(const slideo_group* g, uint32_t* order) {
    if (!g || !order) return SLIDEO_ERR_INVALID_ARG;
    *order = g->gate_order;
    return SLIDEO_OK;
}

// (the gate settle is part of the gate-reference setting; behind the range check the group's own rule: settle on needs a group of one
// member, and a refused call changes no member)
int32_t slideo_group_set_gate_settle(slideo_group* g, float settle_similarity, int32_t max_defer) {
    return group_set(g, SET_GATE_REFERENCE, [&](const FrameSettings& s) {
        const FrameSettings next = propose_gate_settle(s, settle_similarity, max_defer);
        gate_settle_group_rule((int)g->members.size(), settle_similarity, g->gate_order);
        return next;
    });
}

// (the gate memory is part of the gate-reference setting; behind the range check the group's own rule: a memory that is on needs a
// group of one member, and a refused call changes no member)
int32_t slideo_group_set_gate_memory(slideo_group* g, int32_t capacity) {
    return group_set(g, SET_GATE_REFERENCE, [&](const FrameSettings& s) {
        const FrameSettings next = propose_gate_memory(s, capacity);
        gate_memory_group_rule((int)g->members.size(), capacity);
        return next;
    });
}

// a group of one member forwards; with more members no memory can be on
int32_t slideo_group_last_gate_refs(slideo_group* g, int64_t* refs_out, int64_t capacity, int64_t* n) {
    if (!g) return SLIDEO_ERR_INVALID_ARG;
    GROUP_TRY
    if (!n) fail(SLIDEO_ERR_INVALID_ARG, "null n");
    *n = 0;
    slideo_matcher* m0 = g->members[0];
    if (g->members.size() > 1 || m0->fs.gate_memory == 0) fail(SLIDEO_ERR_STATE, "last_gate_refs: no gate memory is on (slideo_group_set_gate_memory)");
    const int32_t rc = slideo_matcher_last_gate_refs(m0, refs_out, capacity, n);
    if (rc != SLIDEO_OK) fail(rc, "%s", slideo_last_error(m0));
    GROUP_CATCH(g)
}

// Page sets: every member builds the same set from the same deck (ids are handed out in the same order: they agree)
int32_t slideo_group_create_page_set(slideo_group* g, int32_t n_pages, const int32_t* pages, int32_t* set_out) {
    if (!g) return SLIDEO_ERR_INVALID_ARG;
    GROUP_TRY
    if (!set_out) fail(SLIDEO_ERR_INVALID_ARG, "null set_out");
    std::vector<int32_t> ids;
    try {
        for (slideo_matcher* m : g->members) {
            int32_t id = 0;
            check_member_call(m, slideo_matcher_create_page_set(m, n_pages, pages, &id));
            ids.push_back(id);
            if (id != ids[0]) fail(SLIDEO_ERR_STATE, "members handed out page set ids %d and %d (sets made on a member directly)", ids[0], id);
        }
    } catch (...) {
        for (size_t r = 0; r < ids.size(); ++r) (void)slideo_matcher_release_page_set(g->members[r], ids[r]);
        throw;
    }
    *set_out = ids[0];
    GROUP_CATCH(g)
}

int32_t slideo_group_use_page_set(slideo_group* g, int32_t set) {
    if (!g) return SLIDEO_ERR_INVALID_ARG;
    GROUP_TRY
    for (slideo_matcher* m : g->members) check_member_call(m, slideo_matcher_use_page_set(m, set));
    GROUP_CATCH(g)
}

int32_t slideo_group_release_page_set(slideo_group* g, int32_t set) {
    if (!g) return SLIDEO_ERR_INVALID_ARG;
    GROUP_TRY
    for (slideo_matcher* m : g->members) check_member_call(m, slideo_matcher_release_page_set(m, set));
    GROUP_CATCH(g)
}

int32_t slideo_group_add_pages_bgr8(slideo_group* g, int32_t n_pages, const uint8_t* const* data, const int32_t* width,
                                    const int32_t* height, const int32_t* stride_bytes) {
    if (!g) return SLIDEO_ERR_INVALID_ARG;
    GROUP_TRY
    if (n_pages < 0 || (n_pages > 0 && (!data || !width || !height || !stride_bytes))) fail(SLIDEO_ERR_INVALID_ARG, "null page arrays");
    for (slideo_matcher* m : g->members) if (m->finalized) fail(SLIDEO_ERR_STATE, "pages cannot be added after finalize");
    const int N = (int)g->members.size();
    const uint64_t total = (uint64_t)n_pages;
    begin_progress(g, total, nullptr);
    if (g->progress) g->progress(g->progress_user, 0, total, "Analyzing PDF pages...");              // lib.rs:43
    // every member analyses its contiguous share of the call's pages (lib.rs:45-47: independent per page) ...
    std::vector<std::vector<HostPage>> got((size_t)N);
    for_each_member(g, [&](int r) {
        int lo, hi;
        shard_range(n_pages, r, N, lo, hi);
        if (hi > lo) analyse_pages(g->members[r], hi - lo, data + lo, width + lo, height + lo, stride_bytes + lo, got[r], 0, (uint64_t)(hi - lo));
    });
    // ... and every member's database receives the whole call, in page order — each on its own thread (the records are plain
    // host data: N copies of the deck's records side by side instead of one after the other on the caller's thread)
    for_each_member(g, [&](int me) {
        for (int r = 0; r < N; ++r)
            for (const HostPage& pg : got[r]) append_page(g->members[me], pg);
    });
    if (g->progress) g->progress(g->progress_user, total, total, "PDF page analysis successful.");   // lib.rs:58
    GROUP_CATCH(g)
}

int32_t slideo_group_finalize_pages(slideo_group* g) {
    if (!g) return SLIDEO_ERR_INVALID_ARG;
    GROUP_TRY
    for_each_member(g, [&](int r) { check_member_call(g->members[r], slideo_matcher_finalize_pages(g->members[r])); });
    GROUP_CATCH(g)
}

int32_t slideo_group_page_count(const slideo_group* g) { return g ? slideo_matcher_page_count(g->members[0]) : -1; }
int64_t slideo_group_descriptor_count(const slideo_group* g) { return g ? slideo_matcher_descriptor_count(g->members[0]) : -1; }

int32_t slideo_group_match_frames_bgr8(slideo_group* g, int32_t n_frames, const uint8_t* frames, int32_t width, int32_t height,
                                       int32_t stride_bytes, int64_t frame_stride_bytes, slideo_verdict* verdicts_out) {
    if (!g) return SLIDEO_ERR_INVALID_ARG;
    GROUP_TRY
    group_match_impl(g, n_frames, FrameSrc::bgr8(frames, false, width, height, stride_bytes, frame_stride_bytes), verdicts_out);
    GROUP_CATCH(g)
}

int32_t slideo_group_match_frames_yuv420(slideo_group* g, int32_t n_frames, const uint8_t* frames, int32_t width, int32_t height,
                                         const slideo_yuv420_layout* layout, int64_t frame_stride_bytes, slideo_verdict* verdicts_out) {
    if (!g) return SLIDEO_ERR_INVALID_ARG;
    GROUP_TRY
    group_match_impl(g, n_frames, FrameSrc::yuv420(frames, false, width, height, layout, frame_stride_bytes), verdicts_out);
    GROUP_CATCH(g)
}

// ---- Frame lists (include/slideo_amd.h "Frame lists"): host lists; a shard is a sub-range of the array (FrameSrc::from) --------------
static FrameSrc group_list_src(slideo_group* g, const slideo_frame_list* list) {
    FrameSrc src = FrameSrc::from_list(list, g->members[0]->fs);
    if (src.on_device) fail(SLIDEO_ERR_INVALID_ARG, "frame list: the group's forms take host lists (on_device 0)");
    return src;
}

int32_t slideo_group_match_frames_list(slideo_group* g, const slideo_frame_list* list, slideo_verdict* verdicts_out) {
    if (!g) return SLIDEO_ERR_INVALID_ARG;
    GROUP_TRY
    const FrameSrc src = group_list_src(g, list);
    group_match_impl(g, list->n_frames, src, verdicts_out);
    GROUP_CATCH(g)
}

int32_t slideo_group_changed_mask_list(slideo_group* g, const slideo_frame_list* list, const uint8_t* prev_small, uint8_t* last_small_out,
                                       uint8_t* changed_out, float* similarity_out) {
    if (!g) return SLIDEO_ERR_INVALID_ARG;
    GROUP_TRY
    const FrameSrc src = group_list_src(g, list);
    group_mask_impl(g, list->n_frames, src, prev_small, last_small_out, changed_out, similarity_out);
    GROUP_CATCH(g)
}

int32_t slideo_group_match_changed_frames_list(slideo_group* g, const slideo_frame_list* list, uint8_t* changed_out, float* similarity_out,
                                               slideo_verdict* verdicts_out) {
    if (!g) return SLIDEO_ERR_INVALID_ARG;
    GROUP_TRY
    const FrameSrc src = group_list_src(g, list);
    group_gated_impl(g, list->n_frames, src, changed_out, similarity_out, verdicts_out);
    GROUP_CATCH(g)
}

int32_t slideo_group_last_frame_candidates(const slideo_group* g, int32_t frame_in_batch, slideo_candidate* out, int32_t capacity, int32_t* n_out) {
    if (!g || !n_out || g->match_lo.empty()) return SLIDEO_ERR_INVALID_ARG;
    for (size_t r = 0; r + 1 < g->match_lo.size(); ++r)
        if (frame_in_batch >= g->match_lo[r] && frame_in_batch < g->match_lo[r + 1])
            return slideo_last_frame_candidates(g->members[r], frame_in_batch - g->match_lo[r], out, capacity, n_out);
    return SLIDEO_ERR_INVALID_ARG;
}

int32_t slideo_group_changed_mask_bgr8(slideo_group* g, int32_t n_frames, const uint8_t* frames, int32_t width, int32_t height,
                                       int32_t stride_bytes, int64_t frame_stride_bytes, const uint8_t* prev_small,
                                       uint8_t* last_small_out, uint8_t* changed_out, float* similarity_out) {
    if (!g) return SLIDEO_ERR_INVALID_ARG;
    GROUP_TRY
    group_mask_impl(g, n_frames, FrameSrc::bgr8(frames, false, width, height, stride_bytes, frame_stride_bytes), prev_small, last_small_out,
                    changed_out, similarity_out);
    GROUP_CATCH(g)
}

int32_t slideo_group_changed_mask_yuv420(slideo_group* g, int32_t n_frames, const uint8_t* frames, int32_t width, int32_t height,
                                         const slideo_yuv420_layout* layout, int64_t frame_stride_bytes, const uint8_t* prev_small,
                                         uint8_t* last_small_out, uint8_t* changed_out, float* similarity_out) {
    if (!g) return SLIDEO_ERR_INVALID_ARG;
    GROUP_TRY
    group_mask_impl(g, n_frames, FrameSrc::yuv420(frames, false, width, height, layout, frame_stride_bytes), prev_small, last_small_out,
                    changed_out, similarity_out);
    GROUP_CATCH(g)
}

int32_t slideo_group_match_kept_frames(slideo_group* g, int32_t n_sel, const int32_t* sel, slideo_verdict* verdicts_out) {
    if (!g) return SLIDEO_ERR_INVALID_ARG;
    GROUP_TRY
    if (n_sel < 0 || (n_sel > 0 && (!sel || !verdicts_out))) fail(SLIDEO_ERR_INVALID_ARG, "null selection/verdicts");
    if (!g->kept_valid) fail(SLIDEO_ERR_STATE, "no frames kept: slideo_group_changed_mask_bgr8 must be the call before (its upload is what is matched)");
    const int N = (int)g->members.size();
    const int n_kept = g->kept.empty() ? 0 : g->kept.back().hi;
    // a selected frame is matched by the member whose block holds it, from the copy the mask call left on that device
    std::vector<std::vector<int32_t>> local((size_t)N), where((size_t)N);
    for (int i = 0; i < n_sel; ++i) {
        if (sel[i] < 0 || sel[i] >= n_kept) fail(SLIDEO_ERR_INVALID_ARG, "selected frame %d outside the %d kept", sel[i], n_kept);
        for (int r = 0; r < N; ++r)
            if (sel[i] >= g->kept[r].lo && sel[i] < g->kept[r].hi) { local[r].push_back(sel[i] - g->kept[r].read_lo); where[r].push_back(i); break; }
    }
    begin_progress(g, (uint64_t)n_sel, nullptr);
    g->match_lo.clear();
    for_each_member(g, [&](int r) {
        if (local[r].empty()) return;
        std::vector<slideo_verdict> v(local[r].size());
        check_member_call(g->members[r], slideo_match_kept_frames(g->members[r], (int32_t)local[r].size(), local[r].data(), v.data()));
        for (size_t j = 0; j < v.size(); ++j) verdicts_out[where[r][j]] = v[j];
    });
    GROUP_CATCH(g)
}

int32_t slideo_group_gate_reset(slideo_group* g, const uint8_t* prev_small, int32_t small_w, int32_t small_h) {
    if (!g) return SLIDEO_ERR_INVALID_ARG;
    GROUP_TRY
    const int small_area = g->members[0]->cfg.small_area;
    if (prev_small && (small_w < 1 || small_h < 1 || (int64_t)small_w * small_h > small_area))
        fail(SLIDEO_ERR_INVALID_ARG, "gate_reset: a %dx%d small image (at most small_area = %d pixels)", small_w, small_h, small_area);
    for (slideo_matcher* m : g->members) require_idle(m);
    group_gate_none(g);
    if (!prev_small) return SLIDEO_OK;
    g->gate_small.assign(prev_small, prev_small + (size_t)small_w * small_h * 3);
    g->gate.has = true; g->gate.sw = small_w; g->gate.sh = small_h;
    GROUP_CATCH(g)
}

int32_t slideo_group_gate_last_small(slideo_group* g, uint8_t* out, int64_t out_capacity, int32_t* sw, int32_t* sh) {
    if (!g) return SLIDEO_ERR_INVALID_ARG;
    GROUP_TRY
    if (!sw || !sh) fail(SLIDEO_ERR_INVALID_ARG, "null sw/sh");
    for (slideo_matcher* m : g->members) require_idle(m);
    if (!g->gate.has) fail(SLIDEO_ERR_STATE, "the gate state is \"none\": no frame was gated since the last reset");
    if (g->gate_owner >= 0) {
        slideo_matcher* o = g->members[g->gate_owner];
        check_member_call(o, slideo_matcher_gate_last_small(o, out, out_capacity, sw, sh));
        return SLIDEO_OK;
    }
    *sw = g->gate.sw; *sh = g->gate.sh;
    if ((int64_t)g->gate_small.size() > out_capacity) fail(SLIDEO_ERR_CAPACITY, "small image needs %lld bytes", (long long)g->gate_small.size());
    if (out) std::memcpy(out, g->gate_small.data(), g->gate_small.size());
    GROUP_CATCH(g)
}

int32_t slideo_group_gate_chain_waited(const slideo_group* g, int32_t member, double* seconds) {
    if (!g || !seconds || member < 1 || member >= (int)g->members.size()) return SLIDEO_ERR_INVALID_ARG;
    *seconds = g->gate_links[(size_t)member - 1]->waited_s;
    return SLIDEO_OK;
}

// The group's one state as a record: its owner's, or — a reset's small image — what a single matcher exports after that reset
int32_t slideo_group_gate_state_export(slideo_group* g, uint8_t* out, int64_t capacity, int64_t* bytes) {
    if (!g) return SLIDEO_ERR_INVALID_ARG;
    GROUP_TRY
    if (!bytes) fail(SLIDEO_ERR_INVALID_ARG, "null bytes");
    gate_record_memory_rule(g->members[0]->fs.gate_memory);
    for (slideo_matcher* m : g->members) require_idle(m);
    if (g->gate.has && g->gate_owner >= 0) {
        slideo_matcher* o = g->members[g->gate_owner];
        check_member_call(o, slideo_matcher_gate_state_export(o, out, capacity, bytes));
        return SLIDEO_OK;
    }
    const FrameSettings& fs = g->members[0]->fs;
    GateRecordHead h;
    h.has = g->gate.has; h.gate_ref = fs.gate_ref; h.settle = fs.settle_similarity > 0.f;
    if (h.has) { h.sw = g->gate.sw; h.sh = g->gate.sh; }
    *bytes = h.bytes();
    if (!out || h.bytes() > capacity) fail(SLIDEO_ERR_CAPACITY, "the gate state record needs %lld bytes", (long long)h.bytes());
    gate_record_encode(h, out);
    if (h.has) {
        std::memcpy(out + GATE_RECORD_HEADER, g->gate_small.data(), g->gate_small.size());
        if (h.settle) std::memcpy(out + GATE_RECORD_HEADER + g->gate_small.size(), g->gate_small.data(), g->gate_small.size());
    }
    GROUP_CATCH(g)
}

// ... and back: into member 0, where the next gated call's first frame is compared (a refused record leaves the group's state)
int32_t slideo_group_gate_state_import(slideo_group* g, const uint8_t* rec, int64_t bytes) {
    if (!g) return SLIDEO_ERR_INVALID_ARG;
    GROUP_TRY
    slideo_matcher* m0 = g->members[0];
    gate_record_memory_rule(m0->fs.gate_memory);
    (void)gate_record_validate(rec, bytes, m0->fs.gate_ref, m0->fs.settle_similarity, m0->fs.settle_max_defer, m0->cfg.small_area);
    for (slideo_matcher* m : g->members) require_idle(m);
    check_member_call(m0, slideo_matcher_gate_state_import(m0, rec, bytes));
    group_gate_none(g);
    g->gate = m0->gate;
    g->gate_owner = 0;
    GROUP_CATCH(g)
}

int32_t slideo_group_match_changed_frames_bgr8(slideo_group* g, int32_t n_frames, const uint8_t* frames, int32_t width, int32_t height,
                                               int32_t stride_bytes, int64_t frame_stride_bytes, uint8_t* changed_out, float* similarity_out,
                                               slideo_verdict* verdicts_out) {
    if (!g) return SLIDEO_ERR_INVALID_ARG;
    GROUP_TRY
    group_gated_impl(g, n_frames, FrameSrc::bgr8(frames, false, width, height, stride_bytes, frame_stride_bytes), changed_out, similarity_out,
                     verdicts_out);
    GROUP_CATCH(g)
}

int32_t slideo_group_match_changed_frames_yuv420(slideo_group* g, int32_t n_frames, const uint8_t* frames, int32_t width, int32_t height,
                                                 const slideo_yuv420_layout* layout, int64_t frame_stride_bytes, uint8_t* changed_out,
                                                 float* similarity_out, slideo_verdict* verdicts_out) {
    if (!g) return SLIDEO_ERR_INVALID_ARG;
    GROUP_TRY
    group_gated_impl(g, n_frames, FrameSrc::yuv420(frames, false, width, height, layout, frame_stride_bytes), changed_out, similarity_out,
                     verdicts_out);
    GROUP_CATCH(g)
}

// ---- Match evidence map (include/slideo_amd.h "Match evidence map"): every member carries a session, the read-outs return the sums --
int32_t slideo_group_evidence_begin(slideo_group* g, int32_t cell, int32_t min_inliers) {
    if (!g) return SLIDEO_ERR_INVALID_ARG;
    GROUP_TRY
    if (cell != 16 && cell != 32 && cell != 64) fail(SLIDEO_ERR_INVALID_ARG, "evidence_begin: cell %d is none of 16, 32, 64", cell);
    if (min_inliers < 0) fail(SLIDEO_ERR_INVALID_ARG, "evidence_begin: min_inliers %d below 0", min_inliers);
    // validated before any member is touched
    for (slideo_matcher* m : g->members) {
        if (m->sift_on) fail(SLIDEO_ERR_UNSUPPORTED, "evidence_begin: the evidence map is not defined in SIFT mode");
        require_idle(m);
        if (m->evidence.on) fail(SLIDEO_ERR_STATE, "evidence_begin: a session is open (slideo_group_evidence_end first)");
    }
    for (slideo_matcher* m : g->members) check_member_call(m, slideo_matcher_evidence_begin(m, cell, min_inliers));
    GROUP_CATCH(g)
}

int32_t slideo_group_evidence_end(slideo_group* g) {
    if (!g) return SLIDEO_ERR_INVALID_ARG;
    GROUP_TRY
    for (slideo_matcher* m : g->members) require_idle(m);
    for (slideo_matcher* m : g->members) check_member_call(m, slideo_matcher_evidence_end(m));
    GROUP_CATCH(g)
}

namespace {
// the members' sessions as one: every member's open, the members that counted agree on the analysed size
void group_evidence(slideo_group* g, slideo_matcher::Evidence& sum) {
    sum = slideo_matcher::Evidence{};
    for (slideo_matcher* m : g->members) {
        const slideo_matcher::Evidence& E = m->evidence;
        if (!E.on) fail(SLIDEO_ERR_STATE, "no evidence session on every member: slideo_group_evidence_begin first");
        if (!sum.on) { sum = E; sum.aw = sum.ah = sum.gw = sum.gh = 0; sum.through = sum.counted = 0; }
        if (E.cell != sum.cell || E.min_inliers != sum.min_inliers) fail(SLIDEO_ERR_STATE, "the members' evidence sessions differ (one was begun directly)");
        if (E.aw > 0) {
            if (sum.aw > 0 && (sum.aw != E.aw || sum.ah != E.ah))
                fail(SLIDEO_ERR_STATE, "the members' evidence sessions count at %dx%d and %dx%d (a member was called directly)", sum.aw, sum.ah, E.aw, E.ah);
            sum.aw = E.aw; sum.ah = E.ah; sum.gw = E.gw; sum.gh = E.gh;
        }
        sum.through += E.through; sum.counted += E.counted;
    }
}
}  // namespace

int32_t slideo_group_evidence_info(slideo_group* g, int32_t* cell, int32_t* min_inliers, int32_t* aw, int32_t* ah, int32_t* gw, int32_t* gh,
                                   int64_t* frames_through, int64_t* frames_counted) {
    if (!g) return SLIDEO_ERR_INVALID_ARG;
    GROUP_TRY
    if (!cell || !min_inliers || !aw || !ah || !gw || !gh || !frames_through || !frames_counted) fail(SLIDEO_ERR_INVALID_ARG, "null output");
    slideo_matcher::Evidence E;
    group_evidence(g, E);
    *cell = E.cell; *min_inliers = E.min_inliers; *aw = E.aw; *ah = E.ah; *gw = E.gw; *gh = E.gh;
    *frames_through = E.through; *frames_counted = E.counted;
    GROUP_CATCH(g)
}

int32_t slideo_group_evidence_counts(slideo_group* g, uint32_t* seen_out, uint32_t* hit_out, int64_t capacity_elems, int32_t* gw, int32_t* gh,
                                     int64_t* frames_through, int64_t* frames_counted) {
    if (!g) return SLIDEO_ERR_INVALID_ARG;
    GROUP_TRY
    if (!gw || !gh || !frames_through || !frames_counted) fail(SLIDEO_ERR_INVALID_ARG, "null gw/gh/frames_through/frames_counted");
    for (slideo_matcher* m : g->members) require_idle(m);
    slideo_matcher::Evidence E;
    group_evidence(g, E);
    *gw = E.gw; *gh = E.gh; *frames_through = E.through; *frames_counted = E.counted;
    if (E.aw == 0 || (!seen_out && !hit_out)) return SLIDEO_OK;
    if (!seen_out || !hit_out) fail(SLIDEO_ERR_INVALID_ARG, "seen_out and hit_out go together");
    const int64_t nc = (int64_t)E.gw * E.gh;
    if (nc > capacity_elems) fail(SLIDEO_ERR_CAPACITY, "the counts need %lld elements each", (long long)nc);
    std::vector<uint32_t> part((size_t)nc * 2);
    std::fill(seen_out, seen_out + nc, 0u);
    std::fill(hit_out, hit_out + nc, 0u);
    for (slideo_matcher* m : g->members) {
        if (m->evidence.aw == 0) continue;               // (its shards were empty: nothing counted)
        int32_t w = 0, h = 0; int64_t t = 0, c = 0;
        check_member_call(m, slideo_matcher_evidence_counts(m, part.data(), part.data() + nc, nc, &w, &h, &t, &c));
        for (int64_t i = 0; i < nc; ++i) {
            // (the frames limit holds per member: a sum over members can pass u32, which is refused, never wrapped)
            if (seen_out[i] > 0xFFFFFFFFu - part[(size_t)i]) fail(SLIDEO_ERR_CAPACITY, "a summed counter passes UINT32_MAX: read the members' counts one by one");
            seen_out[i] += part[(size_t)i]; hit_out[i] += part[(size_t)(nc + i)];
        }
    }
    GROUP_CATCH(g)
}

// ---- Match tone table (include/slideo_amd.h "Match tone table"): every member carries a session, the read-outs return the sums -------
int32_t slideo_group_tone_begin(slideo_group* g, int32_t min_inliers, int32_t min_hits, int32_t flat) {
    if (!g) return SLIDEO_ERR_INVALID_ARG;
    GROUP_TRY
    if (min_inliers < 0) fail(SLIDEO_ERR_INVALID_ARG, "tone_begin: min_inliers %d below 0", min_inliers);
    if (min_hits < 1) fail(SLIDEO_ERR_INVALID_ARG, "tone_begin: min_hits %d below 1", min_hits);
    if (flat < 0 || flat > 255) fail(SLIDEO_ERR_INVALID_ARG, "tone_begin: flat %d outside 0..255", flat);
    // validated before any member is touched
    for (slideo_matcher* m : g->members) {
        if (m->sift_on) fail(SLIDEO_ERR_UNSUPPORTED, "tone_begin: the tone table is not defined in SIFT mode");
        require_idle(m);
        if (m->tone.on) fail(SLIDEO_ERR_STATE, "tone_begin: a session is open (slideo_group_tone_end first)");
    }
    for (slideo_matcher* m : g->members) check_member_call(m, slideo_matcher_tone_begin(m, min_inliers, min_hits, flat));
    GROUP_CATCH(g)
}

int32_t slideo_group_tone_end(slideo_group* g) {
    if (!g) return SLIDEO_ERR_INVALID_ARG;
    GROUP_TRY
    for (slideo_matcher* m : g->members) require_idle(m);
    for (slideo_matcher* m : g->members) check_member_call(m, slideo_matcher_tone_end(m));
    GROUP_CATCH(g)
}

namespace {
// the members' sessions as one: every member's open and of the same settings; `through` summed
void group_tone(slideo_group* g, slideo_matcher::Tone& sum) {
    sum = slideo_matcher::Tone{};
    for (slideo_matcher* m : g->members) {
        const slideo_matcher::Tone& T = m->tone;
        if (!T.on) fail(SLIDEO_ERR_STATE, "no tone session on every member: slideo_group_tone_begin first");
        if (!sum.on) { sum = T; sum.through = 0; }
        if (T.min_inliers != sum.min_inliers || T.min_hits != sum.min_hits || T.flat != sum.flat)
            fail(SLIDEO_ERR_STATE, "the members' tone sessions differ (one was begun directly)");
        sum.through += T.through;
    }
}
}  // namespace

int32_t slideo_group_tone_info(slideo_group* g, int32_t* min_inliers, int32_t* min_hits, int32_t* flat, int64_t* frames_through) {
    if (!g) return SLIDEO_ERR_INVALID_ARG;
    GROUP_TRY
    if (!min_inliers || !min_hits || !flat || !frames_through) fail(SLIDEO_ERR_INVALID_ARG, "null output");
    slideo_matcher::Tone T;
    group_tone(g, T);
    *min_inliers = T.min_inliers; *min_hits = T.min_hits; *flat = T.flat; *frames_through = T.through;
    GROUP_CATCH(g)
}

int32_t slideo_group_tone_counts(slideo_group* g, uint64_t* cnt_out, uint64_t* sum_out, int64_t* frames_through, int64_t* frames_counted) {
    if (!g) return SLIDEO_ERR_INVALID_ARG;
    GROUP_TRY
    if (!cnt_out || !sum_out || !frames_through || !frames_counted) fail(SLIDEO_ERR_INVALID_ARG, "null cnt_out/sum_out/frames_through/frames_counted");
    for (slideo_matcher* m : g->members) require_idle(m);
    slideo_matcher::Tone T;
    group_tone(g, T);
    // (every member holds fewer than 2^31 frames of fewer than 2^24 samples of at most 255: the members' sums stay inside u64)
    std::vector<uint64_t> part(1536), cnt(768, 0), sum(768, 0);
    int64_t counted = 0;
    for (slideo_matcher* m : g->members) {
        int64_t t = 0, c = 0;
        check_member_call(m, slideo_matcher_tone_counts(m, part.data(), part.data() + 768, &t, &c));
        for (int i = 0; i < 768; ++i) { cnt[(size_t)i] += part[(size_t)i]; sum[(size_t)i] += part[(size_t)(768 + i)]; }
        counted += c;
    }
    std::copy(cnt.begin(), cnt.end(), cnt_out);
    std::copy(sum.begin(), sum.end(), sum_out);
    *frames_through = T.through; *frames_counted = counted;
    GROUP_CATCH(g)
}

// ---- Match placement map (include/slideo_amd.h "Match placement map"): every member carries a session, the read-outs return the sums --
int32_t slideo_group_placement_begin(slideo_group* g, int32_t cell, int32_t min_inliers, double reach) {
    if (!g) return SLIDEO_ERR_INVALID_ARG;
    GROUP_TRY
    if (cell != 16 && cell != 32 && cell != 64) fail(SLIDEO_ERR_INVALID_ARG, "placement_begin: cell %d is none of 16, 32, 64", cell);
    if (min_inliers < 0) fail(SLIDEO_ERR_INVALID_ARG, "placement_begin: min_inliers %d below 0", min_inliers);
    if (!(reach > 0.0) || !std::isfinite(reach * reach)) fail(SLIDEO_ERR_INVALID_ARG, "placement_begin: reach %g is not a finite distance above 0", reach);
    // validated before any member is touched
    for (slideo_matcher* m : g->members) {
        if (m->sift_on) fail(SLIDEO_ERR_UNSUPPORTED, "placement_begin: the placement map is not defined in SIFT mode");
        require_idle(m);
        if (m->placement.on) fail(SLIDEO_ERR_STATE, "placement_begin: a session is open (slideo_group_placement_end first)");
    }
    for (slideo_matcher* m : g->members) check_member_call(m, slideo_matcher_placement_begin(m, cell, min_inliers, reach));
    GROUP_CATCH(g)
}

int32_t slideo_group_placement_end(slideo_group* g) {
    if (!g) return SLIDEO_ERR_INVALID_ARG;
    GROUP_TRY
    for (slideo_matcher* m : g->members) require_idle(m);
    for (slideo_matcher* m : g->members) check_member_call(m, slideo_matcher_placement_end(m));
    GROUP_CATCH(g)
}

namespace {
// the members' sessions as one: every member's open, the members that counted agree on the analysed size
void group_placement(slideo_group* g, slideo_matcher::Placement& sum) {
    sum = slideo_matcher::Placement{};
    for (slideo_matcher* m : g->members) {
        const slideo_matcher::Placement& P = m->placement;
        if (!P.on) fail(SLIDEO_ERR_STATE, "no placement session on every member: slideo_group_placement_begin first");
        if (!sum.on) { sum = P; sum.aw = sum.ah = sum.gw = sum.gh = 0; sum.through = 0; }
        if (P.cell != sum.cell || P.min_inliers != sum.min_inliers || P.reach != sum.reach)
            fail(SLIDEO_ERR_STATE, "the members' placement sessions differ (one was begun directly)");
        if (P.aw > 0) {
            if (sum.aw > 0 && (sum.aw != P.aw || sum.ah != P.ah))
                fail(SLIDEO_ERR_STATE, "the members' placement sessions count at %dx%d and %dx%d (a member was called directly)", sum.aw, sum.ah, P.aw, P.ah);
            sum.aw = P.aw; sum.ah = P.ah; sum.gw = P.gw; sum.gh = P.gh;
        }
        sum.through += P.through;
    }
}
}  // namespace

int32_t slideo_group_placement_info(slideo_group* g, int32_t* cell, int32_t* min_inliers, double* reach, int32_t* aw, int32_t* ah, int32_t* gw, int32_t* gh,
                                    int64_t* frames_through) {
    if (!g) return SLIDEO_ERR_INVALID_ARG;
    GROUP_TRY
    if (!cell || !min_inliers || !reach || !aw || !ah || !gw || !gh || !frames_through) fail(SLIDEO_ERR_INVALID_ARG, "null output");
    slideo_matcher::Placement P;
    group_placement(g, P);
    *cell = P.cell; *min_inliers = P.min_inliers; *reach = P.reach; *aw = P.aw; *ah = P.ah; *gw = P.gw; *gh = P.gh; *frames_through = P.through;
    GROUP_CATCH(g)
}

int32_t slideo_group_placement_sums(slideo_group* g, uint64_t* n_out, uint64_t* sfx_out, uint64_t* sfy_out, uint64_t* su_out, uint64_t* sv_out,
                                    int64_t capacity_elems, int32_t* gw, int32_t* gh, int64_t* frames_through, int64_t* frames_counted) {
    if (!g) return SLIDEO_ERR_INVALID_ARG;
    GROUP_TRY
    if (!gw || !gh || !frames_through || !frames_counted) fail(SLIDEO_ERR_INVALID_ARG, "null gw/gh/frames_through/frames_counted");
    for (slideo_matcher* m : g->members) require_idle(m);
    slideo_matcher::Placement P;
    group_placement(g, P);
    *gw = P.gw; *gh = P.gh; *frames_through = P.through; *frames_counted = 0;
    if (P.aw == 0) return SLIDEO_OK;
    uint64_t* outs[5] = {n_out, sfx_out, sfy_out, su_out, sv_out};
    int given = 0;
    for (uint64_t* o : outs) given += o != nullptr;
    if (given != 0 && given != 5) fail(SLIDEO_ERR_INVALID_ARG, "the five output arrays go together");
    const int64_t nc = (int64_t)P.gw * P.gh;
    if (given && nc > capacity_elems) fail(SLIDEO_ERR_CAPACITY, "the sums need %lld elements each", (long long)nc);
    // (every member's sums stay below 2^52: the members' sums stay inside u64)
    std::vector<uint64_t> part(given ? (size_t)nc * 5 : 0);
    for (int i = 0; given && i < 5; ++i) std::fill(outs[i], outs[i] + nc, (uint64_t)0);
    int64_t counted = 0;
    for (slideo_matcher* m : g->members) {
        if (m->placement.aw == 0) continue;              // (its shards were empty: nothing counted)
        int32_t w = 0, h = 0; int64_t t = 0, c = 0;
        uint64_t* p = given ? part.data() : nullptr;
        check_member_call(m, slideo_matcher_placement_sums(m, p, p ? p + nc : p, p ? p + 2 * nc : p, p ? p + 3 * nc : p, p ? p + 4 * nc : p, nc, &w, &h, &t, &c));
        for (int i = 0; given && i < 5; ++i)
            for (int64_t j = 0; j < nc; ++j) outs[i][j] += part[(size_t)(i * nc + j)];
        counted += c;
    }
    *frames_counted = counted;
    GROUP_CATCH(g)
}

// ---- Match shading map (include/slideo_amd.h "Match shading map"): every member carries a session, the read-outs return the sums ------
int32_t slideo_group_shading_begin(slideo_group* g, int32_t cell, int32_t min_inliers, int32_t min_hits, int32_t flat) {
    if (!g) return SLIDEO_ERR_INVALID_ARG;
    GROUP_TRY
    // validated on every member before one is touched: the matcher's own rules
    for (slideo_matcher* m : g->members) shading_map_begin_check(m, cell, min_inliers, min_hits, flat);
    for (slideo_matcher* m : g->members) check_member_call(m, slideo_matcher_shading_begin(m, cell, min_inliers, min_hits, flat));
    GROUP_CATCH(g)
}

int32_t slideo_group_shading_end(slideo_group* g) {
    if (!g) return SLIDEO_ERR_INVALID_ARG;
    GROUP_TRY
    for (slideo_matcher* m : g->members) require_idle(m);
    for (slideo_matcher* m : g->members) check_member_call(m, slideo_matcher_shading_end(m));
    GROUP_CATCH(g)
}

namespace {
// the members' sessions as one: every member's open, the members that counted agree on the analysed size
void group_shading_map(slideo_group* g, slideo_matcher::ShadingMap& sum) {
    sum = slideo_matcher::ShadingMap{};
    for (slideo_matcher* m : g->members) {
        const slideo_matcher::ShadingMap& H = m->shading_map;
        if (!H.on) fail(SLIDEO_ERR_STATE, "no shading session on every member: slideo_group_shading_begin first");
        if (!sum.on) { sum = H; sum.aw = sum.ah = sum.gw = sum.gh = 0; sum.through = 0; }
        if (H.cell != sum.cell || H.min_inliers != sum.min_inliers || H.min_hits != sum.min_hits || H.flat != sum.flat)
            fail(SLIDEO_ERR_STATE, "the members' shading sessions differ (one was begun directly)");
        if (H.aw > 0) {
            if (sum.aw > 0 && (sum.aw != H.aw || sum.ah != H.ah))
                fail(SLIDEO_ERR_STATE, "the members' shading sessions count at %dx%d and %dx%d (a member was called directly)", sum.aw, sum.ah, H.aw, H.ah);
            sum.aw = H.aw; sum.ah = H.ah; sum.gw = H.gw; sum.gh = H.gh;
        }
        sum.through += H.through;
    }
}
}  // namespace

int32_t slideo_group_shading_info(slideo_group* g, int32_t* cell, int32_t* min_inliers, int32_t* min_hits, int32_t* flat, int32_t* aw, int32_t* ah,
                                  int32_t* gw, int32_t* gh, int64_t* frames_through) {
    if (!g) return SLIDEO_ERR_INVALID_ARG;
    GROUP_TRY
    if (!cell || !min_inliers || !min_hits || !flat || !aw || !ah || !gw || !gh || !frames_through) fail(SLIDEO_ERR_INVALID_ARG, "null output");
    slideo_matcher::ShadingMap H;
    group_shading_map(g, H);
    *cell = H.cell; *min_inliers = H.min_inliers; *min_hits = H.min_hits; *flat = H.flat; *aw = H.aw; *ah = H.ah; *gw = H.gw; *gh = H.gh;
    *frames_through = H.through;
    GROUP_CATCH(g)
}

int32_t slideo_group_shading_sums(slideo_group* g, uint64_t* cnt_out, uint64_t* sum_f_out, uint64_t* sum_p_out, int64_t capacity_elems, int32_t* gw,
                                  int32_t* gh, int64_t* frames_through, int64_t* frames_counted) {
    if (!g) return SLIDEO_ERR_INVALID_ARG;
    GROUP_TRY
    if (!gw || !gh || !frames_through || !frames_counted) fail(SLIDEO_ERR_INVALID_ARG, "null gw/gh/frames_through/frames_counted");
    for (slideo_matcher* m : g->members) require_idle(m);
    slideo_matcher::ShadingMap H;
    group_shading_map(g, H);
    *gw = H.gw; *gh = H.gh; *frames_through = H.through; *frames_counted = 0;
    if (H.aw == 0) return SLIDEO_OK;
    uint64_t* outs[3] = {cnt_out, sum_f_out, sum_p_out};
    int given = 0;
    for (uint64_t* o : outs) given += o != nullptr;
    if (given != 0 && given != 3) fail(SLIDEO_ERR_INVALID_ARG, "the three output arrays go together");
    const int64_t nc = (int64_t)H.gw * H.gh;
    if (given && nc > capacity_elems) fail(SLIDEO_ERR_CAPACITY, "the sums need %lld elements each", (long long)nc);
    // (a member's sums stay below 765 * 2^24 * 2^20 < 2^54: the members' sums stay inside u64)
    std::vector<uint64_t> part(given ? (size_t)nc * 3 : 0);
    for (int i = 0; given && i < 3; ++i) std::fill(outs[i], outs[i] + nc, (uint64_t)0);
    int64_t counted = 0;
    for (slideo_matcher* m : g->members) {
        if (m->shading_map.aw == 0) continue;            // (its shards were empty: nothing counted)
        int32_t w = 0, h = 0; int64_t t = 0, c = 0;
        uint64_t* p = given ? part.data() : nullptr;
        check_member_call(m, slideo_matcher_shading_sums(m, p, p ? p + nc : p, p ? p + 2 * nc : p, nc, &w, &h, &t, &c));
        for (int i = 0; given && i < 3; ++i)
            for (int64_t j = 0; j < nc; ++j) outs[i][j] += part[(size_t)(i * nc + j)];
        counted += c;
    }
    *frames_counted = counted;
    GROUP_CATCH(g)
}

}  // extern "C"
