// group_gate_chain_hostcheck — the host side of the group gate order (include/slideo_amd.h "Group gate order", "Gate state record";
// csrc/frame_settings.h, csrc/gate_baton.h) on its own: the rule table of the three set calls that can complete the refused
// combination, the record header's encode / validate round trip with every refusal, and the baton with real threads.  No GPU,
// nothing loaded into Python.
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -I include -I slideo_amd/csrc tools/group_gate_chain_hostcheck.cpp -o hostcheck && ./hostcheck
//   (the baton part is what -fsanitize=thread is for:  ./hostcheck baton)
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <thread>
#include <vector>

#include "frame_settings.h"
#include "gate_baton.h"

using namespace slideo;

namespace {

int fails = 0;
void expect(bool ok, const char* what) {
    if (ok) return;
    ++fails;
    std::fprintf(stderr, "FAIL %s\n", what);
}

template <class F>
int code_of(F f) {
    try { f(); } catch (const Error& e) { return e.code; }
    return 0;
}

// ---- the rule table -------------------------------------------------------------------------------------------------------------------
// A group as capi_group.hip keeps it: the order is the group's, reference and settle are the members' frame settings (alike on all).
struct G {
    int members = 1;
    uint32_t order = SLIDEO_GROUP_GATE_HALO;
    FrameSettings fs;
    // slideo_group_set_gate_order / _set_gate_reference / _set_gate_settle: nothing changes unless every check passed
    int set_order(uint32_t o) {
        return code_of([&] {
            const uint32_t next = propose_group_gate_order(o);
            group_gate_order_rule(members, next, fs.gate_ref, fs.settle_similarity);
            order = next;
        });
    }
    int set_ref(uint32_t r) {
        return code_of([&] {
            gate_reference_group_rule(members, r, order);
            const FrameSettings next = propose_gate_reference(fs, r);
            frame_settings_rules(next, SET_GATE_REFERENCE, false);
            fs = next;
        });
    }
    int set_settle(float s, int32_t cap) {
        return code_of([&] {
            const FrameSettings next = propose_gate_settle(fs, s, cap);
            gate_settle_group_rule(members, s, order);
            frame_settings_rules(next, SET_GATE_REFERENCE, false);
            fs = next;
        });
    }
};

// what the header states, written down once more: a settle needs ANCHOR; with more than one member HALO stands beside PREVIOUS
// without a settle only
bool allowed(int members, uint32_t order, uint32_t ref, bool settle) {
    if (settle && ref != SLIDEO_GATE_ANCHOR) return false;
    if (members > 1 && order == SLIDEO_GROUP_GATE_HALO && (ref == SLIDEO_GATE_ANCHOR || settle)) return false;
    return true;
}

int rule_table() {
    int walked = 0, refused = 0;
    const uint32_t orders[2] = {SLIDEO_GROUP_GATE_HALO, SLIDEO_GROUP_GATE_CHAIN}, refs[2] = {SLIDEO_GATE_PREVIOUS, SLIDEO_GATE_ANCHOR};
    for (int members : {1, 2, 3})
        for (uint32_t o0 : orders) for (uint32_t r0 : refs) for (int s0 : {0, 1}) {
            if (!allowed(members, o0, r0, s0 != 0)) continue;              // (the values in force keep every rule)
            for (uint32_t o1 : orders) for (uint32_t r1 : refs) for (int s1 : {0, 1}) {
                int perm[3] = {0, 1, 2};
                do {
                    G g;
                    g.members = members; g.order = o0; g.fs.gate_ref = r0;
                    g.fs.settle_similarity = s0 ? 0.99f : 0.f; g.fs.settle_max_defer = s0 ? 7 : 0;
                    for (int step = 0; step < 3; ++step) {
                        const uint32_t bo = g.order, br = g.fs.gate_ref;
                        const float bs = g.fs.settle_similarity;
                        const int32_t bc = g.fs.settle_max_defer;
                        uint32_t no = bo, nr = br;
                        bool ns = bs > 0.f;
                        int rc;
                        if (perm[step] == 0) { no = o1; rc = g.set_order(o1); }
                        else if (perm[step] == 1) { nr = r1; rc = g.set_ref(r1); }
                        else { ns = s1 != 0; rc = g.set_settle(s1 ? 0.99f : 0.f, s1 ? 3 : 0); }
                        const bool ok = allowed(members, no, nr, ns);
                        expect(rc == (ok ? 0 : SLIDEO_ERR_UNSUPPORTED), "the call that completes the refused combination is SLIDEO_ERR_UNSUPPORTED, every other passes");
                        if (ok) expect(g.order == no && g.fs.gate_ref == nr && (g.fs.settle_similarity > 0.f) == ns, "an accepted call is in force");
                        else {
                            ++refused;
                            expect(g.order == bo && g.fs.gate_ref == br && g.fs.settle_similarity == bs && g.fs.settle_max_defer == bc, "a refused call leaves the values before");
                        }
                        expect(allowed(members, g.order, g.fs.gate_ref, g.fs.settle_similarity > 0.f), "the values in force keep every rule");
                        ++walked;
                    }
                } while (std::next_permutation(perm, perm + 3));
            }
        }
    // the range check comes first and leaves the value
    for (int members : {1, 2}) {
        G g;
        g.members = members;
        for (uint32_t bad : {2u, 7u, 0xFFFFFFFFu}) expect(g.set_order(bad) == SLIDEO_ERR_INVALID_ARG && g.order == SLIDEO_GROUP_GATE_HALO, "an unknown order is SLIDEO_ERR_INVALID_ARG");
    }
    // the default order refuses with the words the earlier sections promise
    try { gate_reference_group_rule(2, SLIDEO_GATE_ANCHOR); expect(false, "HALO refuses ANCHOR on two members"); }
    catch (const Error& e) { expect(e.code == SLIDEO_ERR_UNSUPPORTED && std::strstr(e.what(), "one member") != nullptr, "the ANCHOR refusal names one member"); }
    try { gate_settle_group_rule(2, 0.99f); expect(false, "HALO refuses a settle on two members"); }
    catch (const Error& e) { expect(e.code == SLIDEO_ERR_UNSUPPORTED && std::strstr(e.what(), "one member") != nullptr, "the settle refusal names one member"); }
    expect(code_of([] { gate_reference_group_rule(5, SLIDEO_GATE_ANCHOR, SLIDEO_GROUP_GATE_CHAIN); }) == 0, "CHAIN accepts ANCHOR on five members");
    expect(code_of([] { gate_settle_group_rule(5, 0.99f, SLIDEO_GROUP_GATE_CHAIN); }) == 0, "CHAIN accepts a settle on five members");
    std::printf("rule table: %d set calls walked, %d refused\n", walked, refused);
    return walked;
}

// ---- the record header ------------------------------------------------------------------------------------------------------------------
void record_header() {
    const int small_area = 4096;
    int trips = 0;
    for (uint32_t ref : {SLIDEO_GATE_PREVIOUS, SLIDEO_GATE_ANCHOR})
        for (int settle : {0, 1}) {
            if (settle && ref != SLIDEO_GATE_ANCHOR) continue;
            for (int has : {0, 1})
                for (uint32_t d : {0u, 1u, 3u}) {
                    if (d && !(has && settle)) continue;
                    GateRecordHead h;
                    h.has = has != 0; h.gate_ref = ref; h.settle = settle != 0;
                    if (has) { h.sw = 85; h.sh = 48; h.d = d; }
                    std::vector<uint8_t> rec((size_t)h.bytes(), 0xA5);
                    gate_record_encode(h, rec.data());
                    expect(h.bytes() == 32 + (has ? 85 * 48 * 3 * (settle ? 2 : 1) : 0), "the record's size: header, anchor and, under a settle, the previous image");
                    const float s = settle ? 0.99f : 0.f;
                    GateRecordHead back;
                    expect(code_of([&] { back = gate_record_validate(rec.data(), (int64_t)rec.size(), ref, s, 3, small_area); }) == 0, "a record validates under its own settings");
                    expect(back.has == h.has && back.gate_ref == h.gate_ref && back.settle == h.settle && back.sw == h.sw && back.sh == h.sh && back.d == h.d, "the header round trip");
                    ++trips;
                    auto refused = [&](std::vector<uint8_t> r, int64_t bytes, uint32_t mref, float ms, int32_t cap, int area, const char* what) {
                        expect(code_of([&] { gate_record_validate(r.data(), bytes, mref, ms, cap, area); }) == SLIDEO_ERR_INVALID_ARG, what);
                    };
                    const int64_t n = (int64_t)rec.size();
                    refused(rec, n - 1, ref, s, 3, small_area, "one byte short");
                    refused(rec, n + 1, ref, s, 3, small_area, "one byte long");
                    refused(rec, 31, ref, s, 3, small_area, "shorter than a header");
                    refused(rec, 0, ref, s, 3, small_area, "empty");
                    { auto r = rec; r[0] ^= 1; refused(r, n, ref, s, 3, small_area, "bad magic"); }
                    { auto r = rec; r[4] = 2; refused(r, n, ref, s, 3, small_area, "bad version"); }
                    { auto r = rec; r[8] = 2; refused(r, n, ref, s, 3, small_area, "has outside 0, 1"); }
                    refused(rec, n, ref ^ 1u, s, 3, small_area, "another gate reference");
                    refused(rec, n, ref, settle ? 0.f : 0.99f, 3, small_area, "another settle on / off");
                    if (has) {
                        refused(rec, n, ref, s, 3, 85 * 48 - 1, "a small image beyond small_area");
                        { auto r = rec; gate_record_put32(r.data() + 20, 0); refused(r, n, ref, s, 3, small_area, "sw 0"); }
                        { auto r = rec; gate_record_put32(r.data() + 24, 0xFFFFFFFFu); refused(r, n, ref, s, 3, small_area, "sh -1"); }
                        { auto r = rec; gate_record_put32(r.data() + 28, 4); refused(r, n, ref, s, 3, small_area, "d beyond max_defer"); }
                    } else {
                        auto r = rec; gate_record_put32(r.data() + 20, 5); refused(r, n, ref, s, 3, small_area, "a record of none with a size");
                    }
                }
        }
    expect(code_of([] { gate_record_validate(nullptr, 32, 0, 0.f, 0, 4096); }) == SLIDEO_ERR_INVALID_ARG, "a null record");
    // little-endian, byte by byte
    GateRecordHead h;
    h.has = true; h.gate_ref = SLIDEO_GATE_ANCHOR; h.settle = true; h.sw = 0x0102; h.sh = 3; h.d = 0x01020304u;
    uint8_t head[32];
    gate_record_encode(h, head);
    const uint8_t want[32] = {0x53, 0x47, 0x53, 0x54, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 2, 1, 0, 0, 3, 0, 0, 0, 4, 3, 2, 1};
    expect(std::memcmp(head, want, 32) == 0, "the header's bytes are the layout the public header states");
    std::printf("record header: %d round trips, every refusal\n", trips);
}

// ---- the baton ----------------------------------------------------------------------------------------------------------------------------
void baton() {
    using namespace std::chrono_literals;
    {   // publish, then await: returns at once
        GateBaton b;
        b.publish();
        expect(b.settled(), "a published baton is settled");
        double w = -1.0;
        std::thread t([&] { w = b.await(); });
        t.join();
        expect(w >= 0.0, "await behind publish returns");
    }
    {   // await, then publish: the reader sees what was written in front of the publish
        GateBaton b;
        int payload = 0, seen = -1;
        std::thread t([&] { b.await(); seen = payload; });
        std::this_thread::sleep_for(20ms);
        payload = 42;
        b.publish();
        t.join();
        expect(seen == 42, "await in front of publish sees the record");
    }
    {   // fail makes await throw, with the reason
        GateBaton b;
        bool threw = false;
        std::thread t([&] { try { b.await(); } catch (const std::runtime_error& e) { threw = std::strstr(e.what(), "boom") != nullptr; } });
        b.fail("boom");
        t.join();
        expect(threw, "fail makes await throw");
        b.publish();                                    // (settled once: a later publish changes nothing)
        expect(code_of([&] { try { b.await(); } catch (const std::runtime_error&) { throw Error(SLIDEO_ERR_HIP, "failed"); } }) == SLIDEO_ERR_HIP, "a failed baton stays failed");
        b.reset();
        expect(!b.settled(), "reset makes it pending again");
    }
    {   // a guard dropped unpublished counts as a failure; a published one does not
        GateBaton b, c;
        { GateBatonGuard g(&b); }
        bool threw = false;
        try { b.await(); } catch (const std::runtime_error&) { threw = true; }
        expect(threw, "a guard dropped unpublished fails the baton");
        { GateBatonGuard g(&c); g.publish(); }
        expect(code_of([&] { c.await(); }) == 0, "a guard that published leaves the baton published");
        { GateBatonGuard none(nullptr); none.publish(); }                     // (the last member owes nothing)
    }
    {   // a chain of 5 with member 2 failing: 0 and 1 publish, 2 throws before it publishes, 3 and 4 end with a failure; all threads end
        const int N = 5;
        std::vector<std::unique_ptr<GateBaton>> link;
        for (int r = 0; r + 1 < N; ++r) link.emplace_back(new GateBaton());
        std::vector<int> outcome((size_t)N, -1);              // 0: ran, 1: failed itself, 2: released with a failure
        std::vector<std::thread> th;
        for (int r = 0; r < N; ++r)
            th.emplace_back([&, r] {
                try {
                    GateBatonGuard owed(r + 1 < N ? link[(size_t)r].get() : nullptr);
                    if (r > 0) {
                        try { link[(size_t)r - 1]->await(); } catch (const std::runtime_error&) { outcome[(size_t)r] = 2; throw; }
                    }
                    if (r == 2) { outcome[(size_t)r] = 1; throw std::runtime_error("member 2"); }
                    owed.publish();
                    outcome[(size_t)r] = 0;
                } catch (const std::runtime_error&) {}
            });
        for (auto& t : th) t.join();
        expect(outcome == std::vector<int>({0, 0, 1, 2, 2}), "a chain of 5 with member 2 failing ends every thread, the later ones with a failure");
    }
    {   // a chain that runs: every member hands a count on, in order
        const int N = 8;
        std::vector<std::unique_ptr<GateBaton>> link;
        for (int r = 0; r + 1 < N; ++r) link.emplace_back(new GateBaton());
        std::vector<int> rec((size_t)N, 0);
        std::vector<std::thread> th;
        for (int r = N - 1; r >= 0; --r)
            th.emplace_back([&, r] {
                GateBatonGuard owed(r + 1 < N ? link[(size_t)r].get() : nullptr);
                int carried = 0;
                if (r > 0) { link[(size_t)r - 1]->await(); carried = rec[(size_t)r - 1]; }
                rec[(size_t)r] = carried + 1;
                owed.publish();
            });
        for (auto& t : th) t.join();
        expect(rec[(size_t)N - 1] == N, "a chain of 8 hands its state on in order");
    }
    std::printf("baton: publish / await in both orders, fail, guard, chains of 5 and 8\n");
}

}  // namespace

int main(int argc, char** argv) {
    const char* part = argc > 1 ? argv[1] : "all";
    const bool all = std::strcmp(part, "all") == 0;
    if (all || std::strcmp(part, "rules") == 0) rule_table();
    if (all || std::strcmp(part, "record") == 0) record_header();
    if (all || std::strcmp(part, "baton") == 0) baton();
    if (fails) { std::fprintf(stderr, "%d checks failed\n", fails); return 1; }
    std::printf("group gate chain host check (%s): as stated\n", part);
    return 0;
}
