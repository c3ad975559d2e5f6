// gate_anchor_hostcheck — the host side of the gate reference (include/slideo_amd.h "Gate reference"; csrc/frame_settings.h) on its own:
// propose_gate_reference's refusals, the SETTING_ENDS row, the group rule as a pure function, and the walk of gate_settle_kernel at a cap of 0 —
// restated lane by lane in plain C++: 64 frames per step, the first flagged one becomes the anchor — over the SSD tables of a case
// file, against the flags, SSDs and last anchor the file states (tests/test_gate_anchor_abi.py writes them from the numpy
// restatement, tests/gate_anchor_ref.py).  No GPU, nothing loaded into Python.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -I include -I slideo_amd/csrc tools/gate_anchor_hostcheck.cpp -o hostcheck && ./hostcheck cases.txt
// Case file, whitespace separated: the number of cases, then per case  n thr none | carried[n] | table[n * n] (row a, column j; read
// for a < j alone) | flags[n] | ssd[n] | last anchor.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "frame_settings.h"

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

// The walk of gate_settle_kernel (csrc/gate_anchor.hip.h) at a cap of 0 — plain ANCHOR — as its own loop, a second opinion on the
// kernel the settle shares: the 64 lanes test frames i .. i + 63 against the anchor a
// (-1: the carried one), the ballot's first set bit f is the next anchor, lanes <= f write their frame
struct Walk { std::vector<uint8_t> flags; std::vector<int64_t> ssd; std::vector<int32_t> kept; int32_t anchor; };
Walk walk(const std::vector<int64_t>& table, const std::vector<int64_t>& carried, int n, int64_t thr, bool none) {
    Walk w{std::vector<uint8_t>((size_t)n, 0xEE), std::vector<int64_t>((size_t)n, -1), {}, -1};
    int a = -1, i = 0;
    if (none && n > 0) { w.flags[0] = 1; w.ssd[0] = 0; w.kept.push_back(0); a = 0; i = 1; }
    while (i < n) {
        int64_t s[64];
        uint64_t ballot = 0;
        for (int lane = 0; lane < 64; ++lane) {
            const int j = i + lane;
            s[lane] = 0;
            if (j >= n) continue;
            s[lane] = a < 0 ? carried[(size_t)j] : table[(size_t)a * n + j];
            if (s[lane] >= thr) ballot |= 1ull << lane;
        }
        const int f = ballot ? __builtin_ctzll(ballot) : 64;
        for (int lane = 0; lane < 64; ++lane) {
            const int j = i + lane;
            if (j >= n || lane > f) continue;
            w.flags[(size_t)j] = lane == f ? 1 : 0;
            w.ssd[(size_t)j] = s[lane];
            if (lane == f) w.kept.push_back(j);
        }
        if (f < 64) { a = i + f; i = a + 1; }
        else i += 64;
    }
    w.anchor = a;
    return w;
}

bool read_i64(std::FILE* fp, int64_t& v) { long long t; if (std::fscanf(fp, "%lld", &t) != 1) return false; v = t; return true; }

int run_cases(const char* path) {
    std::FILE* fp = std::fopen(path, "r");
    if (!fp) { std::fprintf(stderr, "cannot open %s\n", path); return -1; }
    int64_t cases = 0;
    if (!read_i64(fp, cases) || cases < 0 || cases > 10000) { std::fclose(fp); return -1; }
    for (int64_t c = 0; c < cases; ++c) {
        int64_t n = 0, thr = 0, none = 0, v = 0, last = 0;
        if (!read_i64(fp, n) || !read_i64(fp, thr) || !read_i64(fp, none) || n < 0 || n > 4096) { std::fclose(fp); return -1; }
        std::vector<int64_t> carried((size_t)n), table((size_t)n * n), ssd((size_t)n);
        std::vector<uint8_t> flags((size_t)n);
        bool ok = true;
        for (auto& x : carried) ok = ok && read_i64(fp, x);
        for (auto& x : table) ok = ok && read_i64(fp, x);
        for (auto& x : flags) { ok = ok && read_i64(fp, v); x = (uint8_t)v; }
        for (auto& x : ssd) ok = ok && read_i64(fp, x);
        ok = ok && read_i64(fp, last);
        if (!ok) { std::fclose(fp); return -1; }
        const Walk w = walk(table, carried, (int)n, thr, none != 0);
        char what[96];
        std::snprintf(what, sizeof(what), "case %lld (n %lld, thr %lld, none %lld)", (long long)c, (long long)n, (long long)thr, (long long)none);
        expect(w.flags == flags && w.ssd == ssd && w.anchor == (int32_t)last, what);
        // the kept list is the flagged frames, ascending
        std::vector<int32_t> kept;
        for (int j = 0; j < (int)n; ++j) if (flags[(size_t)j]) kept.push_back(j);
        expect(w.kept == kept, what);
    }
    std::fclose(fp);
    return (int)cases;
}

}  // namespace

int main(int argc, char** argv) {
    // the proposal: the two values pass and are what the record then holds; anything else is refused and nothing changes
    FrameSettings s;
    expect(s.gate_ref == SLIDEO_GATE_PREVIOUS, "the default is PREVIOUS");
    expect(propose_gate_reference(s, SLIDEO_GATE_ANCHOR).gate_ref == SLIDEO_GATE_ANCHOR, "ANCHOR is accepted");
    expect(propose_gate_reference(propose_gate_reference(s, SLIDEO_GATE_ANCHOR), SLIDEO_GATE_PREVIOUS).gate_ref == SLIDEO_GATE_PREVIOUS, "and PREVIOUS after it");
    for (uint32_t bad : {2u, 3u, 255u, 0x80000000u, 0xFFFFFFFFu}) {
        FrameSettings t = propose_gate_reference(s, SLIDEO_GATE_ANCHOR);
        expect(code_of([&] { t = propose_gate_reference(t, bad); }) == SLIDEO_ERR_INVALID_ARG, "an unknown value is SLIDEO_ERR_INVALID_ARG");
        expect(t.gate_ref == SLIDEO_GATE_ANCHOR, "a refused proposal leaves the value before");
    }
    {   // no other setting moves, and no rule between settings refuses either value
        FrameSettings t = propose_direct_similarity(propose_working_size(s, 160, 90), 0.9f);
        const FrameSettings u = propose_gate_reference(t, SLIDEO_GATE_ANCHOR);
        expect(u.work_w == 160 && u.work_h == 90 && u.direct_t == 0.9f && u.mask_scope == t.mask_scope && u.direct_scope == t.direct_scope, "other settings stay");
        expect(code_of([&] { frame_settings_rules(u, SET_GATE_REFERENCE, false); }) == 0 && code_of([&] { frame_settings_rules(u, SET_GATE_REFERENCE, true); }) == 0,
               "no rule between settings refuses a gate reference");
    }
    // what a change ends: the gate state alone (the state means another frame), not the kept frames, not the map's generation
    static_assert(SET_GATE_REFERENCE == N_SETTINGS - 1, "the newest setting is the last row");
    const SettingEnds e = SETTING_ENDS[SET_GATE_REFERENCE];
    expect(!e.kept && e.gate && !e.map_gen, "SETTING_ENDS[SET_GATE_REFERENCE] = {kept false, gate true, map_gen false}");
    // the group rule: ANCHOR needs one member; PREVIOUS always passes
    for (int members : {1, 2, 3, 8, 64}) {
        expect(code_of([&] { gate_reference_group_rule(members, SLIDEO_GATE_PREVIOUS); }) == 0, "a group accepts PREVIOUS");
        expect(code_of([&] { gate_reference_group_rule(members, SLIDEO_GATE_ANCHOR); }) == (members == 1 ? 0 : SLIDEO_ERR_UNSUPPORTED),
               "a group of one member accepts ANCHOR, a larger one is SLIDEO_ERR_UNSUPPORTED");
    }
    static_assert(GATE_ANCHOR_MAX_UNIT == 1024, "include/slideo_amd.h states the cap");
    int cases = 0;
    if (argc > 1) {
        cases = run_cases(argv[1]);
        if (cases < 0) { std::fprintf(stderr, "bad case file\n"); return 2; }
    }
    if (fails) { std::fprintf(stderr, "%d checks failed\n", fails); return 1; }
    std::printf("gate reference: proposal, ends row, group rule and %d walks: as stated\n", cases);
    return 0;
}
