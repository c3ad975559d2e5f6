// gate_settle_hostcheck — the host side of the gate settle (include/slideo_amd.h "Gate settle"; csrc/frame_settings.h) on its own:
// propose_gate_settle's ranges, the rule between the settle and the gate reference whichever call completes the combination, the
// group rule as a pure function, the unchanged Setting enum, and gate_settle_kernel's walk — restated lane by lane in plain C++: 64
// frames per step, one ballot of `away` from which every lane has its deferral count, the first matched lane becomes the anchor —
// over the SSD tables of a case file, against the flags, SSDs, last anchor and count the file states
// (tests/test_gate_settle_abi.py writes them from the numpy restatement, tests/gate_settle_ref.py).  No GPU, nothing loaded into Python.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -I include -I slideo_amd/csrc tools/gate_settle_hostcheck.cpp -o hostcheck && ./hostcheck cases.txt
// Case file, whitespace separated: the number of cases, then per case  n thr_c thr_s max_defer d_in none | carried[n + 1] |
// table[n * n] (row a, column j; read for a < j alone) | flags[n] | ssd[n] | last anchor | d_out.
#include <climits>
#include <cmath>
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

// a setter as it is made: the proposal, then the rules on the proposed settings; the settings in force change only when both pass
template <class P>
int set(FrameSettings& s, P propose) {
    return code_of([&] {
        const FrameSettings next = propose(s);
        frame_settings_rules(next, SET_GATE_REFERENCE, false);
        s = next;
    });
}

// settle_run of csrc/gate_anchor.hip.h
uint32_t settle_run(uint64_t away, int pos, uint32_t d, uint32_t max_defer) {
    const uint64_t below = pos >= 64 ? ~0ull : (1ull << pos) - 1ull;
    const uint64_t stop = ~away & below;
    const uint32_t run = stop ? (uint32_t)(pos - 1 - (63 - __builtin_clzll(stop))) : (uint32_t)pos + d;
    return run < max_defer ? run : max_defer;
}

// gate_settle_kernel's walk with its 64 lanes as loops; as the kernel, with max_defer == 0 (plain ANCHOR, a settle with a cap of 0)
// it reads neither d_in nor the previous-frame SSDs — carried[n] and the table's sub-diagonal —: matched = away, d = 0
struct Walk { std::vector<uint8_t> flags; std::vector<int64_t> ssd; std::vector<int32_t> kept; int32_t anchor; uint32_t d; };
Walk walk(const std::vector<int64_t>& table, const std::vector<int64_t>& carried, int n, int64_t thr_c, int64_t thr_s, uint32_t max_defer, uint32_t d_in,
          bool none) {
    Walk w{std::vector<uint8_t>((size_t)n, 0xEE), std::vector<int64_t>((size_t)n, -1), {}, -1, 0};
    int a = -1, i = 0;
    uint32_t d = 0;
    const bool defer = max_defer != 0;
    if (none) {
        if (n > 0) { w.flags[0] = 1; w.ssd[0] = 0; w.kept.push_back(0); a = 0; i = 1; }
    } else if (defer) d = d_in > max_defer ? max_defer : d_in;
    while (i < n) {
        int64_t s[64];
        bool away[64], still[64];
        uint64_t ab = 0, b = 0;
        for (int lane = 0; lane < 64; ++lane) {
            const int j = i + lane;
            s[lane] = 0; away[lane] = still[lane] = false;
            if (j >= n) continue;
            s[lane] = a < 0 ? carried[(size_t)j] : table[(size_t)a * n + j];
            away[lane] = s[lane] >= thr_c;
            if (away[lane]) ab |= 1ull << lane;
        }
        b = ab;
        if (defer) {
            b = 0;
            for (int lane = 0; lane < 64; ++lane) {
                const int j = i + lane;
                if (j < n) still[lane] = (j == 0 ? carried[(size_t)n] : table[(size_t)(j - 1) * n + j]) < thr_s;
                if (away[lane] && (still[lane] || settle_run(ab, lane, d, max_defer) >= max_defer)) b |= 1ull << lane;
            }
        }
        const int f = b ? __builtin_ctzll(b) : 64;
        for (int lane = 0; lane < 64; ++lane) {
            const int j = i + lane;
            if (j >= n || lane > f) continue;
            w.flags[(size_t)j] = lane == f ? 1 : 0;
            w.ssd[(size_t)j] = s[lane];
            if (lane == f) w.kept.push_back(j);
        }
        if (f < 64) { a = i + f; i = a + 1; d = 0; }
        else { d = settle_run(ab, n - i < 64 ? n - i : 64, d, max_defer); i += 64; }
    }
    w.anchor = a; w.d = d;
    return w;
}

bool read_i64(std::FILE* fp, int64_t& v) { long long t; if (std::fscanf(fp, "%lld", &t) != 1) return false; v = t; return true; }

int run_cases(const char* path) {
    std::FILE* fp = std::fopen(path, "r");
    if (!fp) { std::fprintf(stderr, "cannot open %s\n", path); return -1; }
    int64_t cases = 0;
    if (!read_i64(fp, cases) || cases < 0 || cases > 10000) { std::fclose(fp); return -1; }
    for (int64_t c = 0; c < cases; ++c) {
        int64_t n = 0, thr_c = 0, thr_s = 0, max_defer = 0, d_in = 0, none = 0, v = 0, last = 0, d_out = 0;
        if (!read_i64(fp, n) || !read_i64(fp, thr_c) || !read_i64(fp, thr_s) || !read_i64(fp, max_defer) || !read_i64(fp, d_in) || !read_i64(fp, none) ||
            n < 1 || n > 4096 || max_defer < 0 || max_defer > INT32_MAX || d_in < 0 || d_in > max_defer) { std::fclose(fp); return -1; }
        std::vector<int64_t> carried((size_t)n + 1), table((size_t)n * n), ssd((size_t)n);
        std::vector<uint8_t> flags((size_t)n);
        bool ok = true;
        for (auto& x : carried) ok = ok && read_i64(fp, x);
        for (auto& x : table) ok = ok && read_i64(fp, x);
        for (auto& x : flags) { ok = ok && read_i64(fp, v); x = (uint8_t)v; }
        for (auto& x : ssd) ok = ok && read_i64(fp, x);
        ok = ok && read_i64(fp, last) && read_i64(fp, d_out);
        if (!ok) { std::fclose(fp); return -1; }
        const Walk w = walk(table, carried, (int)n, thr_c, thr_s, (uint32_t)max_defer, (uint32_t)d_in, none != 0);
        char what[128];
        std::snprintf(what, sizeof(what), "case %lld (n %lld, max_defer %lld, d_in %lld, none %lld)", (long long)c, (long long)n, (long long)max_defer,
                      (long long)d_in, (long long)none);
        expect(w.flags == flags && w.ssd == ssd && w.anchor == (int32_t)last && w.d == (uint32_t)d_out, what);
        std::vector<int32_t> kept;
        for (int j = 0; j < (int)n; ++j) if (flags[(size_t)j]) kept.push_back(j);
        expect(w.kept == kept, what);
    }
    std::fclose(fp);
    return (int)cases;
}

}  // namespace

int main(int argc, char** argv) {
    // the proposal: off by default; the ranges; a refused proposal leaves the values before
    FrameSettings s;
    expect(s.settle_similarity == 0.f && s.settle_max_defer == 0, "the default is off");
    const FrameSettings anchor = propose_gate_reference(s, SLIDEO_GATE_ANCHOR);
    for (float ok : {0.f, 1e-6f, 0.5f, 0.99f, 1.f})
        for (int32_t md : {0, 1, 4, 1 << 30, INT32_MAX}) {
            FrameSettings t = anchor;
            expect(code_of([&] { t = propose_gate_settle(t, ok, md); }) == 0 && t.settle_similarity == ok && t.settle_max_defer == md, "a value in range is accepted");
            expect(t.gate_ref == SLIDEO_GATE_ANCHOR && t.direct_t == anchor.direct_t && t.mask_scope == anchor.mask_scope && t.work_w == anchor.work_w, "other settings stay");
        }
    const float bad_s[] = {-0.5f, -1e-6f, 1.0001f, 2.f, NAN, INFINITY, -INFINITY};
    for (float bad : bad_s) {
        FrameSettings t = propose_gate_settle(anchor, 0.9f, 7);
        expect(code_of([&] { t = propose_gate_settle(t, bad, 3); }) == SLIDEO_ERR_INVALID_ARG, "a settle similarity outside 0 .. 1 is SLIDEO_ERR_INVALID_ARG");
        expect(t.settle_similarity == 0.9f && t.settle_max_defer == 7, "a refused proposal leaves the values before");
    }
    for (int32_t bad : {-1, -70, INT32_MIN}) {
        FrameSettings t = propose_gate_settle(anchor, 0.9f, 7);
        expect(code_of([&] { t = propose_gate_settle(t, 0.5f, bad); }) == SLIDEO_ERR_INVALID_ARG, "a negative max_defer is SLIDEO_ERR_INVALID_ARG");
        expect(code_of([&] { t = propose_gate_settle(t, 0.f, bad); }) == SLIDEO_ERR_INVALID_ARG, "also when the settle is off");
        expect(t.settle_similarity == 0.9f && t.settle_max_defer == 7, "a refused proposal leaves the values before");
    }
    // the rule, against both gate references and whichever call completes the combination
    {
        FrameSettings t;                                             // PREVIOUS
        expect(set(t, [](const FrameSettings& u) { return propose_gate_settle(u, 0.99f, 4); }) == SLIDEO_ERR_UNSUPPORTED, "settle on under PREVIOUS is SLIDEO_ERR_UNSUPPORTED");
        expect(t.settle_similarity == 0.f && t.settle_max_defer == 0 && t.gate_ref == SLIDEO_GATE_PREVIOUS, "and nothing changes");
        expect(set(t, [](const FrameSettings& u) { return propose_gate_settle(u, 0.f, 9); }) == 0 && t.settle_max_defer == 9, "settle off under PREVIOUS is accepted");
        expect(set(t, [](const FrameSettings& u) { return propose_gate_reference(u, SLIDEO_GATE_ANCHOR); }) == 0, "ANCHOR");
        expect(set(t, [](const FrameSettings& u) { return propose_gate_settle(u, 0.99f, 4); }) == 0 && t.settle_similarity == 0.99f && t.settle_max_defer == 4,
               "settle on under ANCHOR is accepted");
        expect(set(t, [](const FrameSettings& u) { return propose_gate_reference(u, SLIDEO_GATE_PREVIOUS); }) == SLIDEO_ERR_UNSUPPORTED,
               "PREVIOUS while a settle is on is SLIDEO_ERR_UNSUPPORTED");
        expect(t.gate_ref == SLIDEO_GATE_ANCHOR && t.settle_similarity == 0.99f && t.settle_max_defer == 4, "and the values before stay in force");
        expect(set(t, [](const FrameSettings& u) { return propose_gate_reference(u, SLIDEO_GATE_ANCHOR); }) == 0, "ANCHOR again is accepted");
        expect(set(t, [](const FrameSettings& u) { return propose_gate_reference(u, 2u); }) == SLIDEO_ERR_INVALID_ARG && t.gate_ref == SLIDEO_GATE_ANCHOR,
               "the gate reference keeps its two values");
        expect(set(t, [](const FrameSettings& u) { return propose_gate_settle(u, 0.f, 0); }) == 0, "settle off");
        expect(set(t, [](const FrameSettings& u) { return propose_gate_reference(u, SLIDEO_GATE_PREVIOUS); }) == 0 && t.gate_ref == SLIDEO_GATE_PREVIOUS,
               "then PREVIOUS is accepted");
        // the rule is a rule between settings: it holds whatever setting is being changed, and in SIFT mode
        FrameSettings u = propose_gate_settle(anchor, 0.5f, 1);
        u.gate_ref = SLIDEO_GATE_PREVIOUS;
        for (int what = 0; what < N_SETTINGS; ++what)
            for (bool sift : {false, true})
                expect(code_of([&] { frame_settings_rules(u, (Setting)what, sift); }) == SLIDEO_ERR_UNSUPPORTED, "the rule holds for every setting");
    }
    // the settle is part of the gate-reference setting: the enum did not grow, its row ends the gate state alone
    static_assert(N_SETTINGS == 8 && SET_GATE_REFERENCE == N_SETTINGS - 1, "the gate settle adds no setting");
    const SettingEnds e = SETTING_ENDS[SET_GATE_REFERENCE];
    expect(!e.kept && e.gate && !e.map_gen, "SETTING_ENDS[SET_GATE_REFERENCE] = {kept false, gate true, map_gen false}");
    // the group rule: settle on needs one member; off always passes
    for (int members : {1, 2, 3, 8, 64}) {
        expect(code_of([&] { gate_settle_group_rule(members, 0.f); }) == 0, "a group accepts settle off");
        expect(code_of([&] { gate_settle_group_rule(members, 0.99f); }) == (members == 1 ? 0 : SLIDEO_ERR_UNSUPPORTED),
               "a group of one member accepts a settle, a larger one is SLIDEO_ERR_UNSUPPORTED");
    }
    // settle_run: the run of away frames in front of a position, the carried count when it reaches the window's start, the cap
    expect(settle_run(0, 0, 5, 9) == 5 && settle_run(0, 0, 5, 3) == 3, "position 0: the carried count, capped");
    expect(settle_run(0b0111, 3, 2, 100) == 5 && settle_run(0b0110, 3, 2, 100) == 2 && settle_run(0b0011, 3, 2, 100) == 0, "runs below position 3");
    expect(settle_run(~0ull, 64, 6, 1000) == 70 && settle_run(~0ull >> 1, 64, 6, 1000) == 0 && settle_run(~1ull, 64, 6, 1000) == 63, "the whole window");
    expect(settle_run(~0ull, 64, (uint32_t)INT32_MAX, (uint32_t)INT32_MAX) == (uint32_t)INT32_MAX, "no overflow at the largest count");
    int cases = 0;
    if (argc > 1) {
        cases = run_cases(argv[1]);
        if (cases < 0) { std::fprintf(stderr, "bad case file\n"); return 2; }
    }
    if (fails) { std::fprintf(stderr, "%d checks failed\n", fails); return 1; }
    std::printf("gate settle: proposal, rule, group rule and %d walks: as stated\n", cases);
    return 0;
}
