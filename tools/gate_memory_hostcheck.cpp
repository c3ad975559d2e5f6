// gate_memory_hostcheck — the host side of the gate memory (include/slideo_amd.h "Gate memory"; csrc/frame_settings.h) on its own:
// propose_gate_memory's ranges, the ANCHOR-only rule whichever call completes the combination, the group rule and the record calls'
// refusal as pure functions, the unchanged Setting enum, and gate_recall_kernel's walk — restated lane by lane in plain C++: 64 slots
// in 64 lanes, 64 frames per step against the anchor, the first away frame against every slot, a butterfly on (SSD, then the
// greater ordinal) — over the SSD tables of a case file, against the flags, SSDs, refs, occupants and ring the file states
// (tests/test_gate_memory_abi.py writes them from the numpy restatement, tests/gate_memory_ref.py).  No GPU, nothing loaded into Python.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -I include -I slideo_amd/csrc tools/gate_memory_hostcheck.cpp -o hostcheck && ./hostcheck cases.txt
// Case file, whitespace separated: the number of cases, then per case  n M count head anchor prev_ssd0 thr_c thr_s max_defer d_in none
// t0 | ordinals[M] | table[n * n] (row a, column j; read for a < j alone) | mtable[n * M] (row j, column slot) | flags[n] | ssd[n] |
// refs[n] | occupants[64] | head count anchor d.
#include <climits>
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

constexpr int SLOTS = SLIDEO_GATE_MEMORY_MAX;

// gate_recall_kernel's walk with its 64 lanes as loops
struct Walk {
    std::vector<uint8_t> flags; std::vector<int64_t> ssd, refs; std::vector<int32_t> kept;
    int32_t occ[SLOTS]; int32_t head, count, anchor; uint32_t d;
};
Walk walk(const std::vector<int64_t>& table, const std::vector<int64_t>& mtable, const std::vector<int64_t>& ordinals, int n, int M, int count_in,
          int head_in, int anchor_in, int64_t prev_ssd0, int64_t thr_c, int64_t thr_s, uint32_t max_defer, uint32_t d_in, bool none, int64_t t0) {
    Walk w{std::vector<uint8_t>((size_t)n, 0xEE), std::vector<int64_t>((size_t)n, -1), std::vector<int64_t>((size_t)n, -99), {}, {}, 0, 0, 0, 0};
    int occ[64];
    int64_t ord[64];
    for (int l = 0; l < 64; ++l) { occ[l] = -1; ord[l] = LLONG_MIN; }
    int cnt = 0, head = 0, anc = 0, i = 0;
    uint32_t d = 0;
    const bool defer = max_defer != 0;
    if (none) {
        occ[0] = 0; ord[0] = t0;
        w.flags[0] = 1; w.ssd[0] = 0; w.refs[0] = t0; w.kept.push_back(0);
        cnt = 1; head = M > 1 ? 1 : 0; i = 1;
    } else {
        cnt = count_in; head = head_in; anc = anchor_in;
        d = d_in < max_defer ? d_in : max_defer;
        for (int l = 0; l < cnt; ++l) ord[l] = ordinals[(size_t)l];
    }
    auto against = [&](int slot, int j) {
        return occ[slot] < 0 ? mtable[(size_t)j * M + slot] : table[(size_t)occ[slot] * n + j];
    };
    while (i < n) {
        int64_t s[64];
        uint64_t ab = 0, sb = 0;
        for (int lane = 0; lane < 64; ++lane) {
            const int j = i + lane;
            s[lane] = 0;
            if (j >= n) continue;
            s[lane] = against(anc, j);
            if (s[lane] >= thr_c) ab |= 1ull << lane;
            if (defer && (j == 0 ? prev_ssd0 : table[(size_t)(j - 1) * n + j]) < thr_s) sb |= 1ull << lane;
        }
        const int f = ab ? __builtin_ctzll(ab) : 64;
        for (int lane = 0; lane < 64 && lane < f; ++lane) {
            const int j = i + lane;
            if (j >= n) break;
            w.flags[(size_t)j] = 0; w.ssd[(size_t)j] = s[lane]; w.refs[(size_t)j] = ord[anc];
        }
        if (f == 64) { d = 0; i += 64; continue; }
        if (f > 0) d = 0;
        const int jf = i + f;
        int64_t e[64], eo[64];
        int es[64];
        for (int lane = 0; lane < 64; ++lane) {
            e[lane] = LLONG_MAX; eo[lane] = LLONG_MIN; es[lane] = lane;
            if (lane < cnt) { e[lane] = against(lane, jf); eo[lane] = ord[lane]; }
        }
        for (int x = 32; x > 0; x >>= 1) {
            int64_t ne[64], no[64];
            int ns[64];
            for (int lane = 0; lane < 64; ++lane) {
                const int o = lane ^ x;
                const bool take = e[o] < e[lane] || (e[o] == e[lane] && eo[o] > eo[lane]);
                ne[lane] = take ? e[o] : e[lane]; no[lane] = take ? eo[o] : eo[lane]; ns[lane] = take ? es[o] : es[lane];
            }
            std::memcpy(e, ne, sizeof(e)); std::memcpy(eo, no, sizeof(eo)); std::memcpy(es, ns, sizeof(es));
        }
        for (int lane = 1; lane < 64; ++lane) expect(e[lane] == e[0] && eo[lane] == eo[0] && es[lane] == es[0], "every lane ends the butterfly with the same entry");
        int fl = 0;
        int64_t r;
        if (e[0] < thr_c) { anc = es[0]; d = 0; r = eo[0]; }
        else if (((sb >> f) & 1ull) || d >= max_defer) {
            fl = 1;
            occ[head] = jf; ord[head] = t0 + jf;
            anc = head;
            head = head + 1 < M ? head + 1 : 0;
            cnt = cnt < M ? cnt + 1 : M;
            d = 0; r = t0 + jf;
        } else { d = d + 1 < max_defer ? d + 1 : max_defer; r = SLIDEO_GATE_REF_DEFERRED; }
        w.flags[(size_t)jf] = (uint8_t)fl; w.ssd[(size_t)jf] = s[f]; w.refs[(size_t)jf] = r;
        if (fl) w.kept.push_back(jf);
        i = jf + 1;
    }
    for (int l = 0; l < SLOTS; ++l) w.occ[l] = l < M ? occ[l] : -1;
    w.head = head; w.count = cnt; w.anchor = anc; w.d = d;
    return w;
}

bool read_i64(std::FILE* fp, int64_t& v) { long long t; if (std::fscanf(fp, "%lld", &t) != 1) return false; v = t; return true; }

int run_cases(const char* path) {
    std::FILE* fp = std::fopen(path, "r");
    if (!fp) { std::fprintf(stderr, "cannot open %s\n", path); return -1; }
    int64_t cases = 0;
    if (!read_i64(fp, cases) || cases < 0 || cases > 10000) { std::fclose(fp); return -1; }
    for (int64_t c = 0; c < cases; ++c) {
        int64_t h[12], v = 0;
        bool ok = true;
        for (auto& x : h) ok = ok && read_i64(fp, x);
        const int64_t n = h[0], M = h[1], count = h[2], head = h[3], anchor = h[4], prev_ssd0 = h[5], thr_c = h[6], thr_s = h[7], max_defer = h[8],
                      d_in = h[9], none = h[10], t0 = h[11];
        if (!ok || n < 1 || n > 4096 || M < 1 || M > SLOTS || max_defer < 0 || max_defer > INT32_MAX || d_in < 0 || d_in > max_defer ||
            (!none && (count < 1 || count > M || head < 0 || head >= M || anchor < 0 || anchor >= count))) { std::fclose(fp); return -1; }
        std::vector<int64_t> ordinals((size_t)M), table((size_t)n * n), mtable((size_t)n * M), ssd((size_t)n), refs((size_t)n);
        std::vector<uint8_t> flags((size_t)n);
        int64_t occ[SLOTS], tail[4];
        for (auto& x : ordinals) ok = ok && read_i64(fp, x);
        for (auto& x : table) ok = ok && read_i64(fp, x);
        for (auto& x : mtable) ok = ok && read_i64(fp, x);
        for (auto& x : flags) { ok = ok && read_i64(fp, v); x = (uint8_t)v; }
        for (auto& x : ssd) ok = ok && read_i64(fp, x);
        for (auto& x : refs) ok = ok && read_i64(fp, x);
        for (auto& x : occ) ok = ok && read_i64(fp, x);
        for (auto& x : tail) ok = ok && read_i64(fp, x);
        if (!ok) { std::fclose(fp); return -1; }
        const Walk w = walk(table, mtable, ordinals, (int)n, (int)M, (int)count, (int)head, (int)anchor, prev_ssd0, thr_c, thr_s, (uint32_t)max_defer,
                            (uint32_t)d_in, none != 0, t0);
        char what[160];
        std::snprintf(what, sizeof(what), "case %lld (n %lld, M %lld, count %lld, max_defer %lld, d_in %lld, none %lld)", (long long)c, (long long)n,
                      (long long)M, (long long)count, (long long)max_defer, (long long)d_in, (long long)none);
        expect(w.flags == flags && w.ssd == ssd && w.refs == refs, what);
        bool same = true;
        for (int l = 0; l < SLOTS; ++l) same = same && w.occ[l] == (int32_t)occ[l];
        expect(same && w.head == (int32_t)tail[0] && w.count == (int32_t)tail[1] && w.anchor == (int32_t)tail[2] && w.d == (uint32_t)tail[3], what);
        std::vector<int32_t> kept;
        for (int j = 0; j < (int)n; ++j) if (flags[(size_t)j]) kept.push_back(j);
        expect(w.kept == kept, what);
    }
    std::fclose(fp);
    return (int)cases;
}

}  // namespace

int main(int argc, char** argv) {
    // the proposal: off by default; the range; a refused proposal leaves the value before
    FrameSettings s;
    expect(s.gate_memory == 0, "the default is off");
    const FrameSettings anchor = propose_gate_reference(s, SLIDEO_GATE_ANCHOR);
    for (int32_t ok : {0, 1, 2, 4, 63, 64}) {
        FrameSettings t = anchor;
        expect(code_of([&] { t = propose_gate_memory(t, ok); }) == 0 && t.gate_memory == ok, "a capacity in range is accepted");
        expect(t.gate_ref == SLIDEO_GATE_ANCHOR && t.settle_similarity == anchor.settle_similarity && t.direct_t == anchor.direct_t, "other settings stay");
    }
    for (int32_t bad : {-1, 65, 128, INT32_MAX, INT32_MIN}) {
        FrameSettings t = propose_gate_memory(anchor, 7);
        expect(code_of([&] { t = propose_gate_memory(t, bad); }) == SLIDEO_ERR_INVALID_ARG, "a capacity outside 0 .. 64 is SLIDEO_ERR_INVALID_ARG");
        expect(t.gate_memory == 7, "a refused proposal leaves the value before");
    }
    // the ANCHOR-only rule, in both call orders, with and without a settle
    {
        FrameSettings t;                                             // PREVIOUS
        expect(set(t, [](const FrameSettings& u) { return propose_gate_memory(u, 4); }) == SLIDEO_ERR_UNSUPPORTED, "a memory under PREVIOUS is SLIDEO_ERR_UNSUPPORTED");
        expect(t.gate_memory == 0 && t.gate_ref == SLIDEO_GATE_PREVIOUS, "and nothing changes");
        expect(set(t, [](const FrameSettings& u) { return propose_gate_memory(u, 0); }) == 0, "a memory of 0 under PREVIOUS is accepted");
        expect(set(t, [](const FrameSettings& u) { return propose_gate_reference(u, SLIDEO_GATE_ANCHOR); }) == 0, "ANCHOR");
        expect(set(t, [](const FrameSettings& u) { return propose_gate_memory(u, 4); }) == 0 && t.gate_memory == 4, "a memory under ANCHOR is accepted");
        expect(set(t, [](const FrameSettings& u) { return propose_gate_reference(u, SLIDEO_GATE_PREVIOUS); }) == SLIDEO_ERR_UNSUPPORTED,
               "PREVIOUS while a memory is on is SLIDEO_ERR_UNSUPPORTED");
        expect(t.gate_ref == SLIDEO_GATE_ANCHOR && t.gate_memory == 4, "and the values before stay in force");
        expect(set(t, [](const FrameSettings& u) { return propose_gate_settle(u, 0.99f, 4); }) == 0 && t.gate_memory == 4, "a settle beside the memory is accepted");
        expect(set(t, [](const FrameSettings& u) { return propose_gate_settle(u, 0.f, 0); }) == 0, "settle off");
        expect(set(t, [](const FrameSettings& u) { return propose_gate_reference(u, SLIDEO_GATE_PREVIOUS); }) == SLIDEO_ERR_UNSUPPORTED, "still refused: the memory is on");
        expect(set(t, [](const FrameSettings& u) { return propose_gate_memory(u, 0); }) == 0, "memory off");
        expect(set(t, [](const FrameSettings& u) { return propose_gate_reference(u, SLIDEO_GATE_PREVIOUS); }) == 0 && t.gate_ref == SLIDEO_GATE_PREVIOUS,
               "then PREVIOUS is accepted");
        FrameSettings u = propose_gate_memory(anchor, 3);
        u.gate_ref = SLIDEO_GATE_PREVIOUS;
        for (int what = 0; what < N_SETTINGS; ++what)
            for (bool sift : {false, true})
                expect(code_of([&] { frame_settings_rules(u, (Setting)what, sift); }) == SLIDEO_ERR_UNSUPPORTED, "the rule holds for every setting");
    }
    // the memory is part of the gate-reference setting: the enum did not grow, its row ends the gate state alone
    static_assert(N_SETTINGS == 8 && SET_GATE_REFERENCE == N_SETTINGS - 1, "the gate memory adds no setting");
    const SettingEnds e = SETTING_ENDS[SET_GATE_REFERENCE];
    expect(!e.kept && e.gate && !e.map_gen, "SETTING_ENDS[SET_GATE_REFERENCE] = {kept false, gate true, map_gen false}");
    // the group rule: a memory that is on needs one member; off always passes
    for (int members : {1, 2, 3, 8, 64}) {
        expect(code_of([&] { gate_memory_group_rule(members, 0); }) == 0, "a group accepts a memory of 0");
        expect(code_of([&] { gate_memory_group_rule(members, 4); }) == (members == 1 ? 0 : SLIDEO_ERR_UNSUPPORTED),
               "a group of one member accepts a memory, a larger one is SLIDEO_ERR_UNSUPPORTED");
    }
    // the record calls: refused by name while a memory is on
    expect(code_of([&] { gate_record_memory_rule(0); }) == 0, "the record calls work without a memory");
    for (int32_t M : {1, 4, 64}) expect(code_of([&] { gate_record_memory_rule(M); }) == SLIDEO_ERR_UNSUPPORTED, "the record calls are SLIDEO_ERR_UNSUPPORTED while a memory is on");
    static_assert(SLIDEO_GATE_REF_RESET == -1 && SLIDEO_GATE_REF_DEFERRED == -2 && SLIDEO_GATE_MEMORY_MAX == 64, "the header's three values");
    int cases = 0;
    if (argc > 1) {
        cases = run_cases(argv[1]);
        if (cases < 0) { std::fprintf(stderr, "bad case file\n"); return 2; }
    }
    if (fails) { std::fprintf(stderr, "%d checks failed\n", fails); return 1; }
    std::printf("gate memory: proposal, rule, group rule, record rule and %d walks: as stated\n", cases);
    return 0;
}
