// frame_settings_hostcheck — the rules of csrc/frame_settings.h walked on the host: every ordered pair of the six frame settings,
// each with a value that is in force and a value that is off, from a matcher's defaults; then the refused combinations.  The
// outcome of the second call — accepted or refused, the error code, what it ends — is asserted against the literal tables below,
// which are written from include/slideo_amd.h ("Working size", "Frame region", "Frame mask", "Frame mask scope", "Direct page
// look-up", "Direct look-up scope"), not from the code under test.  tests/test_gpu_frame_settings.py holds the same pair table.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -I include -I slideo_amd/csrc tools/frame_settings_hostcheck.cpp -o hostcheck && ./hostcheck
#include <cstdio>
#include <cstring>

#include "frame_settings.h"

using namespace slideo;

namespace {

// the twelve calls: setting x {in force, off}
enum Call { WS_ON, WS_OFF, REGION_ON, REGION_OFF, MASK_ON, MASK_OFF, SCOPE_ON, SCOPE_OFF, T_ON, T_OFF, DSCOPE_ON, DSCOPE_OFF, N_CALLS };
const char* const CALL_NAME[N_CALLS] = {"working_size(160, 90)", "working_size(0, 0)", "frame_region(320x180 -> 128x72)", "frame_region(none)",
                                        "frame_mask(320x180)", "frame_mask(none)", "mask_scope(DETECT | GATE)", "mask_scope(DETECT)",
                                        "direct_similarity(0.9)", "direct_similarity(0)", "direct_scope(VALID)", "direct_scope(WHOLE)"};
const double REGION_M[9] = {2.5, 0, 0, 0, 2.5, 0, 0, 0, 1};      // the 128x72 output over the whole 320x180 frame

Setting setting_of(int call) { return (Setting)(call / 2); }

// one call against the settings in force, as a setter makes it: the proposal (range checks), the rules, the install.
// Returns the error code (0: accepted, `s` is then the new settings); *ends: "KGM" letters of what an accepted call ends.
int apply(FrameSettings& s, int call, bool sift_on, char* ends, int ws_w = 160, int ws_h = 90) {
    std::strcpy(ends, "---");
    try {
        FrameSettings next;
        switch (call) {
            case WS_ON: next = propose_working_size(s, ws_w, ws_h); break;
            case WS_OFF: next = propose_working_size(s, 0, 0); break;
            case REGION_ON: next = propose_frame_region(s, 320, 180, REGION_M, 128, 72); break;
            case REGION_OFF: next = propose_frame_region(s, 0, 0, nullptr, 0, 0); break;
            case MASK_ON: next = propose_frame_mask(s, true, 320, 180, 320); break;
            case MASK_OFF: next = propose_frame_mask(s, false, 0, 0, 0); break;
            case SCOPE_ON: next = propose_frame_mask_scope(s, SLIDEO_MASK_DETECT | SLIDEO_MASK_GATE); break;
            case SCOPE_OFF: next = propose_frame_mask_scope(s, SLIDEO_MASK_DETECT); break;
            case T_ON: next = propose_direct_similarity(s, 0.9f); break;
            case T_OFF: next = propose_direct_similarity(s, 0.f); break;
            case DSCOPE_ON: next = propose_direct_scope(s, SLIDEO_DIRECT_VALID); break;
            default: next = propose_direct_scope(s, SLIDEO_DIRECT_WHOLE); break;
        }
        frame_settings_rules(next, setting_of(call), sift_on);
        s = next;
        const SettingEnds e = SETTING_ENDS[setting_of(call)];
        if (e.kept) ends[0] = 'K';
        if (e.gate) ends[1] = 'G';
        if (e.map_gen) ends[2] = 'M';
        return 0;
    } catch (const Error& e) { return e.code; }
}

// The second call of every ordered pair, first call down, second call across: "<code>:<ends>".  With these values no pair is
// refused — the region's 128x72 fits the 160x90 working size, and the refused look-up needs three settings —, and what a call
// ends depends on its setting alone: working size K(ept frames) G(ate state) M(ap generation), region K G, mask and mask scope
// K M, the direct settings nothing.
#define ROW "0:KGM", "0:KGM", "0:KG-", "0:KG-", "0:K-M", "0:K-M", "0:K-M", "0:K-M", "0:---", "0:---", "0:---", "0:---"
const char* const PAIRS[N_CALLS][N_CALLS] = {{ROW}, {ROW}, {ROW}, {ROW}, {ROW}, {ROW}, {ROW}, {ROW}, {ROW}, {ROW}, {ROW}, {ROW}};
#undef ROW

// The refused combinations (and their allowed neighbours): the calls before, the call under test, SIFT mode, the code.
struct Combo { int n_before; int before[4]; int call; bool sift; int code; const char* ends; int ws_w, ws_h; };
const Combo COMBOS[] = {
    // a direct similarity beside a mask under SLIDEO_MASK_GATE: whichever of the three calls completes it is refused (5) ...
    {2, {MASK_ON, SCOPE_ON}, T_ON, false, SLIDEO_ERR_UNSUPPORTED, "---", 160, 90},
    {2, {T_ON, SCOPE_ON}, MASK_ON, false, SLIDEO_ERR_UNSUPPORTED, "---", 160, 90},
    {2, {T_ON, MASK_ON}, SCOPE_ON, false, SLIDEO_ERR_UNSUPPORTED, "---", 160, 90},
    // ... unless the direct scope is VALID; the way back to WHOLE is then the refused call
    {3, {DSCOPE_ON, MASK_ON, SCOPE_ON}, T_ON, false, 0, "---", 160, 90},
    {3, {DSCOPE_ON, T_ON, SCOPE_ON}, MASK_ON, false, 0, "K-M", 160, 90},
    {3, {DSCOPE_ON, T_ON, MASK_ON}, SCOPE_ON, false, 0, "K-M", 160, 90},
    {4, {DSCOPE_ON, MASK_ON, SCOPE_ON, T_ON}, DSCOPE_OFF, false, SLIDEO_ERR_UNSUPPORTED, "---", 160, 90},
    {4, {DSCOPE_ON, MASK_ON, SCOPE_ON, T_ON}, MASK_OFF, false, 0, "K-M", 160, 90},
    // a region's output fits the working size, whichever comes second
    {1, {REGION_ON}, WS_ON, false, SLIDEO_ERR_UNSUPPORTED, "---", 100, 60},
    {1, {REGION_ON}, WS_ON, false, 0, "KGM", 128, 72},
    {1, {WS_ON}, REGION_ON, false, 0, "KG-", 160, 90},
    // no mask in SIFT mode; clearing is allowed
    {0, {}, MASK_ON, true, SLIDEO_ERR_UNSUPPORTED, "---", 160, 90},
    {0, {}, MASK_OFF, true, 0, "K-M", 160, 90},
};

int fails = 0;
void expect(bool ok, const char* what, const char* a, const char* b) {
    if (ok) return;
    ++fails;
    std::fprintf(stderr, "FAIL %s: %s then %s\n", what, a, b);
}

// range refusals: SLIDEO_ERR_INVALID_ARG, nothing changed
template <class F>
void refused(const char* what, F propose) {
    int code = 0;
    try { (void)propose(FrameSettings{}); } catch (const Error& e) { code = e.code; }
    expect(code == SLIDEO_ERR_INVALID_ARG, "range", what, "");
}

}  // namespace

int main() {
    char ends[4], want[16];
    for (int a = 0; a < N_CALLS; ++a)
        for (int b = 0; b < N_CALLS; ++b) {
            FrameSettings s;
            expect(apply(s, a, false, ends) == 0, "first call", CALL_NAME[a], CALL_NAME[b]);
            const FrameSettings before = s;
            const int code = apply(s, b, false, ends);
            std::snprintf(want, sizeof(want), "%d:%s", code, ends);
            expect(std::strcmp(want, PAIRS[a][b]) == 0, want, CALL_NAME[a], CALL_NAME[b]);
            // an accepted call leaves every other setting as it was
            FrameSettings other = s;
            switch (setting_of(b)) {
                case SET_WORKING_SIZE: other.work_w = before.work_w; other.work_h = before.work_h; break;
                case SET_FRAME_REGION: other.region = before.region; break;
                case SET_FRAME_MASK: other.mask = before.mask; break;
                case SET_FRAME_MASK_SCOPE: other.mask_scope = before.mask_scope; break;
                case SET_DIRECT_SIMILARITY: other.direct_t = before.direct_t; break;
                default: other.direct_scope = before.direct_scope; break;
            }
            expect(other.work_w == before.work_w && other.work_h == before.work_h && other.region.set == before.region.set &&
                       other.region.out_w == before.region.out_w && other.mask.set == before.mask.set && other.mask.w == before.mask.w &&
                       other.mask_scope == before.mask_scope && other.direct_t == before.direct_t && other.direct_scope == before.direct_scope,
                   "other settings", CALL_NAME[a], CALL_NAME[b]);
        }
    for (const Combo& c : COMBOS) {
        FrameSettings s;
        for (int i = 0; i < c.n_before; ++i) expect(apply(s, c.before[i], c.sift, ends) == 0, "combination's set-up", CALL_NAME[c.before[i]], CALL_NAME[c.call]);
        const FrameSettings before = s;
        const int code = apply(s, c.call, c.sift, ends, c.ws_w, c.ws_h);
        expect(code == c.code && std::strcmp(ends, c.ends) == 0, "combination", c.n_before ? CALL_NAME[c.before[c.n_before - 1]] : "defaults", CALL_NAME[c.call]);
        if (code != 0)      // a refused call leaves the values before in force
            expect(s.work_w == before.work_w && s.region.set == before.region.set && s.mask.set == before.mask.set && s.mask_scope == before.mask_scope &&
                       s.direct_t == before.direct_t && s.direct_scope == before.direct_scope, "refused call changed a setting", "", CALL_NAME[c.call]);
    }
    refused("working_size(0, 90)", [](FrameSettings s) { return propose_working_size(s, 0, 90); });
    refused("working_size(-1, -1)", [](FrameSettings s) { return propose_working_size(s, -1, -1); });
    refused("frame_mask(stride < width)", [](FrameSettings s) { return propose_frame_mask(s, true, 320, 180, 319); });
    refused("mask_scope(0)", [](FrameSettings s) { return propose_frame_mask_scope(s, 0); });
    refused("mask_scope(4)", [](FrameSettings s) { return propose_frame_mask_scope(s, 4); });
    refused("direct_similarity(1.5)", [](FrameSettings s) { return propose_direct_similarity(s, 1.5f); });
    refused("direct_similarity(nan)", [](FrameSettings s) { return propose_direct_similarity(s, NAN); });
    refused("direct_scope(2)", [](FrameSettings s) { return propose_direct_scope(s, 2); });
    refused("frame_region(out 0x72)", [](FrameSettings s) { return propose_frame_region(s, 320, 180, REGION_M, 0, 72); });
    refused("frame_region(W changes sign)", [](FrameSettings s) {
        const double M[9] = {1, 0, 0, 0, 1, 0, 1, 0, -10};
        return propose_frame_region(s, 320, 180, M, 128, 72);
    });
    if (fails) { std::fprintf(stderr, "%d checks failed\n", fails); return 1; }
    std::printf("frame settings: %d ordered pairs, %d combinations, 10 range refusals: as the tables say\n", N_CALLS * N_CALLS, (int)(sizeof(COMBOS) / sizeof(COMBOS[0])));
    return 0;
}
