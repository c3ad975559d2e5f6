// frame_settings_hostcheck — the rules of csrc/frame_settings.h walked on the host: every ordered pair of the six frame settings,
// each with a value that is in force and a value that is off, from a matcher's defaults; then the refused combinations.  The
// outcome of the second call — accepted or refused, the error code, what it ends — is asserted against the literal tables below,
// which are written from include/slideo_amd.h ("Working size", "Frame region", "Frame mask", "Frame mask scope", "Direct page
// look-up", "Direct look-up scope"), not from the code under test.  tests/test_gpu_frame_settings.py holds the same pair table.
// Then the frame lens ("Frame lens"), which commits under the region's row: its ranges, the off value, the reach rule with and
// without a region, and lens x region x working size in both orders (frame_lens_rules; tests/test_frame_lens_abi.py runs it).
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

// ---- the frame lens ("Frame lens"): its range rules, the off value, the reach rule and the rules between lens, region and working
// size, in both orders.  The lens commits under the region's row (SET_FRAME_REGION: it ends K and G).  The expected codes are
// written from the header: 320x180 frames, c the image centre, f half the diagonal, so r2 = 1 at the source's corners.
int lens_checks = 0;
const double LCX = 159.5, LCY = 89.5, LF = 183.575597506858;          // 0.5 * hypot(320, 180)

int set_lens(FrameSettings& s, int w, int h, double cx, double cy, double f, double k1, double k2) {
    try {
        FrameSettings next = propose_frame_lens(s, w, h, cx, cy, f, k1, k2);
        frame_settings_rules(next, SET_FRAME_REGION, false);
        s = next;
        return 0;
    } catch (const Error& e) { return e.code; }
}
int set_region(FrameSettings& s, int w, int h, const double* M, int ow, int oh) {
    try {
        FrameSettings next = propose_frame_region(s, w, h, M, ow, oh);
        frame_settings_rules(next, SET_FRAME_REGION, false);
        s = next;
        return 0;
    } catch (const Error& e) { return e.code; }
}
int set_ws(FrameSettings& s, int w, int h) {
    try {
        FrameSettings next = propose_working_size(s, w, h);
        frame_settings_rules(next, SET_WORKING_SIZE, false);
        s = next;
        return 0;
    } catch (const Error& e) { return e.code; }
}
void lens_expect(bool ok, const char* what) {
    ++lens_checks;
    if (ok) return;
    ++fails;
    std::fprintf(stderr, "FAIL frame lens: %s\n", what);
}

void frame_lens_rules() {
    const int BAD = SLIDEO_ERR_INVALID_ARG, UNS = SLIDEO_ERR_UNSUPPORTED;
    {   // range rules: nothing changes
        FrameSettings s;
        lens_expect(set_lens(s, 0, 180, LCX, LCY, LF, -0.1, 0) == BAD, "source width 0");
        lens_expect(set_lens(s, 320, 4097, LCX, LCY, LF, -0.1, 0) == BAD, "source height 4097");
        lens_expect(set_lens(s, 320, 180, NAN, LCY, LF, -0.1, 0) == BAD, "cx nan");
        lens_expect(set_lens(s, 320, 180, LCX, INFINITY, LF, -0.1, 0) == BAD, "cy inf");
        lens_expect(set_lens(s, 320, 180, LCX, LCY, NAN, -0.1, 0) == BAD, "f nan");
        lens_expect(set_lens(s, 320, 180, LCX, LCY, LF, NAN, 0) == BAD, "k1 nan");
        lens_expect(set_lens(s, 320, 180, LCX, LCY, LF, -0.1, INFINITY) == BAD, "k2 inf");
        lens_expect(set_lens(s, 320, 180, LCX, LCY, 0.0, -0.1, 0) == BAD, "f 0");
        lens_expect(set_lens(s, 320, 180, LCX, LCY, -5.0, -0.1, 0) == BAD, "f negative");
        lens_expect(!s.lens.set, "a refused lens is not set");
    }
    {   // k1 == k2 == 0 is off, and the other arguments are not looked at
        FrameSettings s;
        lens_expect(set_lens(s, 320, 180, LCX, LCY, LF, -0.1, 0.02) == 0 && s.lens.set && s.lens.k2 == 0.02 && s.lens.q == 1.0 / (LF * LF), "a lens is set");
        lens_expect(set_lens(s, 0, -7, NAN, NAN, -1.0, 0.0, 0.0) == 0 && !s.lens.set && s.lens.src_w == 0, "k = 0 is off whatever else is given");
        lens_expect(set_lens(s, 320, 180, LCX, LCY, LF, -0.0, 0.0) == 0 && !s.lens.set, "k = -0 is off");
    }
    {   // the reach rule without a region: R2 = 1 at the source's corners (to rounding: the values below keep clear of the edge)
        FrameSettings s;
        lens_expect(set_lens(s, 320, 180, LCX, LCY, LF, -0.3, 0) == 0, "1 - 0.9 > 0 at the corner");
        lens_expect(set_lens(s, 320, 180, LCX, LCY, LF, -0.34, 0) == BAD && s.lens.k1 == -0.3, "1 - 1.02 < 0 at the corner; the lens before stays");
        lens_expect(set_lens(s, 320, 180, LCX, LCY, LF, 0.5, 0) == 0, "a pincushion k1 is increasing everywhere");
        lens_expect(set_lens(s, 320, 180, LCX, LCY, LF, -0.3, 0.12) == 0, "k1 -0.3 with k2 0.12: 0.6625 at the vertex 0.75, 0.7 at the corner");
        lens_expect(set_lens(s, 320, 180, LCX, LCY, LF, -1.5, 1.0) == BAD, "k1 -1.5 with k2 1: 1.5 at the corner but -0.0125 at the vertex 0.45");
        lens_expect(set_lens(s, 320, 180, LCX, LCY, LF, 0.2, -0.5) == BAD, "a negative k2 turns the map back before the corner: 1 + 0.6 - 2.5");
        lens_expect(set_lens(s, 320, 180, LCX, LCY, 2.0 * LF, -1.2, 0) == 0, "the same frame under f twice as large reaches r2 = 0.25 only: 1 - 0.9");
        lens_expect(set_lens(s, 320, 180, 0.0, 0.0, LF, -0.1, 0) == BAD, "an off-centre lens reaches r2 = 3.98 at the far corner: 1 - 1.19");
    }
    {   // the reach is the region's in force: whichever of the two set calls enlarges it beyond the rule is refused
        const double IN[9] = {2.5, 0, 0, 0, 2.5, 0, 0, 0, 1};                 // the 128x72 output over (0, 0) .. (317.5, 177.5): inside the source
        const double OUT[9] = {3.75, 0, -80, 0, 3.75, -45, 0, 0, 1};          // ... over (-80, -45) .. (396.25, 221.25): r2 = 2.24 at the corner
        FrameSettings s;
        lens_expect(set_lens(s, 320, 180, LCX, LCY, LF, -0.3, 0) == 0 && set_region(s, 320, 180, IN, 128, 72) == 0, "a region inside the source");
        lens_expect(set_region(s, 320, 180, OUT, 128, 72) == BAD && s.region.M[0] == 2.5, "a region whose quad reaches r2 = 2.24 under k1 -0.3; the region before stays");
        lens_expect(set_lens(s, 320, 180, LCX, LCY, LF, 0, 0) == 0 && set_region(s, 320, 180, OUT, 128, 72) == 0, "the same region without a lens");
        lens_expect(set_lens(s, 320, 180, LCX, LCY, LF, -0.3, 0) == BAD && !s.lens.set, "the lens second: refused, no lens");
        lens_expect(set_lens(s, 320, 180, LCX, LCY, LF, -0.1, 0) == 0, "k1 -0.1 holds over r2 = 2.24: 1 - 0.67");
        const double SMALL[9] = {0.5, 0, 120, 0, 0.5, 60, 0, 0, 1};           // a patch around the centre: the reach shrinks
        lens_expect(set_region(s, 320, 180, SMALL, 128, 72) == 0 && set_lens(s, 320, 180, LCX, LCY, LF, -3.0, 0) == 0, "a small reach admits a strong k1");
        lens_expect(set_region(s, 0, 0, nullptr, 0, 0) == BAD && s.region.set, "clearing the region widens the reach to the source's corners: refused");
    }
    {   // a lens and a region describe the same frames
        const double IN[9] = {2.5, 0, 0, 0, 2.5, 0, 0, 0, 1};
        FrameSettings s;
        lens_expect(set_region(s, 320, 180, IN, 128, 72) == 0 && set_lens(s, 640, 360, 319.5, 179.5, 2.0 * LF, -0.1, 0) == UNS && !s.lens.set, "region, then a lens of another size");
        FrameSettings t;
        lens_expect(set_lens(t, 640, 360, 319.5, 179.5, 2.0 * LF, -0.1, 0) == 0 && set_region(t, 320, 180, IN, 128, 72) == UNS && !t.region.set, "lens, then a region of another size");
    }
    {   // a lens without a region is a rectifying call of its source size: it fits the working size; with a region the region's output does
        const double IN[9] = {2.5, 0, 0, 0, 2.5, 0, 0, 0, 1};
        FrameSettings s;
        lens_expect(set_lens(s, 320, 180, LCX, LCY, LF, -0.1, 0) == 0 && set_ws(s, 160, 90) == UNS && s.work_w == 0, "lens, then a smaller working size");
        lens_expect(set_ws(s, 320, 180) == 0, "a working size that holds the lens's source");
        FrameSettings t;
        lens_expect(set_ws(t, 160, 90) == 0 && set_lens(t, 320, 180, LCX, LCY, LF, -0.1, 0) == UNS && !t.lens.set, "working size, then a larger lens");
        lens_expect(set_region(t, 320, 180, IN, 128, 72) == 0 && set_lens(t, 320, 180, LCX, LCY, LF, -0.1, 0) == 0, "beside a region the region's output is what fits");
        lens_expect(set_region(t, 0, 0, nullptr, 0, 0) == UNS && t.region.set, "clearing that region leaves a lens larger than the working size: refused");
    }
    lens_expect(SETTING_ENDS[SET_FRAME_REGION].kept && SETTING_ENDS[SET_FRAME_REGION].gate && !SETTING_ENDS[SET_FRAME_REGION].map_gen, "the lens's row ends K and G");
}

}  // namespace

int main() {
    frame_lens_rules();
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
    std::printf("frame lens: %d rule checks\n", lens_checks);
    return 0;
}
