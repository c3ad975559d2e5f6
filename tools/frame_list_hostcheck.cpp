// frame_list_hostcheck — the per-thread body of csrc/frame_list.hip.h (frame_gather_thread, compiled for the host) run lane by lane over
// the whole launch grid, and the host planning function of csrc/frame_settings.h that goes with "Frame lists" (frame_list_plan: the
// rules and the staged layout), for tests/test_frame_list_abi.py.
//   g++ -O1 -g -std=c++17 [-fsanitize=address,undefined] -I include -I slideo_amd/csrc tools/frame_list_hostcheck.cpp -o hostcheck
//   hostcheck matrix
//       walks the matrix: every sampling at every depth it has, planar / interleaved in both orders / the four packed orders, BGR8,
//       BGRA8 and planar RGB through the BGR door; 18x10 and 66x34 (plus 17x9 for 4:4:4 and the BGR forms); plane base offsets 0, 1,
//       2, 4, 8, 16; strides tight and row bytes + 2; one frame and two.  Every source plane is its own heap block that starts
//       `offset` bytes in front of the plane and ends with the plane's last byte; the destination is exact-size too: a load or store
//       past either end is the sanitizer's to report, and so is a wide load at an address that is not a multiple of its size.  The
//       gathered frames are compared byte for byte with a restatement by sample address (include/slideo_amd.h "Frame lists").
//       Per case one line:  "case <door> <sampling> <depth> <form> <w> <h> <offset> <pad> <n> ok <y_stride> <uv_stride> <u_offset>
//       <v_offset> <uv_step> <frame_bytes> <stride>"  or  "case ... refused <code> <message>" (an odd address in a 16-bit container);
//       then "paths <rows16> <rows4> <rows1> <heads> <tails>".  Exit status 1 on the first mismatch.
//   hostcheck rules
//       every rule of the list, one refused record each: "<name> <code> <message>", and behind each "state same": the plan of the
//       accepted record before is what it was.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "frame_settings.h"
#include "frame_list.hip.h"

using namespace slideo;

namespace {

struct Block {                       // a plane in its own allocation: `ofs` bytes in, ending with the block
    uint8_t* base = nullptr;
    uint8_t* p = nullptr;
    Block(size_t ofs, size_t bytes) {
        base = static_cast<uint8_t*>(std::malloc(ofs + bytes));
        if (!base || (uintptr_t)base % 16 != 0) { std::fprintf(stderr, "malloc\n"); std::exit(2); }
        p = base + ofs;
    }
    Block(const Block&) = delete;
    Block(Block&& o) noexcept : base(o.base), p(o.p) { o.base = o.p = nullptr; }
    ~Block() { std::free(base); }
};

uint32_t rng_state = 12345u;
uint8_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return (uint8_t)(rng_state >> 24); }

void run_grid(const GatherArgs& a, int n, GatherTally* tally) {
    const int gx = frame_gather_chunks(a);
    for (int z = 0; z < n; ++z)
        for (int j = 0; j < a.n_planes; ++j)
            for (int bx = 0; bx < gx; ++bx)
                for (int ty = 0; ty < GATHER_TY; ++ty)
                    for (int tx = 0; tx < GATHER_TX; ++tx) frame_gather_thread(a, bx, j, z, tx, ty, tally);
}

const char* const SAMPLINGS[4] = {"420", "422", "444", "422_packed"};
const char* const DEPTHS[3] = {"8", "10_msb", "10_lsb"};

// form: YUV door 0 planar, 1 interleaved U V, 2 interleaved V U, 3..6 packed YUY2, YVYU, UYVY, VYUY; BGR door: the pixel format
struct Case { int door, sampling, depth, form, w, h, ofs, pad, n; };

// One case: the planes, the record, the plan, the gather, the restatement.  false: a mismatch
bool run_case(const Case& c, GatherTally* tally) {
    YuvDesc yuv;
    yuv.sampling = c.sampling; yuv.depth = c.depth;
    const int bps = c.door == SLIDEO_FRAME_LIST_YUV ? yuv.bytes_per_sample() : 1;
    const int w = c.w, h = c.h;
    // what the caller has: per address slot k its row bytes and rows (0: the slot is not a plane of its own)
    int64_t rb[3] = {0, 0, 0};
    int rows[3] = {0, 0, 0};
    int uv_step = 0, pixel_format = SLIDEO_PIXEL_BGR8;
    static const int PAIRS[4][2] = {{1, 3}, {3, 1}, {0, 2}, {2, 0}};
    if (c.door == SLIDEO_FRAME_LIST_YUV) {
        const int cw = c.sampling == SLIDEO_YUV_SAMPLING_444 ? w : w / 2, ch = c.sampling == SLIDEO_YUV_SAMPLING_420 ? h / 2 : h;
        if (c.form >= 3) { uv_step = 4; rb[0] = 2 * w; rows[0] = h; }
        else {
            uv_step = c.form == 0 ? 1 : 2;
            rb[0] = (int64_t)bps * w; rows[0] = h;
            rb[1] = (int64_t)bps * cw * uv_step; rows[1] = ch;
            if (c.form == 0) { rb[2] = rb[1]; rows[2] = ch; }
        }
    } else {
        pixel_format = c.form;
        int bpp = 0, planes = 0;
        pixel_format_info(pixel_format, &bpp, &planes);
        for (int k = 0; k < planes; ++k) { rb[k] = (int64_t)bpp * w; rows[k] = h; }
    }
    std::vector<Block> blocks;
    std::vector<const void*> addr((size_t)c.n * 3, nullptr);
    int64_t stride[3] = {0, 0, 0};
    for (int k = 0; k < 3; ++k) stride[k] = rb[k] ? rb[k] + c.pad : 0;
    for (int i = 0; i < c.n; ++i)
        for (int k = 0; k < 3; ++k) {
            if (!rb[k]) continue;
            const size_t bytes = (size_t)(stride[k] * (rows[k] - 1) + rb[k]);
            blocks.emplace_back((size_t)c.ofs, bytes);
            for (size_t b = 0; b < bytes; ++b) blocks.back().p[b] = rnd();
            addr[(size_t)i * 3 + k] = blocks.back().p;
        }
    if (c.door == SLIDEO_FRAME_LIST_YUV && c.form >= 1)
        for (int i = 0; i < c.n; ++i) {
            const uint8_t* a0 = static_cast<const uint8_t*>(addr[(size_t)i * 3]);
            const uint8_t* a1 = static_cast<const uint8_t*>(addr[(size_t)i * 3 + 1]);
            if (c.form >= 3) { addr[(size_t)i * 3 + 1] = a0 + PAIRS[c.form - 3][0]; addr[(size_t)i * 3 + 2] = a0 + PAIRS[c.form - 3][1]; }
            else { addr[(size_t)i * 3 + 1] = a1 + (c.form == 2 ? bps : 0); addr[(size_t)i * 3 + 2] = a1 + (c.form == 1 ? bps : 0); }
        }
    if (c.door == SLIDEO_FRAME_LIST_YUV && c.form >= 1) stride[2] = stride[1] = c.form >= 3 ? stride[0] : stride[1];
    slideo_frame_list L{};
    L.door = c.door; L.on_device = 0; L.n_frames = c.n; L.width = w; L.height = h; L.uv_step = uv_step;
    for (int k = 0; k < 3; ++k) L.stride[k] = stride[k];
    L.planes = addr.data();
    std::printf("case %s %s %s %d %d %d %d %d %d ", c.door ? "yuv" : "bgr", SAMPLINGS[c.sampling], DEPTHS[c.depth], c.form, w, h, c.ofs, c.pad, c.n);
    FrameListPlan P;
    try { P = frame_list_plan(&L, yuv, pixel_format); }
    catch (const Error& e) { std::printf("refused %d %s\n", e.code, e.what()); return true; }
    const size_t total = (size_t)P.frame_bytes * c.n;
    Block dst(0, total);
    std::memset(dst.p, 0xA5, total);
    const GatherArgs a = frame_gather_args(P, reinterpret_cast<const uint8_t* const*>(addr.data()), dst.p);
    run_grid(a, c.n, tally);
    // the restatement, by sample address
    std::vector<uint8_t> want(total, 0xA5);
    for (int i = 0; i < c.n; ++i) {
        uint8_t* f = want.data() + (size_t)P.frame_bytes * i;
        const uint8_t* p0 = static_cast<const uint8_t*>(addr[(size_t)i * 3]);
        const uint8_t* p1 = static_cast<const uint8_t*>(addr[(size_t)i * 3 + 1]);
        const uint8_t* p2 = static_cast<const uint8_t*>(addr[(size_t)i * 3 + 2]);
        if (c.door == SLIDEO_FRAME_LIST_BGR) {
            const uint8_t* pl[3] = {p0, p1, p2};
            for (int k = 0; k < P.n_planes; ++k)
                for (int y = 0; y < h; ++y)
                    for (int64_t x = 0; x < rb[k]; ++x) f[((int64_t)k * h + y) * P.stride + x] = pl[k][y * L.stride[k] + x];
            continue;
        }
        const slideo_yuv420_layout& T = P.yuv;
        if (c.form >= 3) {                               // packed: Y (x, y) at 2x + (1 where chroma is first); U, V of pair cx at 4cx + offset
            const int yo = (T.u_offset & 1) ? 0 : 1;
            for (int y = 0; y < h; ++y) {
                for (int x = 0; x < w; ++x) f[(int64_t)y * T.y_stride + 2 * x + yo] = p0[y * L.stride[0] + 2 * x + yo];
                for (int cx = 0; cx < w / 2; ++cx) {
                    f[(int64_t)y * T.uv_stride + 4 * cx + T.u_offset] = p1[y * L.stride[1] + 4 * cx];
                    f[(int64_t)y * T.uv_stride + 4 * cx + T.v_offset] = p2[y * L.stride[2] + 4 * cx];
                }
            }
            continue;
        }
        const int cw = c.sampling == SLIDEO_YUV_SAMPLING_444 ? w : w / 2, ch = c.sampling == SLIDEO_YUV_SAMPLING_420 ? h / 2 : h;
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x)
                for (int b = 0; b < bps; ++b) f[(int64_t)y * T.y_stride + x * bps + b] = p0[y * L.stride[0] + x * bps + b];
        for (int cy = 0; cy < ch; ++cy)
            for (int cx = 0; cx < cw; ++cx)
                for (int b = 0; b < bps; ++b) {
                    f[T.u_offset + (int64_t)cy * T.uv_stride + cx * uv_step * bps + b] = p1[cy * L.stride[1] + cx * uv_step * bps + b];
                    f[T.v_offset + (int64_t)cy * T.uv_stride + cx * uv_step * bps + b] = p2[cy * L.stride[2] + cx * uv_step * bps + b];
                }
    }
    for (size_t b = 0; b < total; ++b)
        if (want[b] != dst.p[b]) { std::printf("MISMATCH at byte %zu: got %u, want %u\n", b, dst.p[b], want[b]); return false; }
    std::printf("ok %d %d %lld %lld %d %lld %d\n", P.yuv.y_stride, P.yuv.uv_stride, (long long)P.yuv.u_offset, (long long)P.yuv.v_offset, P.yuv.uv_step,
                (long long)P.frame_bytes, P.stride);
    return true;
}

int matrix() {
    GatherTally tally;
    static const int OFS[6] = {0, 1, 2, 4, 8, 16};
    static const int SIZES[3][2] = {{18, 10}, {66, 34}, {17, 9}};
    std::vector<Case> forms;
    for (int s = 0; s < 3; ++s)
        for (int d = 0; d < 3; ++d)
            for (int f = 0; f < 3; ++f) forms.push_back(Case{SLIDEO_FRAME_LIST_YUV, s, d, f, 0, 0, 0, 0, 0});
    for (int f = 3; f < 7; ++f) forms.push_back(Case{SLIDEO_FRAME_LIST_YUV, SLIDEO_YUV_SAMPLING_422_PACKED, 0, f, 0, 0, 0, 0, 0});
    for (int f : {SLIDEO_PIXEL_BGR8, SLIDEO_PIXEL_BGRA8, SLIDEO_PIXEL_PLANAR_RGB8}) forms.push_back(Case{SLIDEO_FRAME_LIST_BGR, 0, 0, f, 0, 0, 0, 0, 0});
    for (Case c : forms)
        for (int sz = 0; sz < 3; ++sz) {
            if (sz == 2 && !(c.door == SLIDEO_FRAME_LIST_BGR || c.sampling == SLIDEO_YUV_SAMPLING_444)) continue;
            for (int o : OFS)
                for (int pad : {0, 2})
                    for (int n : {1, 2}) {
                        c.w = SIZES[sz][0]; c.h = SIZES[sz][1]; c.ofs = o; c.pad = pad; c.n = n;
                        if (!run_case(c, &tally)) return 1;
                    }
        }
    std::printf("paths %llu %llu %llu %llu %llu\n", tally.rows16, tally.rows4, tally.rows1, tally.heads, tally.tails);
    return 0;
}

bool same_plan(const FrameListPlan& a, const FrameListPlan& b) {
    bool same = a.yuv_door == b.yuv_door && a.n_planes == b.n_planes && a.frame_bytes == b.frame_bytes && a.stride == b.stride &&
                std::memcmp(&a.yuv, &b.yuv, sizeof(a.yuv)) == 0;
    for (int j = 0; j < 3; ++j)
        same = same && a.k[j] == b.k[j] && a.rows[j] == b.rows[j] && a.row_bytes[j] == b.row_bytes[j] && a.src_stride[j] == b.src_stride[j] &&
               a.dst_ofs[j] == b.dst_ofs[j];
    return same;
}

// One refused record per rule, derived from an accepted one: 4:2:0 planar (I), interleaved (N), packed (K) and the BGR door's packed
// (B) and planar (R) forms, two frames of 18x10 each, out of one arena (the addresses are checked, never read)
int rules() {
    alignas(16) static uint8_t arena[1 << 16];
    struct Rule { const char* name; char base; int depth; void (*edit)(slideo_frame_list&, const void**); };
    static const Rule RULES[] = {
        {"null_array", 'I', 0, [](slideo_frame_list& L, const void**) { L.planes = nullptr; }},
        {"needed_plane_null", 'I', 0, [](slideo_frame_list&, const void** a) { a[4] = nullptr; }},
        {"needed_plane_null_bgr", 'B', 0, [](slideo_frame_list&, const void** a) { a[3] = nullptr; }},
        {"unneeded_plane_set", 'B', 0, [](slideo_frame_list&, const void** a) { a[1] = arena + 64; }},
        {"door", 'I', 0, [](slideo_frame_list& L, const void**) { L.door = 2; }},
        {"on_device", 'I', 0, [](slideo_frame_list& L, const void**) { L.on_device = 2; }},
        {"n_frames_negative", 'I', 0, [](slideo_frame_list& L, const void**) { L.n_frames = -1; }},
        {"stride_small_y", 'I', 0, [](slideo_frame_list& L, const void**) { L.stride[0] = 17; }},
        {"stride_small_c", 'I', 0, [](slideo_frame_list& L, const void**) { L.stride[2] = 8; }},
        {"stride_small_bgr", 'B', 0, [](slideo_frame_list& L, const void**) { L.stride[0] = 53; }},
        {"stride_negative", 'I', 0, [](slideo_frame_list& L, const void**) { L.stride[0] = -18; }},
        {"odd_address_16bit", 'I', 1, [](slideo_frame_list&, const void** a) { a[1] = static_cast<const uint8_t*>(a[1]) + 1; }},
        {"odd_stride_16bit", 'I', 1, [](slideo_frame_list& L, const void**) { L.stride[0] = 37; }},
        {"interleaved_distance", 'N', 0, [](slideo_frame_list&, const void** a) { a[2] = static_cast<const uint8_t*>(a[1]) + 2; }},
        {"interleaved_distance_16bit", 'N', 1, [](slideo_frame_list&, const void** a) { a[2] = static_cast<const uint8_t*>(a[1]) + 4; }},
        {"interleaved_order_differs", 'N', 0, [](slideo_frame_list&, const void** a) { a[4] = static_cast<const uint8_t*>(a[4]) + 1; a[5] = static_cast<const uint8_t*>(a[4]) - 1; }},
        {"interleaved_strides", 'N', 0, [](slideo_frame_list& L, const void**) { L.stride[2] = L.stride[1] + 2; }},
        {"packed_pair", 'K', 0, [](slideo_frame_list&, const void** a) { a[1] = static_cast<const uint8_t*>(a[0]) + 1; a[2] = static_cast<const uint8_t*>(a[0]) + 2; }},
        {"packed_pair_differs", 'K', 0, [](slideo_frame_list&, const void** a) { a[4] = static_cast<const uint8_t*>(a[3]) + 3; a[5] = static_cast<const uint8_t*>(a[3]) + 1; }},
        {"packed_strides", 'K', 0, [](slideo_frame_list& L, const void**) { L.stride[1] = L.stride[0] + 2; L.stride[2] = L.stride[0] + 2; }},
        {"uv_step", 'I', 0, [](slideo_frame_list& L, const void**) { L.uv_step = 4; }},
        {"uv_step_packed", 'K', 0, [](slideo_frame_list& L, const void**) { L.uv_step = 2; }},
        {"size_odd_420", 'I', 0, [](slideo_frame_list& L, const void**) { L.height = 9; }},
        {"size_odd_width_packed", 'K', 0, [](slideo_frame_list& L, const void**) { L.width = 17; }},
        {"size_limit", 'I', 0, [](slideo_frame_list& L, const void**) { L.width = 2 * MAX_DIM; L.stride[0] = 2 * MAX_DIM; L.stride[1] = L.stride[2] = MAX_DIM; }},
        {"size_zero_bgr", 'B', 0, [](slideo_frame_list& L, const void**) { L.width = 0; }},
        {"planar_rgb_plane_null", 'R', 0, [](slideo_frame_list&, const void** a) { a[2] = nullptr; }},
    };
    try { (void)frame_list_plan(nullptr, YuvDesc{}, SLIDEO_PIXEL_BGR8); std::printf("null_record 0 accepted\n"); }
    catch (const Error& e) { std::printf("null_record %d %s\n", e.code, e.what()); }
    for (const Rule& r : RULES) {
        YuvDesc yuv;
        yuv.depth = r.depth;
        const int bps = yuv.bytes_per_sample(), w = 18, h = 10;
        int pixel_format = SLIDEO_PIXEL_BGR8;
        const void* addr[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        slideo_frame_list L{};
        L.n_frames = 2; L.width = w; L.height = h; L.planes = addr;
        for (int i = 0; i < 2; ++i) {
            const uint8_t* f = arena + 4096 * i;
            if (r.base == 'I') { addr[3 * i] = f; addr[3 * i + 1] = f + 1024; addr[3 * i + 2] = f + 2048; }
            else if (r.base == 'N') { addr[3 * i] = f; addr[3 * i + 1] = f + 1024; addr[3 * i + 2] = f + 1024 + bps; }
            else if (r.base == 'K') { addr[3 * i] = f; addr[3 * i + 1] = f + 1; addr[3 * i + 2] = f + 3; }
            else if (r.base == 'B') addr[3 * i] = f;
            else { addr[3 * i] = f; addr[3 * i + 1] = f + 1024; addr[3 * i + 2] = f + 2048; }
        }
        if (r.base == 'I') { L.door = 1; L.uv_step = 1; L.stride[0] = bps * w; L.stride[1] = L.stride[2] = bps * w / 2; }
        else if (r.base == 'N') { L.door = 1; L.uv_step = 2; L.stride[0] = L.stride[1] = L.stride[2] = bps * w; }
        else if (r.base == 'K') { L.door = 1; L.uv_step = 4; L.stride[0] = L.stride[1] = L.stride[2] = 2 * w; yuv.sampling = SLIDEO_YUV_SAMPLING_422_PACKED; }
        else if (r.base == 'B') { L.door = 0; L.stride[0] = 3 * w; }
        else { L.door = 0; pixel_format = SLIDEO_PIXEL_PLANAR_RGB8; L.stride[0] = L.stride[1] = L.stride[2] = w; }
        FrameListPlan before;
        try { before = frame_list_plan(&L, yuv, pixel_format); }
        catch (const Error& e) { std::printf("%s BASE-REFUSED %d %s\n", r.name, e.code, e.what()); return 1; }
        slideo_frame_list bad = L;
        const void* bad_addr[6];
        std::memcpy(bad_addr, addr, sizeof(addr));
        bad.planes = bad_addr;
        r.edit(bad, bad_addr);
        try { (void)frame_list_plan(&bad, yuv, pixel_format); std::printf("%s 0 accepted\n", r.name); }
        catch (const Error& e) { std::printf("%s %d %s\n", r.name, e.code, e.what()); }
        const FrameListPlan after = frame_list_plan(&L, yuv, pixel_format);
        std::printf("state %s\n", same_plan(before, after) ? "same" : "CHANGED");
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "matrix") return matrix();
    if (cmd == "rules") return rules();
    std::fprintf(stderr, "usage: frame_list_hostcheck matrix | rules\n");
    return 2;
}
