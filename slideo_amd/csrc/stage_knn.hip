// stage_knn.hip — index build and the k-NN stage (kernels: knn.hip.h, knn_tile.hip.h, knn_l2.hip.h, knn_lsh.hip.h).
#include "runtime.hpp"
#include "knn.hip.h"
#include "knn_tile.hip.h"
#include "knn_l2.hip.h"
#include "knn_lsh.hip.h"

using namespace slideo;

namespace slideo {

// ---- exact Hamming kNN: keys into S.d_keys[0 .. nq*KLIST) ------------------------------
int knn_operand_rows(int nt) { return cdiv(std::max(nt, 1), KT_ST_ROWS) * KT_ST_ROWS; }
OperandLayout knn_operand_layout() { return OperandLayout{KT_ST_ROWS, KT_SIDE_U32, KT_PAD_NORM}; }

void knn_expand_operand(const uint32_t* t, int nt, int nt_pad, const int32_t* perm, uint4* tx, hipStream_t st) {
    knn_tile_expand_kernel<<<cdiv(nt_pad * 8, 256), 256, 0, st>>>(t, nt, nt_pad, perm, tx);
    check_launch("knn_tile_expand_kernel");
}

// The 32-row TILES of an operand (each of one norm, which is all the fast path needs) are streamed in a fixed pseudo-random order.
// Streaming them in norm order is adversarial for the running thresholds: E[d] = |q| + |t| (1 - |q| / 128), so for every
// query with more than 128 set bits the nearest rows would come LAST, the k-th distance would keep falling along the
// stream and almost every tile would send some lane to the slow path (measured: 17.3 ms against 11.9 ms for the
// +-1 engine on the headline launch).  A shuffled tile order makes the stream i.i.d. again for every query.  The L2 engine alike:
// in norm order a query meets its neighbours — rows of about its own norm — only at its own place in the stream and keeps a loose
// threshold until then.  The order depends on the tile count alone: a page set (stage_page_set.hip) draws the one a deck of its
// pages would.
std::vector<int32_t> knn_tile_order(int ntiles) {
    std::vector<int32_t> order((size_t)ntiles);
    for (int i = 0; i < ntiles; ++i) order[i] = i;
    uint64_t st_ = 0x9E3779B97F4A7C15ull;
    for (int i = ntiles - 1; i > 0; --i) {
        st_ = st_ * 6364136223846793005ull + 1442695040888963407ull;
        std::swap(order[i], order[(int)((st_ >> 33) % (uint64_t)(i + 1))]);
    }
    return order;
}

// The host side of an operand's build: `sorted` (the nt source rows in ascending norm order) put in tile order and padded to
// op.nt_pad (-1: pad rows, which may then sit inside the stream: the partial last tile), the side array per super-tile ([norm |
// row id]) and the per-tile bounds filled, all three uploaded.  enc(source row or -1, bound&): the side word of the row's norm and
// the bound a tile takes from it when the row is the tile's first (ascending order: its smallest norm).  rowid (may be null): the
// row number a key carries for a source row.  expand(): the caller's kernel that gathers op.tx through op.perm.
template <class Enc, class Expand>
static void operand_build(SearchOperand& op, const std::vector<int32_t>& sorted, const int32_t* rowid, Enc enc, Expand expand, hipStream_t st) {
    const int nt = op.nt, nt_pad = op.nt_pad, n_st = nt_pad / KT_ST_ROWS;
    const std::vector<int32_t> order = knn_tile_order(cdiv(nt, 32));
    std::vector<int32_t> perm((size_t)nt_pad, -1);
    for (size_t p = 0; p < order.size(); ++p)
        for (int r = 0; r < 32; ++r) {
            const size_t src = (size_t)order[p] * 32 + r;
            if (src < (size_t)nt) perm[p * 32 + r] = sorted[src];
        }
    std::vector<uint32_t> side((size_t)n_st * KT_SIDE_U32), bound((size_t)n_st * 4);
    for (int r = 0; r < nt_pad; ++r) {
        uint32_t b;
        side[(size_t)(r / KT_ST_ROWS) * KT_SIDE_U32 + (r % KT_ST_ROWS)] = enc(perm[r], b);
        side[(size_t)(r / KT_ST_ROWS) * KT_SIDE_U32 + KT_ST_ROWS + (r % KT_ST_ROWS)] = (uint32_t)(perm[r] >= 0 && rowid ? rowid[perm[r]] : perm[r]);
        if (r % 32 == 0) bound[r / 32] = b;
    }
    HIP_CHECK(hipMemcpyAsync(op.perm.p, perm.data(), perm.size() * 4, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(op.side.p, side.data(), side.size() * 4, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(op.bound.p, bound.data(), bound.size() * 4, hipMemcpyHostToDevice, st));
    expand();
    HIP_CHECK(hipStreamSynchronize(st));                                 // the host vectors die here
}

// Operand of the {0,1} x {0,1} engine (knn_tile.hip.h): rows in ascending popcount order (stable counting sort on the host:
// nt x 32 bytes of popcounts), expanded to tile-major FP4 on the device, plus per super-tile the rows' norms and original
// indices and per tile half its smallest norm; the tiles in the order of knn_tile_order (see there for why).  `t_host`: the packed
// rows in host memory.
// rowid (may be null): the row number a key carries for row i of t_host / t_dev (de-duplicated sets: the lowest original row).
// norm_order (may be null): receives the nt rows' norm order before the tile shuffle (what a page set compacts, stage_page_set.hip)
static void prepare_train_bits(const uint8_t* t_host, const uint32_t* t_dev, int nt, SearchOperand& op, hipStream_t st, const int32_t* rowid = nullptr,
                               std::vector<int32_t>* norm_order = nullptr) {
    std::vector<uint16_t> norm((size_t)std::max(nt, 1));
    uint32_t hist[258] = {0};
    for (int i = 0; i < nt; ++i) {
        uint64_t w[4];
        std::memcpy(w, t_host + (size_t)i * 32, 32);
        const int n = __builtin_popcountll(w[0]) + __builtin_popcountll(w[1]) + __builtin_popcountll(w[2]) + __builtin_popcountll(w[3]);
        norm[i] = (uint16_t)n; hist[n + 1]++;
    }
    for (int i = 0; i < 257; ++i) hist[i + 1] += hist[i];
    std::vector<int32_t> sorted((size_t)nt);
    for (int i = 0; i < nt; ++i) sorted[hist[norm[i]]++] = i;             // stable: ties keep row order
    if (norm_order) *norm_order = sorted;
    op.reserve(nt, knn_operand_rows(nt), knn_operand_layout());
    operand_build(op, sorted, rowid, [&](int32_t row, uint32_t& b) {
        const float nf = row >= 0 ? (float)norm[row] : KT_PAD_NORM, half = 0.5f * nf;
        uint32_t bits; std::memcpy(&bits, &nf, 4); std::memcpy(&b, &half, 4);
        return bits;
    }, [&] { knn_expand_operand(t_dev, nt, op.nt_pad, op.perm.as<int32_t>(), op.tx.as<uint4>(), st); }, st);
}

// slideo_config.matcher 1: the tables of FLANN's LshIndex over `nt` host rows (geom.h lsh_params / lsh_key_host), uploaded
static void build_lsh_set(const slideo_config& c, const uint8_t* t_host, int nt, slideo_matcher::LshSet& S, hipStream_t st) {
    const LshParams P = lsh_params(c);
    const int nb = 1 << P.kb;
    std::vector<uint16_t> keys((size_t)std::max(nt, 1) * P.ntab);
    std::vector<int32_t> ofs((size_t)P.ntab * (nb + 1), 0), rows((size_t)P.ntab * std::max(nt, 1));
    for (int tb = 0; tb < P.ntab; ++tb) {
        int32_t* o = ofs.data() + (size_t)tb * (nb + 1);
        for (int i = 0; i < nt; ++i) { const uint32_t k = lsh_key_host(P, tb, t_host + (size_t)i * 32); keys[(size_t)i * P.ntab + tb] = (uint16_t)k; o[k + 1]++; }
        for (int i = 0; i < nb; ++i) o[i + 1] += o[i];
        std::vector<int32_t> cur(o, o + nb);
        for (int i = 0; i < nt; ++i) rows[(size_t)tb * std::max(nt, 1) + cur[keys[(size_t)i * P.ntab + tb]]++] = i;      // rows ascend inside a bucket
    }
    S.ofs.reserve(ofs.size() * 4 + 16); S.rows.reserve(rows.size() * 4 + 16); S.keys.reserve(keys.size() * 2 + 16);
    HIP_CHECK(hipMemcpyAsync(S.ofs.p, ofs.data(), ofs.size() * 4, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(S.rows.p, rows.data(), rows.size() * 4, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(S.keys.p, keys.data(), keys.size() * 2, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));
    S.dev.p = P; S.dev.nbuckets = nb; S.dev.ofs = S.ofs.as<int32_t>(); S.dev.rows = S.rows.as<int32_t>(); S.dev.keys = S.keys.as<uint16_t>();
    S.dev.M = std::max(nt, 1);
    S.ready = true;
}

// One search block per CU instead of two (knn_tile.hip.h: 2 instead of 4 waves per SIMD) while other units are in flight: two
// blocks hold every register of a CU (4 waves x 128 per SIMD), so the ORB and verify kernels of the other units cannot share
// a CU with them and run in the gaps the search launches leave.  With one block the other half of the registers and 72 KB of
// LDS stay free; the search alone is slower (9.4 instead of 7.9 ms for the headline launch), the step of overlapped units
// is 5 % shorter (profiles/r04_experiments.txt).  The block count is capped through the launch's dynamic LDS size: the
// kernel's own 70 KB + this pad exceed half of the CU's 160 KB.  The exact Hamming search only: the LSH-filtered stream is
// VALU-bound on its row filter and dominates its step (one block per CU: 26.2 instead of 21.4 ms per step), and the SIFT
// matcher's step is its extraction stage (L2 search one or two blocks per CU: 73.3 ms either way).
#ifndef KT_SHARE_PAD_V
#define KT_SHARE_PAD_V (16 * 1024)
#endif
constexpr unsigned KT_SHARE_PAD = KT_SHARE_PAD_V;
static_assert(KT_SHARE_PAD == 0 || KT_RING * (KT_ST_U4 * 16 + KT_SIDE_U32 * 4) + KT_SHARE_PAD > 160 * 1024 / 2, "the pad must push a block past half of the CU's LDS");
#ifdef KT_PROBE
void knn_probe_report() {
    unsigned long long v[8] = {0};
    if (hipMemcpyFromSymbol(v, HIP_SYMBOL(slideo::kt_probe), sizeof(v)) != hipSuccess || !v[6]) return;
    const double w = (double)v[6];
    fprintf(stderr, "KT_PROBE waves %.0f  cycles per wave: total %.0f  vmcnt %.0f  wait_done %.0f  wait_filled %.0f  slow %.0f  flush %.0f\n",
            w, v[0] / w, v[1] / w, v[2] / w, v[3] / w, v[4] / w, v[5] / w);
    fprintf(stderr, "KT_PROBE s_memtime ticks per 100 MHz wall tick: %.3f (x 100 MHz = the shader clock the waves saw, if s_memtime counts it)\n", (double)v[0] / (double)std::max<unsigned long long>(v[7], 1));
    static unsigned int ww[64][8][4];
    if (hipMemcpyFromSymbol(ww, HIP_SYMBOL(slideo::kt_wave), sizeof(ww)) == hipSuccess)
        for (int b = 0; b < 64; b += 7) {
            fprintf(stderr, "KT_WAVE block %3d:", 100 + b);
            for (int k = 0; k < 8; ++k) fprintf(stderr, "  [%u s%u d%u f%u]", ww[b][k][0], ww[b][k][1], ww[b][k][2], ww[b][k][3]);
            fprintf(stderr, "\n");
        }
    unsigned long long z[8] = {0};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(slideo::kt_probe), z, sizeof(z));
}
#endif
static unsigned share_pad(const slideo_matcher* m, bool shared) { return (m->knn_share == 1 || (m->knn_share < 0 && shared)) ? KT_SHARE_PAD : 0u; }
// The block shape of the exact Hamming search (engine 3).  SHAPE_T2: knn_tile2_kernel, 8 waves x 2 query tiles, two blocks per CU or
// — with the LDS pad — one.  SHAPE_T2W12 (by default for LARGE decks while units share the chip — knn_w12_ratio —; SLIDEO_KNN_SHARE=3 / 4 force it):
// the same wave shape, 12 waves, one block per CU by its registers.  Only the exact search (matcher 0): the LSH-filtered stream has
// its own kernel, the 8-wave shape and no LDS pad.
enum KnnShape { SHAPE_T2 = 0, SHAPE_T2W12 = 1 };
static KnnShape knn_shape(const slideo_matcher* m, bool shared, bool w12) {
    if (m->cfg.matcher != 0) return SHAPE_T2;
    if ((m->knn_share == 3 && shared) || m->knn_share == 4) return SHAPE_T2W12;
    if (m->knn_share < 0 && shared && w12) return SHAPE_T2W12;       // large decks (knn_plan_unit)
    return SHAPE_T2;
}
// Engine 0 ("mfma") = the 2-tile wave shape (knn_tile2_kernel: 4 waves/SIMD, two 512-query blocks per CU) at every size: since the
// {0,1} operand alphabet it runs the headline launch in 10.0 ms alone against 11.3 for the 4-tile shape and the step is 2 %
// shorter.  The 4-tile shape (engine 2) and the VALU popcount kernel (engine 1) stay selectable for A/B: identical results.
static int knn_engine_for(const slideo_matcher* m) { return m->knn_engine != 0 ? m->knn_engine : 3; }
bool knn_unit_is_valu(const slideo_matcher* m) { return knn_engine_for(m) == 1; }

// The plan of one search over nt train rows.  shared / w12: what the unit observed (KnnPlan).  nq: the query count the plan is made
// for (the real one, or its estimate when only the device knows it); nq_grid >= nq: what the grid and the buffers are sized for
// (blocks past the device-side count leave at once)
static KnnPlan knn_plan(const slideo_matcher* m, bool shared, bool w12, int nq, int nt, int nq_grid = 0) {
    KnnPlan p{};
    p.shared = shared; p.w12 = w12; p.nt = nt;
    nq = std::max(nq, 1);            // a unit may hold no keypoint at all (e.g. one flat frame)
    p.nq_all = std::max(nq_grid, nq);
    p.engine = nt > 0 ? knn_engine_for(m) : 1;
    p.shape = knn_shape(m, shared, w12);
    p.lds_pad = share_pad(m, shared);
    if (p.engine != 1) {
        const bool t4 = p.engine == 2, w12s = !t4 && p.shape == SHAPE_T2W12;
        const int qpb = t4 ? knn_qpb<4>() : w12s ? knn_qpb<2, KT_WAVES12>() : knn_qpb<2>();
        // the chip holds 512 blocks of the 8-wave 2-tile shape (two per CU); 256 of the 1024-query blocks of the 4-tile shape and of
        // the 12-wave blocks (one per CU whatever else runs).  From 3/4 of that on, one pass over the train set is best (every
        // segment pays its own list warm-up and the merge); fewer query blocks split the train set so that the blocks
        // fill the chip in ONE round (floor, not ceil: 1.4 rounds of smaller blocks lose more to the tail than the
        // empty slots do).  Measured (r01): 236 query blocks x 1.8 M rows (64 4K frames): 1 segment 33.2 ms, 2 segments 24.2 ms,
        // 3 segments 23.5 ms; 239 query blocks x 517 k rows (128 1080p frames): 2 segments 6.24 ms, 3 segments 6.65 ms
        const int slots = t4 || w12s ? 256 : 512;
        p.qblocks = cdiv(nq, qpb);
        const int n_st = knn_operand_rows(nt) / KT_ST_ROWS;
        const int nseg = p.qblocks >= slots * 3 / 4 ? 1 : std::min(std::max(slots / std::max(p.qblocks, 1), 1), n_st);
        p.per_seg = cdiv(n_st, std::max(nseg, 1));
        p.nseg = cdiv(n_st, p.per_seg);
        p.qblocks = cdiv(p.nq_all, qpb);
    } else {
        p.qblocks = cdiv(nq, KNN_BLOCK);
        int nseg = 1;
        if (p.qblocks < 1024) nseg = std::min(cdiv(1024, p.qblocks), std::max(1, nt / 4096));
        p.nseg = std::max(1, std::min(nseg, 256));
        p.per_seg = cdiv(std::max(nt, 1), p.nseg);
        p.qblocks = cdiv(p.nq_all, KNN_BLOCK);
    }
    return p;
}

static void knn_reserve(Slot& S, const KnnPlan& p) {
    S.d_keys.reserve((size_t)p.nseg * p.nq_all * KLIST * 4);
    if (p.engine == 2) S.d_knn_pend.reserve((size_t)p.qblocks * p.nseg * KT_WAVES * knn_pend_words_per_wave<4>() * 4);
    if (p.engine == 3) S.d_knn_pend.reserve((size_t)p.qblocks * p.nseg * (p.shape == SHAPE_T2W12 ? KT_WAVES12 : KT_WAVES) * knn_pend_words_per_wave<2>() * 4);
}

void knn_plan_unit(slideo_matcher* m, Slot& S, int n, int64_t frame_pixels, uint32_t qplan, uint32_t qtot) {
    // (the matrix-core engine searches the unique rows of the train set, the VALU engine — A/B only — all of them; a page set — never
    // under the VALU engine, page_set_check_mode — its own distinct rows)
    const PageSet* ps = page_set_of(m, S.u_set);
    const bool dedup = ps ? ps->urows < ps->rows : (m->Mu < m->M && !knn_unit_is_valu(m));
    const int nt = (int)(ps ? ps->urows : dedup ? m->Mu : m->M);
    // While units share the chip the search runs the 12-wave block (three waves per SIMD, 128 registers each) instead of the 8-wave
    // block + LDS pad when a unit carries at least knn_w12_ratio (query, train row) pairs per frame pixel — how much search there is
    // per pixel of ORB work: the larger the deck, the more of a step is search, and from ~290 pairs per pixel on the fuller matrix
    // pipe is worth more than the co-runners' occupancy (profiles/r06_experiments.txt 7: headline 197: - 2..4 %; 700 pages 275:
    // - 1.7 %; 800 pages 314: + 5.5 %; configs[3] 392: + 6.8 %; configs[4] 352: + 4.7 %).  SLIDEO_KNN_W12_RATIO overrides (0 = never).
    const bool w12 = m->knn_w12_ratio > 0.0 && (double)qplan * (double)nt >= m->knn_w12_ratio * (double)n * (double)frame_pixels;
    S.knn = knn_plan(m, S.knn.shared, w12, (int)qplan, nt, (int)qtot);
    S.knn.dedup = dedup;
    knn_reserve(S, S.knn);
}

// The matrix-core search over `op` as p plans it, then the merge of its segments' lists.  lsh: the LSH-filtered stream's context
// (its own kernel) or null: the exact search in p's engine and block shape.  nq_dev != null: the real query count lives on the
// device (the host did not wait for the ORB counts); then `nq` is the estimate the plan was made for.
static void knn_launch_tiles(slideo_matcher* m, Slot& S, const KnnPlan& p, const uint32_t* q_dev, int nq, const SearchOperand& op, float prune_tol,
                             const uint32_t* nq_dev, const KtLshCtx* lsh = nullptr) {
    hipStream_t st = S.st;
    const dim3 grid(p.qblocks, p.nseg);
    const uint4* tx = op.tx.as<uint4>(); const uint32_t* side = op.side.as<uint32_t>(); const float4* nminh = op.bound.as<float4>();
    const int nt_pad = knn_operand_rows(p.nt);
    uint32_t *keys = S.d_keys.as<uint32_t>(), *pend = S.d_knn_pend.as<uint32_t>();
    unsigned long long* const clk = m->profiling ? m->d_clk.as<unsigned long long>() : nullptr;      // (slideo_matcher_read_shader_clock)
    if (lsh)
        knn_tile2_lsh_kernel<<<grid, KT_THREADS, 0, st>>>(q_dev, nq, tx, side, nminh, nt_pad, p.per_seg, keys, pend, prune_tol, nq_dev, *lsh);
    else if (p.engine == 2)
        knn_tile4_kernel<<<grid, KT_THREADS, 0, st>>>(q_dev, nq, tx, side, nminh, nt_pad, p.per_seg, keys, pend, prune_tol, nq_dev);
    else if (p.shape == SHAPE_T2W12)
        knn_tile2w12_kernel<<<grid, KT_WAVES12 * 64, 0, st>>>(q_dev, nq, tx, side, nminh, nt_pad, p.per_seg, keys, pend, prune_tol, nq_dev, clk);
    else
        knn_tile2_kernel<<<grid, KT_THREADS, p.lds_pad, st>>>(q_dev, nq, tx, side, nminh, nt_pad, p.per_seg, keys, pend, prune_tol, nq_dev, clk);
    check_launch(lsh ? "knn_tile2_lsh_kernel" : "knn_tile_kernel");
    if (p.nseg > 1) {
        knn_merge_kernel<KLIST><<<cdiv(p.nq_all, KNN_BLOCK), KNN_BLOCK, 0, st>>>(keys, nq, p.nseg, nq_dev);
        check_launch("knn_merge_kernel");
    }
}

// The exact search as p plans it (its workspace reserved): q_dev -> S.d_keys.  t: the packed rows (VALU engine), op: their operand
// (matrix-core engines).  prune_tol > 0: only neighbours that can pass the vote's `d < best * tol` need to be exact (matrix-core
// engine; the VALU engine always returns full lists).  nq_dev: see knn_launch_tiles; only the matrix-core engine.
static void run_knn(slideo_matcher* m, Slot& S, const KnnPlan& p, const uint32_t* q_dev, int nq, const uint32_t* t, const SearchOperand& op,
                    float prune_tol, const uint32_t* nq_dev = nullptr) {
    if (nq <= 0 && !nq_dev) return;
    if ((int64_t)p.nt >= ((int64_t)1 << KNN_KEY_SHIFT)) fail(SLIDEO_ERR_UNSUPPORTED, "train set of %d rows exceeds %d", p.nt, 1 << KNN_KEY_SHIFT);
    if (p.engine != 1) { knn_launch_tiles(m, S, p, q_dev, nq, op, prune_tol, nq_dev); return; }
    if (nq_dev) fail(SLIDEO_ERR_STATE, "internal: the VALU kNN engine needs the query count on the host");
    knn_hamming_kernel<KLIST><<<dim3(p.qblocks, p.nseg), KNN_BLOCK, 0, S.st>>>(q_dev, nq, t, p.nt, p.per_seg, S.d_keys.as<uint32_t>());
    check_launch("knn_hamming_kernel");
    if (p.nseg > 1) {
        knn_merge_kernel<KLIST><<<p.qblocks, KNN_BLOCK, 0, S.st>>>(S.d_keys.as<uint32_t>(), nq, p.nseg);
        check_launch("knn_merge_kernel");
    }
}

// A unit's search: S.d_desc (n frames' descriptors, offsets S.d_qofs) -> S.d_keys.  async: the real query count lives on the
// device (S.d_qofs[n]), qplan is what the launch is planned for and qtot the capacity the grid covers.
void unit_knn(slideo_matcher* m, Slot& S, int n, uint32_t qplan, uint32_t qtot, bool async, bool prof) {
    const slideo_config& c = m->cfg;
    hipStream_t st = S.st;
    const KnnPlan& p = S.knn;
    const PageSet* ps = page_set_of(m, S.u_set);            // (the unit's page set: its operand and chain instead of the deck's)
    const SearchOperand& op = ps ? ps->op : m->train_op;
    const uint32_t* nqd = async ? S.d_qofs.as<uint32_t>() + n : nullptr;
    // a neighbour counts iff d < best * vote_tolerance (verify.hip.h vote_kernel); with tolerance < 1 rows below the
    // current best must still be kept, hence max(tol, 1)
    // (the ratio test needs the exact two nearest rows: exact lists)
    const float prune = (m->knn_exact_lists || m->cfg.ratio_test > 0.f) ? 0.f : std::max(m->cfg.vote_tolerance, 1.0f);
    if (c.matcher == 1 && (m->lsh_gather || knn_unit_is_valu(m))) {
        // the reference's index, gathered: only the LSH candidates of a query are scored (knn_lsh.hip.h); same key lists out
        knn_lsh_kernel<KLIST><<<cdiv((int)std::max(qtot, 1u), 4), 256, 0, st>>>(m->lsh.dev, S.d_desc.as<uint32_t>(), (int)qtot, m->d_train.as<uint32_t>(),
                                                                               S.d_keys.as<uint32_t>(), nqd);
        check_launch("knn_lsh_kernel");
    } else if (c.matcher == 1) {
        // the same result from the matrix-core stream over ALL rows with the candidate rule applied where a row passes the
        // distance test (KtHammingLsh): a fifth of all rows are candidates of a query on these descriptors (skewed buckets),
        // so gathering them is 60x slower than streaming everything
        S.d_qkeys.reserve(std::max<size_t>((size_t)qtot * c.lsh_tables * 2, 64));
        lsh_query_keys_kernel<<<cdiv((int)std::max(qtot, 1u), 256), 256, 0, st>>>(m->lsh.dev.p, S.d_desc.as<uint32_t>(), (int)qtot, S.d_qkeys.as<uint16_t>(), nqd);
        check_launch("lsh_query_keys_kernel");
        const KtLshCtx ctx{m->lsh.dev.keys, S.d_qkeys.as<uint16_t>(), c.lsh_tables, c.lsh_multi_probe};
        knn_launch_tiles(m, S, p, S.d_desc.as<uint32_t>(), (int)qplan, op, prune, nqd, &ctx);
    } else
        run_knn(m, S, p, S.d_desc.as<uint32_t>(), (int)qplan, ps ? nullptr : m->d_train.as<uint32_t>(), op, prune, nqd);
    if (prof) HIP_CHECK(hipEventRecord(S.ev[2], st));      // the kNN interval ends here: the search kernel (+ its segment merge)
    if (p.dedup) {
        knn_expand_dups_kernel<KLIST><<<cdiv((int)std::max(qtot, 1u), KNN_BLOCK), KNN_BLOCK, 0, st>>>(
            S.d_keys.as<uint32_t>(), (int)qtot, (ps ? ps->d_grp_next : m->d_grp_next).as<int32_t>(), nqd);
        check_launch("knn_expand_dups_kernel");
    }
}

// FlannMatcher::new (mo/flann.rs:65-71) for the Hamming index over the M packed rows of `train` (page order).
void knn_build_index(slideo_matcher* m, const std::vector<uint8_t>& train, int64_t M) {
    m->d_train.reserve(std::max<size_t>(train.size(), 64) + 64);   // + slack: the kNN loop reads whole rows only, no overrun
    HIP_CHECK(hipMemcpy(m->d_train.p, train.data(), train.size(), hipMemcpyHostToDevice));
    // equal rows: sort the row numbers by descriptor (ties by row), chain each group, keep the lowest row of each
    std::vector<int32_t> order((size_t)M), grp_next((size_t)M, -1), urow;
    for (int64_t i = 0; i < M; ++i) order[i] = (int32_t)i;
    m->Mu = M;
    if (m->cfg.matcher == 1) build_lsh_set(m->cfg, train.data(), (int)M, m->lsh, m->stream);
    if (m->knn_dedup && m->cfg.matcher == 0) {
        const uint64_t* t64 = reinterpret_cast<const uint64_t*>(train.data());
        auto less = [&](int32_t a, int32_t b) {
            const uint64_t* x = t64 + (size_t)a * 4; const uint64_t* y = t64 + (size_t)b * 4;
            for (int j = 0; j < 4; ++j) if (x[j] != y[j]) return x[j] < y[j];
            return a < b;
        };
        std::sort(order.begin(), order.end(), less);
        std::vector<uint8_t> head((size_t)M, 1);
        for (int64_t i = 1; i < M; ++i)
            if (std::memcmp(t64 + (size_t)order[i - 1] * 4, t64 + (size_t)order[i] * 4, 32) == 0) { grp_next[order[i - 1]] = order[i]; head[order[i]] = 0; }
        for (int64_t i = 0; i < M; ++i) if (head[i]) urow.push_back((int32_t)i);
        m->Mu = (int64_t)urow.size();
    }
    m->d_grp_next.reserve(grp_next.size() * 4 + 16);
    HIP_CHECK(hipMemcpy(m->d_grp_next.p, grp_next.data(), grp_next.size() * 4, hipMemcpyHostToDevice));
    if (m->Mu < M) {
        std::vector<uint8_t> utrain((size_t)m->Mu * 32);
        for (int64_t i = 0; i < m->Mu; ++i) std::memcpy(utrain.data() + (size_t)i * 32, train.data() + (size_t)urow[i] * 32, 32);
        m->d_utrain.reserve(utrain.size() + 64);
        HIP_CHECK(hipMemcpy(m->d_utrain.p, utrain.data(), utrain.size(), hipMemcpyHostToDevice));
        prepare_train_bits(utrain.data(), m->d_utrain.as<uint32_t>(), (int)m->Mu, m->train_op, m->stream, urow.data(), &m->h_uorder);
        m->h_urow.swap(urow);                                              // (page sets: distinct row -> its head row)
    } else {
        prepare_train_bits(train.data(), m->d_train.as<uint32_t>(), (int)M, m->train_op, m->stream, nullptr, &m->h_uorder);
        m->h_urow.clear();                                                 // (every row is its own head)
    }
    HIP_CHECK(hipStreamSynchronize(m->stream));
}

// ---- L2 k-NN (cfg2): train set prepared once, queries from device memory ----
void l2_prepare(slideo_matcher::L2Set& L, const uint8_t* t, int nt, hipStream_t st) {
    SearchOperand& op = L.op;
    DevBuf d_t, d_norm;
    d_t.reserve(std::max<size_t>((size_t)nt * 128, 64)); d_norm.reserve(std::max<size_t>((size_t)nt * 4, 64));
    op.reserve(nt, knn_operand_rows(nt), knn_operand_layout(), 0);
    // norms on the device, the norm order on the host (a stable index sort), then the centred tile-major operand gathered in
    // that order, its tiles shuffled (knn_tile_order)
    std::vector<int32_t> h_norm((size_t)std::max(nt, 1)), sorted((size_t)nt);
    if (nt) {
        HIP_CHECK(hipMemcpyAsync(d_t.p, t, (size_t)nt * 128, hipMemcpyHostToDevice, st));
        knl_norms_kernel<<<cdiv(nt, 256), 256, 0, st>>>(d_t.as<uint8_t>(), nt, d_norm.as<int32_t>());
        check_launch("knl_norms_kernel");
        HIP_CHECK(hipMemcpyAsync(h_norm.data(), d_norm.p, (size_t)nt * 4, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        for (int i = 0; i < nt; ++i) sorted[i] = i;
        std::stable_sort(sorted.begin(), sorted.end(), [&](int32_t a, int32_t b) { return h_norm[a] < h_norm[b]; });
    }
    // the side array of the tile engine (knn_tile.hip.h): per super-tile 128 negated norms (as i32) and 128 original rows; and
    // per tile the negated norm of its first row (the tile's bound: rows ascend inside a tile)
    operand_build(op, sorted, nullptr, [&](int32_t row, uint32_t& b) { return b = (uint32_t)(row >= 0 ? -h_norm[row] : -KNL_PAD_NORM); }, [&] {
        knl_expand_train_kernel<<<cdiv(op.nt_pad * 8, 256), 256, 0, st>>>(d_t.as<uint8_t>(), op.nt_pad, op.perm.as<int32_t>(), op.tx.as<uint4>());
        check_launch("knl_expand_train_kernel");
    }, st);                                          // (synchronised: d_t / d_norm go out of scope)
    L.ready = true;
}

// list length of the kernel instance that serves k neighbours (see knn_l2.hip.h)
static int l2_list_len(int k) { return k <= 8 ? 8 : (k <= 16 ? 16 : KLIST); }

template <int KL>
static void launch_knn_l2(int qblocks, hipStream_t st, const uint8_t* q_dev, int nq, const SearchOperand& op, DevBuf* keys, DevBuf* pend, float prune_tol) {
    knn_l2_kernel<KL><<<qblocks, KT_THREADS, 0, st>>>(q_dev, nq, op.tx.as<uint4>(), op.side.as<uint32_t>(), op.bound.as<uint4>(), op.nt_pad,
                                                      keys->as<unsigned long long>(), pend->as<unsigned long long>(), prune_tol);
}

// queries on the device -> idx / dist on the device (m->d_tapidx / d_tapdist); kernel time between two events if asked for
// keys / pend: the list and pending-key buffers of this search — the set's own by default (results then unpacked into
// m->d_tapidx / d_tapdist), a slot's in SIFT matcher mode (the lists are consumed as they are: no unpack)
void l2_query(slideo_matcher* m, slideo_matcher::L2Set& L, const uint8_t* q_dev, int nq, int k, hipStream_t st, Slot& S, bool timed,
              DevBuf* keys, DevBuf* pend, float prune_tol) {
    const int qblocks = cdiv(nq, knn_qpb<2>());
    const bool own = keys == nullptr;
    if (own) { keys = &L.d_keys; pend = &L.d_pend; }
    keys->reserve((size_t)nq * KLIST * 8); pend->reserve((size_t)qblocks * KT_WAVES * knn_pend_words_per_wave<2>() * 8);   // (u64 keys)
    if (own) { m->d_tapidx.reserve((size_t)nq * k * 4); m->d_tapdist.reserve((size_t)nq * k * 4); }
    if (timed) HIP_CHECK(hipEventRecord(S.ev[0], st));
    const int kl = l2_list_len(k);
    switch (kl) {
        case 8: launch_knn_l2<8>(qblocks, st, q_dev, nq, L.op, keys, pend, prune_tol); break;
        case 16: launch_knn_l2<16>(qblocks, st, q_dev, nq, L.op, keys, pend, prune_tol); break;
        default: launch_knn_l2<KLIST>(qblocks, st, q_dev, nq, L.op, keys, pend, prune_tol);
    }
    check_launch("knn_l2_kernel");
    if (own) {
        knl_unpack_kernel<<<cdiv(nq * k, 256), 256, 0, st>>>(keys->as<unsigned long long>(), nq, kl, k, m->d_tapidx.as<int32_t>(), m->d_tapdist.as<uint32_t>());
        check_launch("knl_unpack_kernel");
    }
    if (timed) HIP_CHECK(hipEventRecord(S.ev[1], st));
}

// SIFT matcher mode: the outcome of the vote rule on the L2 lists (u64 keys, kl per query) as neighbour lists in the HAMMING key
// format, so that the vote kernel and everything after it run unchanged (knn_l2.hip.h l2_ratio_keys_kernel / l2_tol_keys_kernel)
void l2_lists_to_keys(slideo_matcher* m, Slot& S, const DevBuf& lists, int kq, uint32_t qtot, bool lowe, hipStream_t st) {
    const int kl = l2_list_len(kq);                                       // (the instance l2_query picked)
    if (lowe)
        l2_ratio_keys_kernel<<<cdiv((int)qtot, 256), 256, 0, st>>>(lists.as<unsigned long long>(), kl, (int)qtot, m->sift_ratio, S.d_keys.as<uint32_t>(), KLIST);
    else
        l2_tol_keys_kernel<<<cdiv((int)qtot, 256), 256, 0, st>>>(lists.as<unsigned long long>(), kl, kq, (int)qtot, m->cfg.vote_tolerance, S.d_keys.as<uint32_t>(), KLIST);
    check_launch("l2 keys kernel");
}

}  // namespace slideo

// The argument rules the k-NN taps share
static void tap_check_args(const void* q, int nq, const void* t, int nt, int k, const void* idx_out, const void* dist_out) {
    if (nq < 0 || nt < 0 || k < 1 || k > KLIST) fail(SLIDEO_ERR_INVALID_ARG, "bad nq/nt/k (k must be 1..%d)", KLIST);
    if ((nq && !q) || (nt && !t) || (nq && (!idx_out || !dist_out))) fail(SLIDEO_ERR_INVALID_ARG, "null argument");
}

// The two taps over 32-byte descriptors, on slot 0: queries and train rows to m->d_tapq / d_tapt (t_slack bytes behind the rows),
// search(S) fills S.d_keys with nq whole key lists, their first k entries unpacked and downloaded.
template <class Search>
static void tap_hamming(slideo_matcher* m, const uint8_t* q, int nq, const uint8_t* t, int nt, int k, int32_t* idx_out, uint16_t* dist_out, size_t t_slack,
                        Search search) {
    HIP_CHECK(hipSetDevice(m->device));
    require_idle(m);
    Slot& S = m->slots[0];
    hipStream_t st = S.st;
    m->d_tapq.reserve((size_t)nq * 32); m->d_tapt.reserve(std::max<size_t>((size_t)nt * 32, 64) + t_slack);
    HIP_CHECK(hipMemcpyAsync(m->d_tapq.p, q, (size_t)nq * 32, hipMemcpyHostToDevice, st));
    if (nt) HIP_CHECK(hipMemcpyAsync(m->d_tapt.p, t, (size_t)nt * 32, hipMemcpyHostToDevice, st));
    search(S);
    m->d_tapidx.reserve((size_t)nq * k * 4); m->d_tapdist.reserve((size_t)nq * k * 2);
    knn_unpack_kernel<<<cdiv(nq * k, 256), 256, 0, st>>>(S.d_keys.as<uint32_t>(), nq, KLIST, k, m->d_tapidx.as<int32_t>(), m->d_tapdist.as<uint16_t>());
    check_launch("knn_unpack_kernel");
    HIP_CHECK(hipMemcpyAsync(idx_out, m->d_tapidx.p, (size_t)nq * k * 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(dist_out, m->d_tapdist.p, (size_t)nq * k * 2, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
}

extern "C" {

int32_t slideo_knn_hamming(slideo_matcher* m, const uint8_t* q, int32_t nq, const uint8_t* t, int32_t nt, int32_t k,
                           int32_t* idx_out, uint16_t* dist_out) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    tap_check_args(q, nq, t, nt, k, idx_out, dist_out);
    if (nq == 0) return SLIDEO_OK;
    SearchOperand tap;                            // (lives until the tap has synchronised)
    tap_hamming(m, q, nq, t, nt, k, idx_out, dist_out, 0, [&](Slot& S) {
        if (!knn_unit_is_valu(m) && nt > 0) prepare_train_bits(t, m->d_tapt.as<uint32_t>(), nt, tap, S.st);
        // (no unit: the block shape follows what slot 0's last unit observed; every shape gives the same lists)
        const KnnPlan p = knn_plan(m, S.knn.shared, S.knn.w12, nq, nt);
        knn_reserve(S, p);
        run_knn(m, S, p, m->d_tapq.as<uint32_t>(), nq, m->d_tapt.as<uint32_t>(), tap, 0.f);
    });
    API_CATCH(m)
}

int32_t slideo_knn_lsh(slideo_matcher* m, const uint8_t* q, int32_t nq, const uint8_t* t, int32_t nt, int32_t k, int32_t* idx_out, uint16_t* dist_out) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    tap_check_args(q, nq, t, nt, k, idx_out, dist_out);
    if ((int64_t)nt >= ((int64_t)1 << KNN_KEY_SHIFT)) fail(SLIDEO_ERR_UNSUPPORTED, "train set of %d rows exceeds %d", nt, 1 << KNN_KEY_SHIFT);
    if (m->cfg.lsh_tables < 1 || m->cfg.lsh_tables > 8 || m->cfg.lsh_key_bits < 1 || m->cfg.lsh_key_bits > 16 || m->cfg.lsh_multi_probe < 0 || m->cfg.lsh_multi_probe > 2)
        fail(SLIDEO_ERR_UNSUPPORTED, "lsh_tables must be 1..8, lsh_key_bits 1..16, lsh_multi_probe 0..2");
    if (nq == 0) return SLIDEO_OK;
    slideo_matcher::LshSet set;                   // (lives until the tap has synchronised)
    tap_hamming(m, q, nq, t, nt, k, idx_out, dist_out, 64, [&](Slot& S) {
        build_lsh_set(m->cfg, t, nt, set, S.st);
        S.d_keys.reserve((size_t)nq * KLIST * 4);
        knn_lsh_kernel<KLIST><<<cdiv(nq, 4), 256, 0, S.st>>>(set.dev, m->d_tapq.as<uint32_t>(), nq, m->d_tapt.as<uint32_t>(), S.d_keys.as<uint32_t>(), nullptr);
        check_launch("knn_lsh_kernel");
    });
    API_CATCH(m)
}

int32_t slideo_l2_set_train(slideo_matcher* m, const uint8_t* t, int32_t nt) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (nt < 0 || (nt && !t)) fail(SLIDEO_ERR_INVALID_ARG, "null train set");
    if (m->sift_on) fail(SLIDEO_ERR_STATE, "the L2 train set is the page DB's in SIFT mode");
    if ((int64_t)nt >= ((int64_t)1 << KNN_KEY_SHIFT)) fail(SLIDEO_ERR_UNSUPPORTED, "train set of %d rows exceeds %d", nt, 1 << KNN_KEY_SHIFT);
    HIP_CHECK(hipSetDevice(m->device));
    require_idle(m);
    l2_prepare(m->l2, t, nt, m->slots[0].st);
    API_CATCH(m)
}

int32_t slideo_l2_knn_dev(slideo_matcher* m, const void* q_dev, int32_t nq, int32_t k, void* idx_dev, void* dist_dev, float* kernel_ms) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (!m->l2.ready) fail(SLIDEO_ERR_STATE, "slideo_l2_set_train must be called first");
    if (nq < 0 || k < 1 || k > KLIST) fail(SLIDEO_ERR_INVALID_ARG, "bad nq/k (k must be 1..%d)", KLIST);
    if (nq && (!q_dev || !idx_dev || !dist_dev)) fail(SLIDEO_ERR_INVALID_ARG, "null argument");
    if (kernel_ms) *kernel_ms = 0.f;
    if (nq == 0) return SLIDEO_OK;
    HIP_CHECK(hipSetDevice(m->device));
    require_idle(m);
    Slot& S = m->slots[0];
    l2_query(m, m->l2, static_cast<const uint8_t*>(q_dev), nq, k, S.st, S, kernel_ms != nullptr);
    HIP_CHECK(hipMemcpyAsync(idx_dev, m->d_tapidx.p, (size_t)nq * k * 4, hipMemcpyDeviceToDevice, S.st));
    HIP_CHECK(hipMemcpyAsync(dist_dev, m->d_tapdist.p, (size_t)nq * k * 4, hipMemcpyDeviceToDevice, S.st));
    HIP_CHECK(hipStreamSynchronize(S.st));
    if (kernel_ms) HIP_CHECK(hipEventElapsedTime(kernel_ms, S.ev[0], S.ev[1]));
    API_CATCH(m)
}

int32_t slideo_knn_l2_u8(slideo_matcher* m, const uint8_t* q, int32_t nq, const uint8_t* t, int32_t nt, int32_t k,
                         int32_t* idx_out, uint32_t* dist_out) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    tap_check_args(q, nq, t, nt, k, idx_out, dist_out);
    if ((int64_t)nt >= ((int64_t)1 << KNN_KEY_SHIFT)) fail(SLIDEO_ERR_UNSUPPORTED, "train set of %d rows exceeds %d", nt, 1 << KNN_KEY_SHIFT);
    if (nq == 0) return SLIDEO_OK;
    HIP_CHECK(hipSetDevice(m->device));
    require_idle(m);
    Slot& S = m->slots[0];
    hipStream_t st = S.st;
    slideo_matcher::L2Set tap;                    // a set of its own: the one installed by slideo_l2_set_train stays as it is
    l2_prepare(tap, t, nt, st);
    DevBuf d_q;
    d_q.reserve((size_t)nq * 128);
    HIP_CHECK(hipMemcpyAsync(d_q.p, q, (size_t)nq * 128, hipMemcpyHostToDevice, st));
    l2_query(m, tap, d_q.as<uint8_t>(), nq, k, st, S, false);
    HIP_CHECK(hipMemcpyAsync(idx_out, m->d_tapidx.p, (size_t)nq * k * 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(dist_out, m->d_tapdist.p, (size_t)nq * k * 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    API_CATCH(m)
}

}  // extern "C"
