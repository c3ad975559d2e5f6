// stage_page_set.hip — page sets (include/slideo_amd.h "Page sets"): the search operand of a subset of the finalized deck's pages,
// built on the device from the deck's distinct rows (kernels: page_set.hip.h), and the calls that create, select and release one.
#include "runtime.hpp"
#include "page_set.hip.h"

using namespace slideo;

namespace slideo {

const PageSet* page_set_of(const slideo_matcher* m, int set) {
    if (set == 0) return nullptr;
    const auto it = m->page_sets.find(set);
    if (it == m->page_sets.end()) fail(SLIDEO_ERR_STATE, "internal: page set %d is not live", set);
    return it->second.get();
}

void page_set_check_mode(const slideo_matcher* m) {
    if (m->sift_on) fail(SLIDEO_ERR_UNSUPPORTED, "page sets cover the exact Hamming search only: not in SIFT mode (slideo_matcher_use_sift)");
    if (m->cfg.matcher != 0) fail(SLIDEO_ERR_UNSUPPORTED, "page sets cover the exact Hamming search only: not with matcher %d (LSH)", m->cfg.matcher);
    if (m->knn_engine == 1) fail(SLIDEO_ERR_UNSUPPORTED, "page sets cover the matrix-core k-NN engines only: not the VALU engine (set_knn_engine(1))");
}

// The set's operand is what prepare_train_bits (stage_knn.hip) builds for a deck of exactly the selected pages, with deck row ids
// in the keys: the selected rows of every duplicate group chained in row order (their first one the group's head), the surviving
// groups in the deck's norm order, the tile order of that tile count (knn_tile_order).
int page_set_create(slideo_matcher* m, int n, const int32_t* pages) {
    hipStream_t st = m->stream;
    const int P = (int)m->pages.size();
    int64_t rows = 0;
    std::vector<uint8_t> in_set((size_t)P, 0);
    for (int i = 0; i < n; ++i) { in_set[pages[i]] = 1; rows += (int64_t)m->pages[pages[i]].kp.size(); }
    if (rows == 0) fail(SLIDEO_ERR_EMPTY_INDEX, "the %d selected pages hold no descriptor", n);
    const int nu = (int)m->Mu;
    if (!m->d_uorder.p) {        // (the first set: finalize's host arrays to the device)
        m->d_uorder.reserve(m->h_uorder.size() * 4 + 16);
        HIP_CHECK(hipMemcpyAsync(m->d_uorder.p, m->h_uorder.data(), m->h_uorder.size() * 4, hipMemcpyHostToDevice, st));
        if (!m->h_urow.empty()) {
            m->d_urow.reserve(m->h_urow.size() * 4 + 16);
            HIP_CHECK(hipMemcpyAsync(m->d_urow.p, m->h_urow.data(), m->h_urow.size() * 4, hipMemcpyHostToDevice, st));
        }
    }
    std::unique_ptr<PageSet> ps(new PageSet());
    DevBuf d_in, d_head, d_cnt, d_cu, d_order;
    d_in.reserve(in_set.size() + 16);
    HIP_CHECK(hipMemcpyAsync(d_in.p, in_set.data(), in_set.size(), hipMemcpyHostToDevice, st));
    ps->d_grp_next.reserve((size_t)m->M * 4 + 16);
    HIP_CHECK(hipMemsetAsync(ps->d_grp_next.p, 0xFF, (size_t)m->M * 4, st));
    d_head.reserve((size_t)nu * 4 + 16);
    ps_regroup_kernel<<<cdiv(nu, PS_BLOCK), PS_BLOCK, 0, st>>>(m->h_urow.empty() ? nullptr : m->d_urow.as<int32_t>(), nu, m->d_grp_next.as<int32_t>(),
                                                               m->d_train_page.as<int32_t>(), d_in.as<uint8_t>(), d_head.as<int32_t>(),
                                                               ps->d_grp_next.as<int32_t>());
    check_launch("ps_regroup_kernel");
    const int nb = cdiv(nu, PS_BLOCK);
    d_cnt.reserve((size_t)(nb + 1) * 4 + 16);
    d_cu.reserve((size_t)nu * 4 + 16);
    ps_count_kernel<<<nb, PS_BLOCK, 0, st>>>(m->d_uorder.as<int32_t>(), nu, d_head.as<int32_t>(), d_cnt.as<uint32_t>());
    check_launch("ps_count_kernel");
    ps_scan_kernel<<<1, PS_SCAN_BLOCK, 0, st>>>(d_cnt.as<uint32_t>(), nb, d_cnt.as<uint32_t>() + nb);
    check_launch("ps_scan_kernel");
    ps_scatter_kernel<<<nb, PS_BLOCK, 0, st>>>(m->d_uorder.as<int32_t>(), nu, d_head.as<int32_t>(), d_cnt.as<uint32_t>(), d_cu.as<int32_t>());
    check_launch("ps_scatter_kernel");
    uint32_t ns = 0;
    HIP_CHECK(hipMemcpyAsync(&ns, d_cnt.as<uint32_t>() + nb, 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (ns == 0 || ns > (uint32_t)nu) fail(SLIDEO_ERR_HIP, "internal: page set compaction kept %u of %d distinct rows", ns, nu);
    const std::vector<int32_t> order = knn_tile_order(cdiv((int)ns, 32));
    const OperandLayout L = knn_operand_layout();
    SearchOperand& op = ps->op;
    op.reserve((int)ns, knn_operand_rows((int)ns), L);
    const int nt_pad = op.nt_pad;
    d_order.reserve(order.size() * 4 + 16);
    HIP_CHECK(hipMemcpyAsync(d_order.p, order.data(), order.size() * 4, hipMemcpyHostToDevice, st));
    // the distinct rows: d_utrain when the deck collapsed equal rows, else the deck's rows themselves
    const uint32_t* t = (m->Mu < m->M ? m->d_utrain : m->d_train).as<uint32_t>();
    ps_layout_kernel<<<cdiv(nt_pad, PS_BLOCK), PS_BLOCK, 0, st>>>(d_cu.as<int32_t>(), (int)ns, d_order.as<int32_t>(), nt_pad, t, d_head.as<int32_t>(),
                                                                  L.st_rows, L.side_u32, L.pad_norm, op.perm.as<int32_t>(), op.side.as<uint32_t>(),
                                                                  op.bound.as<float>());
    check_launch("ps_layout_kernel");
    knn_expand_operand(t, (int)ns, nt_pad, op.perm.as<int32_t>(), op.tx.as<uint4>(), st);
    HIP_CHECK(hipStreamSynchronize(st));                                  // (the scratch buffers die here)
    ps->n_pages = n; ps->rows = rows; ps->urows = ns;
    ps->pages.assign(pages, pages + n);
    std::sort(ps->pages.begin(), ps->pages.end());
    const int id = m->next_set_id++;
    m->page_sets[id] = std::move(ps);
    return id;
}

}  // namespace slideo

extern "C" {

int32_t slideo_matcher_create_page_set(slideo_matcher* m, int32_t n_pages, const int32_t* pages, int32_t* set_out) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (!m->finalized) fail(SLIDEO_ERR_STATE, "slideo_matcher_finalize_pages must be called before a page set is created");
    if (n_pages < 1 || !pages || !set_out) fail(SLIDEO_ERR_INVALID_ARG, "a page set needs n_pages >= 1 pages and set_out");
    const int P = (int)m->pages.size();
    std::vector<uint8_t> seen((size_t)P, 0);
    for (int i = 0; i < n_pages; ++i) {
        if (pages[i] < 0 || pages[i] >= P) fail(SLIDEO_ERR_INVALID_ARG, "page %d out of range (%d pages)", pages[i], P);
        if (seen[pages[i]]++) fail(SLIDEO_ERR_INVALID_ARG, "page %d is listed twice", pages[i]);
    }
    if (m->sift_on || m->cfg.matcher != 0) page_set_check_mode(m);
    if ((int)m->page_sets.size() >= MAX_PAGE_SETS) fail(SLIDEO_ERR_UNSUPPORTED, "%d page sets are live: release one first", MAX_PAGE_SETS);
    HIP_CHECK(hipSetDevice(m->device));
    *set_out = page_set_create(m, n_pages, pages);
    API_CATCH(m)
}

int32_t slideo_matcher_use_page_set(slideo_matcher* m, int32_t set) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (!m->finalized) fail(SLIDEO_ERR_STATE, "slideo_matcher_finalize_pages must be called before a page set is used");
    if (set != 0 && !m->page_sets.count(set)) fail(SLIDEO_ERR_INVALID_ARG, "page set %d is not live", set);
    if (set != 0) page_set_check_mode(m);
    m->cur_set = set;
    API_CATCH(m)
}

int32_t slideo_matcher_release_page_set(slideo_matcher* m, int32_t set) {
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (!m->finalized) fail(SLIDEO_ERR_STATE, "slideo_matcher_finalize_pages must be called before a page set is released");
    if (set == 0) fail(SLIDEO_ERR_INVALID_ARG, "set 0 is the whole deck: it cannot be released");
    const auto it = m->page_sets.find(set);
    if (it == m->page_sets.end()) fail(SLIDEO_ERR_INVALID_ARG, "page set %d is not live", set);
    if (m->cur_set == set) fail(SLIDEO_ERR_STATE, "page set %d is selected: select another (slideo_matcher_use_page_set) first", set);
    for (const Slot& S : m->slots)
        if (S.busy && S.u_set == set) fail(SLIDEO_ERR_STATE, "page set %d is searched by ticket %lld, which has not been collected", set, (long long)S.ticket);
    HIP_CHECK(hipSetDevice(m->device));
    m->page_sets.erase(it);
    API_CATCH(m)
}

int32_t slideo_matcher_page_set_info(const slideo_matcher* cm, int32_t set, int32_t* n_pages, int64_t* rows, int64_t* unique_rows, int64_t* bytes) {
    slideo_matcher* m = const_cast<slideo_matcher*>(cm);
    if (!m) return SLIDEO_ERR_INVALID_ARG;
    API_TRY
    if (!m->finalized) fail(SLIDEO_ERR_STATE, "slideo_matcher_finalize_pages must be called before page sets exist");
    if (set == 0) {
        if (n_pages) *n_pages = (int32_t)m->pages.size();
        if (rows) *rows = m->M;
        if (unique_rows) *unique_rows = m->Mu;
        if (bytes) *bytes = (int64_t)(m->train_op.bytes() + m->d_grp_next.cap);
        return SLIDEO_OK;
    }
    const auto it = m->page_sets.find(set);
    if (it == m->page_sets.end()) fail(SLIDEO_ERR_INVALID_ARG, "page set %d is not live", set);
    const PageSet& ps = *it->second;
    if (n_pages) *n_pages = ps.n_pages;
    if (rows) *rows = ps.rows;
    if (unique_rows) *unique_rows = ps.urows;
    if (bytes) *bytes = (int64_t)ps.bytes();
    API_CATCH(m)
}

}  // extern "C"
