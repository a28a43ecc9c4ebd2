// Scoring behind the C ABI (units of the host layer: model.hip.h): edit-distance alignment of label sequences.
#include "model.hip.h"
#include "score.hip.h"

// ------------------------------------------------------------------------------------ scoring: edit-distance alignment
// Where one pair's op-code table lives: the dynamic LDS it needs when that fits the budget, else 0 (the global workspace).
static size_t score_lds_need(const cocr_model *m, int n, int mm) {
    const size_t need = score_carry_bytes(n) + score_dir_words(n, mm) * 4;
    return need <= (size_t)std::min(std::max(m->sw.score_lds_max, 0), 64 * 1024) ? need : 0;
}

extern "C" int64_t cocr_edit_align_lds(cocr_model *m, int len_a, int len_b) {
    if (!m) return fail(COCR_EINVAL, "null argument");
    if (len_a < 0 || len_b < 0 || len_a > SCORE_MAX_LEN || len_b > SCORE_MAX_LEN)
        return fail(COCR_EINVAL, "sequences of %d and %d symbols (0 .. %d)", len_a, len_b, SCORE_MAX_LEN);
    return (int64_t)score_lds_need(m, len_a, len_b);
}

extern "C" int cocr_edit_align(cocr_model *m, const int32_t *a, const int64_t *a_offs, const int32_t *b, const int64_t *b_offs, int P,
                               int32_t *counts, uint8_t *ops, int32_t *ops_len, void *stream) {
    if (!m) return fail(COCR_EINVAL, "null argument");
    if (P < 0) return fail(COCR_EINVAL, "%d pairs", P);
    if (P == 0) return COCR_OK;
    if (!a_offs || !b_offs || !counts || (ops && !ops_len)) return fail(COCR_EINVAL, "null argument");
    if (a_offs[0] < 0 || b_offs[0] < 0) return fail(COCR_EINVAL, "negative offset");
    for (int p = 0; p < P; ++p) {
        const int64_t n = a_offs[p + 1] - a_offs[p], mm = b_offs[p + 1] - b_offs[p];
        if (n < 0 || mm < 0) return fail(COCR_EINVAL, "pair %d: offsets decrease", p);
        if (n > SCORE_MAX_LEN || mm > SCORE_MAX_LEN)
            return fail(COCR_EINVAL, "pair %d: sequences of %lld and %lld symbols (at most %d)", p, (long long)n, (long long)mm, SCORE_MAX_LEN);
    }
    if ((a_offs[P] > a_offs[0] && !a) || (b_offs[P] > b_offs[0] && !b)) return fail(COCR_EINVAL, "null argument");
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t s = (hipStream_t)stream;
    // launches: three LDS classes (a short pair does not pay for a long one's table), then the pairs whose table goes to the workspace;
    // inside a launch the largest matrices first
    static const size_t CLASS_MAX[3] = {2 * 1024, 8 * 1024, 64 * 1024};
    std::vector<int> cls[4];
    size_t cls_lds[4] = {0, 0, 0, 0}, ws_words = 0;
    std::vector<int64_t> cells((size_t)P);
    for (int p = 0; p < P; ++p) {
        const int n = (int)(a_offs[p + 1] - a_offs[p]), mm = (int)(b_offs[p + 1] - b_offs[p]);
        cells[p] = (int64_t)n * mm;
        const size_t need = score_lds_need(m, n, mm);
        int c = 3;
        if (need) c = need <= CLASS_MAX[0] ? 0 : need <= CLASS_MAX[1] ? 1 : 2;
        else ws_words = std::max(ws_words, score_dir_words(n, mm));
        cls[c].push_back(p);
        cls_lds[c] = std::max(cls_lds[c], need ? need : score_carry_bytes(n));
    }
    const int ws_groups = (int)std::min<size_t>(cls[3].size(), 32);      // workgroups of the workspace launch, one region each
    if (ws_groups) HIP_TRY(m->score.score_ws.grow((size_t)ws_groups * ws_words));
    // the tables of this call, through the pinned ring
    const size_t offs_bytes = (size_t)(P + 1) * 8, bytes = 2 * offs_bytes + (size_t)P * 4;
    unsigned char *h, *d;
    HIP_TRY(m->score.score_ring.stage(bytes, h, d));
    memcpy(h, a_offs, offs_bytes);
    memcpy(h + offs_bytes, b_offs, offs_bytes);
    int *order = reinterpret_cast<int *>(h + 2 * offs_bytes);
    size_t at = 0, first[4];
    for (int c = 0; c < 4; ++c) {
        std::sort(cls[c].begin(), cls[c].end(), [&](int x, int y) { return cells[x] != cells[y] ? cells[x] > cells[y] : x < y; });
        first[c] = at;
        for (int p : cls[c]) order[at++] = p;
    }
    HIP_TRY(m->score.score_ring.commit(bytes, s));
    const long long *d_ao = reinterpret_cast<const long long *>(d), *d_bo = reinterpret_cast<const long long *>(d + offs_bytes);
    const int *d_order = reinterpret_cast<const int *>(d + 2 * offs_bytes);
    for (int c = 0; c < 3; ++c) {
        if (cls[c].empty()) continue;
        hipLaunchKernelGGL(edit_align_kernel<true>, dim3((unsigned)cls[c].size()), dim3(64), (cls_lds[c] + 15) & ~(size_t)15, s, a, b, d_ao, d_bo,
                           d_order + first[c], (int)cls[c].size(), counts, ops, ops_len, (unsigned *)nullptr, (size_t)0);
        LAUNCH_CHECK();
    }
    if (ws_groups) {
        hipLaunchKernelGGL(edit_align_kernel<false>, dim3(ws_groups), dim3(64), (cls_lds[3] + 15) & ~(size_t)15, s, a, b, d_ao, d_bo,
                           d_order + first[3], (int)cls[3].size(), counts, ops, ops_len, m->score.score_ws.p, ws_words);
        LAUNCH_CHECK();
    }
    return COCR_OK;
}
