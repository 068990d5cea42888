// Stand-alone host program over fmpnp_localize_build_cpu / fmpnp_localize_pick_cpu (fmpnp_localize_cpu.cpp
// linked in), for sanitizer runs of the glue twins outside Python: `make localize-sanitize` builds it with
// ASan + UBSan and runs it.  One query of six pairs with the row counts of the compaction (1, 63, 64, 65, 257,
// 1000) in exactly-sized heap buffers (so a read or write one element outside a pair's rows or a query's
// output range is an ASan report), seeded argmax / mask bytes, hand-made PnP results for each kind of best
// pair, a plain restatement of both steps to compare with, and the argument errors.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "fmpnp.h"

namespace {

uint64_t rng_state = 0x9e3779b97f4a7c15ull;
uint32_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}
double uni() { return (double)rnd() / 2147483648.0; }

int fails = 0;
#define CHECK(c)                                               \
    do {                                                       \
        if (!(c)) {                                            \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++fails;                                           \
        }                                                      \
    } while (0)

const int ROWS[6] = {1, 63, 64, 65, 257, 1000};
constexpr int W = 16, H = 16;
constexpr unsigned char FILL = 0xA5;

struct Scene {
    std::vector<std::vector<double>> p3, p2;  // per pair, exactly sized
    std::vector<fmpnp_loc_pair> pairs;
    fmpnp_loc_query query;
    fmpnp_loc_params prm;
    std::vector<int> argmax;
    std::vector<unsigned char> mask, pnp_mask;
    long long T = 0;
    // outputs, exactly sized
    std::vector<float> m_q32, b_q32;
    std::vector<double> m_q64, m_x3, m_r2, b_x3, b_r2;
    std::vector<int> m_src, counts, b_idx;
    std::vector<fmpnp_loc_record> rec;
    std::vector<fmpnp_pnp_problem> probs;
    std::vector<fmpnp_pnp_result> results;
    fmpnp_loc_matches m;
    fmpnp_loc_best b;
};

template <class T>
void fill(std::vector<T> &v, size_t n) {
    v.resize(n);
    memset((void *)v.data(), FILL, n * sizeof(T));
}

void make(Scene &s, int fallback_pair) {
    s.pairs.resize(6);
    s.p3.resize(6);
    s.p2.resize(6);
    s.T = 0;
    for (int g = 0; g < 6; ++g) {
        const int n = ROWS[g];
        s.p3[g].resize(3 * (size_t)n);
        s.p2[g].resize(2 * (size_t)n);
        for (double &v : s.p3[g]) v = uni();
        for (double &v : s.p2[g]) v = 64.0 * uni();
        fmpnp_loc_pair &p = s.pairs[g];
        memset(&p, 0, sizeof p);
        p.points3d = s.p3[g].data();
        p.points2d = s.p2[g].data();
        for (int k = 0; k < 9; ++k) p.K[k] = g + k;
        for (int k = 0; k < 4; ++k) p.dist[k] = 0.1 * (g + k);
        for (int k = 0; k < 9; ++k) p.fallback_R[k] = 100 + g + k;
        for (int k = 0; k < 3; ++k) p.fallback_t[k] = 200 + g + k;
        p.row_offset = s.T;
        p.image_shape[0] = 64.0f;
        p.image_shape[1] = 48.0f;
        p.dim[0] = W;
        p.dim[1] = H;
        p.n_rows = n;
        p.has_fallback = g == fallback_pair;
        s.T += n;
    }
    s.query = fmpnp_loc_query{0, 0, 6, 1000, 0};
    s.prm = fmpnp_loc_params{12.0, 99ull, 256, 70, 5, 1};
    s.argmax.resize((size_t)s.T);
    s.mask.resize((size_t)s.T);
    for (long long i = 0; i < s.T; ++i) {
        s.argmax[(size_t)i] = (int)(rnd() % (W * H));
        s.mask[(size_t)i] = uni() < 0.6 ? (unsigned char)(1 + rnd() % 255) : 0;
    }
    const size_t T = (size_t)s.T;
    fill(s.m_q32, 2 * T), fill(s.m_q64, 2 * T), fill(s.m_x3, 3 * T), fill(s.m_r2, 2 * T), fill(s.m_src, T), fill(s.counts, 6);
    fill(s.b_q32, 2 * 1000), fill(s.b_x3, 3 * 1000), fill(s.b_r2, 2 * 1000), fill(s.b_idx, 1000), fill(s.rec, 1);
    fill(s.probs, 6), fill(s.results, 6), fill(s.pnp_mask, T);
    s.m = fmpnp_loc_matches{s.m_q32.data(), s.m_q64.data(), s.m_x3.data(), s.m_r2.data(), s.m_src.data(), s.counts.data()};
    s.b = fmpnp_loc_best{s.b_x3.data(), s.b_r2.data(), s.b_q32.data(), s.b_idx.data(), s.rec.data()};
}

bool is_fill(const void *p, size_t n) {
    const unsigned char *c = (const unsigned char *)p;
    for (size_t i = 0; i < n; ++i)
        if (c[i] != FILL) return false;
    return true;
}

void check_build(Scene &s) {
    CHECK(fmpnp_localize_build_cpu(s.pairs.data(), 6, &s.prm, s.argmax.data(), s.mask.data(), s.T, &s.m, s.probs.data()) == 0);
    for (int g = 0; g < 6; ++g) {
        const fmpnp_loc_pair &p = s.pairs[g];
        const size_t off = (size_t)p.row_offset;
        int m = 0;
        for (int i = 0; i < p.n_rows; ++i) {
            if (!s.mask[off + i]) continue;
            const int a = s.argmax[off + i];
            const float c0 = 64.0f / 16.0f, c1 = 48.0f / 16.0f;
            const float x = (float)(a % H) * c0 + c0 / 2.0f, y = (float)(a / H) * c1 + c1 / 2.0f;
            CHECK(s.m_q32[2 * (off + m)] == x && s.m_q32[2 * (off + m) + 1] == y);
            CHECK(s.m_q64[2 * (off + m)] == (double)x && s.m_q64[2 * (off + m) + 1] == (double)y);
            CHECK(memcmp(&s.m_x3[3 * (off + m)], &s.p3[g][3 * (size_t)i], 24) == 0);
            CHECK(memcmp(&s.m_r2[2 * (off + m)], &s.p2[g][2 * (size_t)i], 16) == 0);
            CHECK(s.m_src[off + m] == i);
            ++m;
        }
        CHECK(s.counts[g] == m);
        const size_t rest = (size_t)(p.n_rows - m);
        CHECK(is_fill(&s.m_q32[2 * (off + m)], 8 * rest) && is_fill(&s.m_x3[3 * (off + m)], 24 * rest));
        CHECK(is_fill(&s.m_src[off + m], 4 * rest));
        const fmpnp_pnp_problem &q = s.probs[g];
        CHECK(q.M == (m > 70 ? m : 0) && q.iters == 256 && q.n_dist == 4 && q.reserved == 0 && q.seed == 99ull);
        CHECK(q.points3d == &s.m_x3[3 * off] && q.points2d == &s.m_q64[2 * off] && q.mask_offset == p.row_offset);
        CHECK(q.threshold == 12.0 && memcmp(q.K, p.K, 72) == 0 && memcmp(q.dist, p.dist, 32) == 0);
    }
}

// hand-made PnP results: pair `solved` solves with n_in inliers (status 0), every other pair fails
void check_pick(Scene &s, int solved, int n_in, int masked, int want_best, int want_kind) {
    s.prm.return_masked = masked;
    for (int g = 0; g < 6; ++g) s.results[g].status = g & 1 ? FMPNP_PNP_NO_MODEL : FMPNP_PNP_TOO_FEW;  // (the rest: fill)
    std::vector<int> inl;
    if (solved >= 0) {
        const size_t off = (size_t)s.pairs[solved].row_offset;
        const int cnt = s.counts[solved];
        memset(&s.pnp_mask[off], 0, (size_t)cnt);
        for (int k = 0; k < n_in; ++k) s.pnp_mask[off + (size_t)((long long)k * cnt / n_in)] = 1;  // ascending, distinct
        for (int mrow = 0; mrow < cnt; ++mrow)
            if (s.pnp_mask[off + mrow]) inl.push_back(mrow);
        fmpnp_pnp_result &r = s.results[solved];
        r.status = FMPNP_PNP_OK;
        r.num_inliers = n_in;
        for (int k = 0; k < 9; ++k) r.R[k] = 0.5 + k;
        for (int k = 0; k < 3; ++k) r.t[k] = -1.5 - k;
    }
    CHECK(fmpnp_localize_pick_cpu(s.pairs.data(), 6, &s.query, 1, &s.prm, s.results.data(), s.pnp_mask.data(), s.T, &s.m,
                                  &s.b) == 0);
    const fmpnp_loc_record &rec = s.rec[0];
    CHECK(rec.best == want_best && rec.kind == want_kind && rec.reserved == 0);
    if (want_best < 0) {
        CHECK(rec.N == 0 && rec.num_matches == 0 && rec.num_inliers == 0 && rec.R0[0] == 0.0 && rec.t0[2] == 0.0);
        CHECK(is_fill(s.b_x3.data(), 24 * 1000) && is_fill(s.b_idx.data(), 4 * 1000));
        return;
    }
    const size_t off = (size_t)s.pairs[want_best].row_offset;
    const int cnt = s.counts[want_best];
    const bool sol = want_kind == FMPNP_LOC_SOLVED;
    const int N = sol && masked ? n_in : cnt;
    CHECK(rec.N == N && rec.num_matches == cnt && rec.num_inliers == (sol ? n_in : 0));
    CHECK(rec.R0[3] == (sol ? 3.5 : 100.0 + want_best + 3) && rec.t0[1] == (sol ? -2.5 : 200.0 + want_best + 1));
    for (int d = 0; d < N; ++d) {
        const size_t src = off + (size_t)(sol && masked ? inl[(size_t)d] : d);
        CHECK(memcmp(&s.b_x3[3 * (size_t)d], &s.m_x3[3 * src], 24) == 0 && memcmp(&s.b_r2[2 * (size_t)d], &s.m_r2[2 * src], 16) == 0);
        CHECK(memcmp(&s.b_q32[2 * (size_t)d], &s.m_q32[2 * src], 8) == 0);
    }
    CHECK(is_fill(&s.b_x3[3 * (size_t)N], 24 * (size_t)(1000 - N)) && is_fill(&s.b_q32[2 * (size_t)N], 8 * (size_t)(1000 - N)));
    const size_t n_idx = sol ? inl.size() : 0;
    for (size_t k = 0; k < n_idx; ++k) CHECK(s.b_idx[k] == inl[k]);
    CHECK(is_fill(&s.b_idx[n_idx], 4 * (1000 - n_idx)));
}

void check_errors(Scene &s) {
    CHECK(fmpnp_localize_build_cpu(nullptr, 6, &s.prm, s.argmax.data(), s.mask.data(), s.T, &s.m, s.probs.data()) == FMPNP_EINVAL);
    CHECK(fmpnp_localize_build_cpu(s.pairs.data(), 6, nullptr, s.argmax.data(), s.mask.data(), s.T, &s.m, s.probs.data()) == FMPNP_EINVAL);
    CHECK(fmpnp_localize_build_cpu(s.pairs.data(), 6, &s.prm, nullptr, s.mask.data(), s.T, &s.m, s.probs.data()) == FMPNP_EINVAL);
    CHECK(fmpnp_localize_build_cpu(s.pairs.data(), 6, &s.prm, s.argmax.data(), nullptr, s.T, &s.m, s.probs.data()) == FMPNP_EINVAL);
    CHECK(fmpnp_localize_build_cpu(s.pairs.data(), 6, &s.prm, s.argmax.data(), s.mask.data(), s.T, nullptr, s.probs.data()) == FMPNP_EINVAL);
    CHECK(fmpnp_localize_build_cpu(s.pairs.data(), 6, &s.prm, s.argmax.data(), s.mask.data(), s.T, &s.m, nullptr) == FMPNP_EINVAL);
    CHECK(fmpnp_localize_build_cpu(s.pairs.data(), -1, &s.prm, s.argmax.data(), s.mask.data(), s.T, &s.m, s.probs.data()) == FMPNP_EINVAL);
    CHECK(fmpnp_localize_build_cpu(s.pairs.data(), 6, &s.prm, s.argmax.data(), s.mask.data(), s.T - 1, &s.m, s.probs.data()) == FMPNP_EINVAL);
    CHECK(fmpnp_localize_build_cpu(s.pairs.data(), 65536, &s.prm, s.argmax.data(), s.mask.data(), s.T, &s.m, s.probs.data()) == FMPNP_ETOOBIG);
    fmpnp_loc_query q = s.query;
    q.out_cap = 999;
    CHECK(fmpnp_localize_pick_cpu(s.pairs.data(), 6, &q, 1, &s.prm, s.results.data(), s.pnp_mask.data(), s.T, &s.m, &s.b) == FMPNP_EINVAL);
    q = s.query;
    q.pair_count = 7;
    CHECK(fmpnp_localize_pick_cpu(s.pairs.data(), 6, &q, 1, &s.prm, s.results.data(), s.pnp_mask.data(), s.T, &s.m, &s.b) == FMPNP_EINVAL);
    CHECK(fmpnp_localize_pick_cpu(s.pairs.data(), 6, &s.query, -1, &s.prm, s.results.data(), s.pnp_mask.data(), s.T, &s.m, &s.b) == FMPNP_EINVAL);
    CHECK(fmpnp_localize_pick_cpu(s.pairs.data(), 6, &s.query, 1, &s.prm, nullptr, s.pnp_mask.data(), s.T, &s.m, &s.b) == FMPNP_EINVAL);
    CHECK(fmpnp_localize_pick_cpu(s.pairs.data(), 6, &s.query, 1, &s.prm, s.results.data(), s.pnp_mask.data(), s.T, &s.m, nullptr) == FMPNP_EINVAL);
    CHECK(fmpnp_localize_pick_cpu(s.pairs.data(), 65536, &s.query, 1, &s.prm, s.results.data(), s.pnp_mask.data(), s.T, &s.m, &s.b) == FMPNP_ETOOBIG);
    // no pairs and no queries: nothing is read or written
    CHECK(fmpnp_localize_build_cpu(nullptr, 0, &s.prm, nullptr, nullptr, 0, &s.m, nullptr) == 0);
    CHECK(fmpnp_localize_pick_cpu(nullptr, 0, nullptr, 0, &s.prm, nullptr, nullptr, 0, &s.m, &s.b) == 0);
}

}  // namespace

int main() {
    struct Run {
        int fallback_pair, solved, n_in, masked, want_best, want_kind;
    };
    const Run runs[] = {
        {-1, 5, 300, 1, 5, FMPNP_LOC_SOLVED},   // the inliers cross a 256-row tile
        {-1, 5, 300, 0, 5, FMPNP_LOC_SOLVED},   // return_masked = 0: every match, idx still the inliers
        {2, 4, 100, 1, 4, FMPNP_LOC_SOLVED},    // a fallback beside a solved pair loses
        {2, 4, 4, 1, 2, FMPNP_LOC_FALLBACK},    // below minimum_inliers: the fallback wins with all its matches
        {1, -1, 0, 1, 1, FMPNP_LOC_FALLBACK},
        {-1, -1, 0, 1, -1, FMPNP_LOC_NONE},
        {-1, 3, 4, 1, -1, FMPNP_LOC_NONE},
    };
    for (const Run &r : runs) {
        Scene s;
        make(s, r.fallback_pair);
        check_build(s);
        check_pick(s, r.solved, r.n_in, r.masked, r.want_best, r.want_kind);
        check_errors(s);
    }
    // a query whose output range is not the first: two queries over the same six pairs' halves
    {
        Scene s;
        make(s, -1);
        check_build(s);
        fmpnp_loc_query qs[2] = {{0, 0, 4, 65, 0}, {65, 4, 2, 1000, 0}};
        fill(s.b_q32, 2 * 1065), fill(s.b_x3, 3 * 1065), fill(s.b_r2, 2 * 1065), fill(s.b_idx, 1065), fill(s.rec, 2);
        s.b = fmpnp_loc_best{s.b_x3.data(), s.b_r2.data(), s.b_q32.data(), s.b_idx.data(), s.rec.data()};
        s.pairs[2].has_fallback = 1;
        for (int g = 0; g < 6; ++g) s.results[g].status = FMPNP_PNP_NO_MODEL;
        s.results[5].status = FMPNP_PNP_OK;  // the second query's second pair: its count > 70 rows were "solved"
        s.results[5].num_inliers = s.counts[5];
        memset(&s.pnp_mask[(size_t)s.pairs[5].row_offset], 1, (size_t)s.counts[5]);
        CHECK(fmpnp_localize_pick_cpu(s.pairs.data(), 6, qs, 2, &s.prm, s.results.data(), s.pnp_mask.data(), s.T, &s.m, &s.b) == 0);
        CHECK(s.rec[0].best == 2 && s.rec[0].kind == FMPNP_LOC_FALLBACK && s.rec[0].N == s.counts[2]);
        CHECK(s.rec[1].best == 1 && s.rec[1].kind == FMPNP_LOC_SOLVED && s.rec[1].N == s.counts[5]);
        CHECK(memcmp(&s.b_x3[3 * 65], &s.m_x3[3 * (size_t)s.pairs[5].row_offset], 24 * (size_t)s.counts[5]) == 0);
        CHECK(s.b_idx[65] == 0 && s.b_idx[65 + (size_t)s.counts[5] - 1] == s.counts[5] - 1);
        CHECK(is_fill(&s.b_x3[3 * (size_t)s.counts[2]], 24 * (size_t)(65 - s.counts[2])));
    }
    if (fails) {
        printf("test_localize_cpu: %d check(s) FAILED\n", fails);
        return 1;
    }
    printf("test_localize_cpu: all checks passed\n");
    return 0;
}
