// Stand-alone host program over fmpnp_localize_refine_prep_cpu (fmpnp_localize_cpu.cpp linked in), for sanitizer
// runs of the refinement stage's twin outside Python: `make localize-refine-sanitize` builds it with ASan + UBSan
// and runs it.  Four queries over six pairs in exactly-sized heap buffers (so a read or write one element outside
// a map, a query's rows or the descriptors is an ASan report): a solved one, a fallback one that reads a float64
// map, one of kind NONE and one whose best pair has no map; inliers outside the map, NaN, beyond int's range and
// on the negative wrap; both storage dtypes, with and without levels; a plain restatement to compare with, and
// the argument errors.
#include <math.h>
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

constexpr int C = 5, CS = 8, HR = 7, WR = 9, IMG0 = 28, IMG1 = 18, NQ = 4, NP = 6;
constexpr unsigned char FILL = 0xA5;
const int CAP[NQ] = {70, 5, 3, 9}, NROW[NQ] = {66, 5, 0, 9};

bool is_fill(const void *p, size_t n) {
    const unsigned char *c = (const unsigned char *)p;
    for (size_t i = 0; i < n; ++i)
        if (c[i] != FILL) return false;
    return true;
}

template <typename T>
void run(int n_levels, int intrinsics, int dtype) {
    std::vector<fmpnp_loc_pair> pairs(NP);
    memset((void *)pairs.data(), 0, sizeof(fmpnp_loc_pair) * NP);
    for (int g = 0; g < NP; ++g)
        for (int k = 0; k < 9; ++k) pairs[g].K[k] = 10.0 * g + k;
    // queries: pairs {0,1}, {2}, {3}, {4,5}; best 1, 0, -, 1
    const fmpnp_loc_query queries[NQ] = {{0, 0, 2, CAP[0], 0}, {70, 2, 1, CAP[1], 0}, {75, 3, 1, CAP[2], 0}, {78, 4, 2, CAP[3], 0}};
    const int R = 87;
    std::vector<float> map32((size_t)C * HR * WR);
    std::vector<double> map64((size_t)C * HR * WR);
    for (size_t i = 0; i < map32.size(); ++i) {
        map32[i] = (float)uni();
        map64[i] = uni();
    }
    std::vector<fmpnp_loc_refine_source> src(NP);
    memset((void *)src.data(), 0, sizeof(fmpnp_loc_refine_source) * NP);
    src[1] = fmpnp_loc_refine_source{map32.data(), FMPNP_F32, HR, WR, 0};
    src[2] = fmpnp_loc_refine_source{map64.data(), FMPNP_F64, HR, WR, 0};
    src[3] = src[1];  // (the NONE query's pair has a map: its kind alone gives N = 0)
    src[4] = src[1];  // (the last query's best pair, 5, has none)
    std::vector<fmpnp_loc_record> rec(NQ);
    memset((void *)rec.data(), 0, sizeof(fmpnp_loc_record) * NQ);
    const int best[NQ] = {1, 0, -1, 1}, kind[NQ] = {FMPNP_LOC_SOLVED, FMPNP_LOC_FALLBACK, FMPNP_LOC_NONE, FMPNP_LOC_SOLVED};
    for (int q = 0; q < NQ; ++q) {
        rec[q].best = best[q];
        rec[q].kind = kind[q];
        rec[q].N = NROW[q];
        for (int k = 0; k < 9; ++k) rec[q].R0[k] = q + 0.25 * k;
        for (int k = 0; k < 3; ++k) rec[q].t0[k] = -q - 0.5 * k;
    }
    std::vector<double> x3(3 * (size_t)R), r2(2 * (size_t)R);
    std::vector<float> q32(2 * (size_t)R);
    std::vector<int> idx((size_t)R);
    for (double &v : x3) v = uni();
    for (int i = 0; i < R; ++i) {
        r2[2 * (size_t)i] = IMG0 * uni() * 0.999;
        r2[2 * (size_t)i + 1] = IMG1 * uni() * 0.999 * HR / WR;  // (row = trunc(y W_ref / img1) must stay below H_ref)
    }
    // the edge rows of query 0 (col = trunc(x H_ref / img0) is checked against W_ref, as the reference does): outside, NaN, beyond int, the negative wrap and its end
    const double edge[][2] = {{36.0, 1.0}, {NAN, 1.0}, {1e300, 1.0}, {-1e300, -1e300}, {-4.5, 3.0},
                              {3.0, -14.0}, {3.0, -14.1 - 2.0}, {-0.5, -0.5}, {INFINITY, 0.0}};
    const bool edge_bad[] = {true, true, true, true, false, false, true, false, true};
    const int n_edge = (int)(sizeof(edge) / sizeof(edge[0]));
    for (int i = 0; i < n_edge; ++i) {
        r2[2 * (size_t)(10 + i)] = edge[i][0];
        r2[2 * (size_t)(10 + i) + 1] = edge[i][1];
    }
    const fmpnp_loc_best b{x3.data(), r2.data(), q32.data(), idx.data(), rec.data()};
    fmpnp_loc_refine_map maps[NQ];
    for (int q = 0; q < NQ; ++q) maps[q] = fmpnp_loc_refine_map{(const void *)(uintptr_t)(0x1000 * (q + 1)), 11 + q, 13 + q};
    const fmpnp_level lv[2] = {{2, 5}, {0, 2}};
    const fmpnp_loc_refine_params rp{C, CS, IMG0, IMG1, intrinsics, n_levels, n_levels ? lv : nullptr};
    const int n_res = n_levels ? n_levels + 1 : 1;
    std::vector<fmpnp_problem> probs((size_t)n_res * NQ);
    memset((void *)probs.data(), FILL, sizeof(fmpnp_problem) * probs.size());
    std::vector<T> fref((size_t)R * CS);
    memset((void *)fref.data(), FILL, sizeof(T) * fref.size());
    std::vector<int> flags(NQ, -1);
    CHECK(fmpnp_localize_refine_prep_cpu(pairs.data(), NP, queries, NQ, src.data(), maps, &rp, dtype, &b, probs.data(),
                                         fref.data(), flags.data()) == 0);
    const int want_n[NQ] = {NROW[0], NROW[1], 0, 0};
    for (int q = 0; q < NQ; ++q) {
        const size_t o = (size_t)queries[q].out_offset;
        for (int r = 0; r < n_res; ++r) {
            const fmpnp_problem &p = probs[(size_t)r * NQ + q];
            CHECK(p.N == want_n[q] && p.Hf == 11 + q && p.Wf == 13 + q && p.cstride == CS && p.ld_ref == CS);
            CHECK(p.feat == maps[q].feat && p.fref == (const void *)(fref.data() + o * CS) && p.pts3d == x3.data() + 3 * o);
            CHECK(p.window == nullptr && p.im_width == IMG0 && p.im_height == IMG1);
            const bool level = n_levels && r > 0;
            CHECK(p.c_begin == (level ? lv[r - 1].c_begin : 0) && p.c_end == (level ? lv[r - 1].c_end : C));
            const int last = queries[q].pair_begin + queries[q].pair_count - 1;
            const int kp = intrinsics == FMPNP_LOC_K_BEST && best[q] >= 0 ? queries[q].pair_begin + best[q] : last;
            CHECK(memcmp(p.K, pairs[kp].K, 72) == 0 && memcmp(p.R0, rec[q].R0, 72) == 0 && memcmp(p.t0, rec[q].t0, 24) == 0);
        }
        bool any_bad = false;
        for (int n = 0; n < want_n[q]; ++n) {
            const double x = r2[2 * (o + n)], y = r2[2 * (o + n) + 1];
            const double colf = (double)HR / IMG0 * x, rowf = (double)WR / IMG1 * y;
            bool bad = !(fabs(colf) < 1e9 && fabs(rowf) < 1e9);
            long col = bad ? 0 : (long)colf, row = bad ? 0 : (long)rowf;
            if (row < 0 && row >= -HR) row += HR;
            if (col < 0 && col >= -WR) col += WR;
            bad = bad || row < 0 || row >= HR || col < 0 || col >= WR;
            if (q == 0 && n >= 10 && n < 10 + n_edge) CHECK(bad == edge_bad[n - 10]);
            any_bad = any_bad || bad;
            for (int c = 0; c < CS; ++c) {
                const size_t at = ((size_t)c * HR + (size_t)row) * WR + (size_t)col;
                const T want = (bad || c >= C) ? (T)0 : q == 1 ? (T)map64[at] : (T)map32[at];
                CHECK(memcmp(&fref[(o + n) * CS + c], &want, sizeof(T)) == 0);
            }
        }
        CHECK(flags[q] == (any_bad ? 1 : 0));
        CHECK(is_fill(&fref[(o + want_n[q]) * CS], sizeof(T) * CS * (size_t)(CAP[q] - want_n[q])));
    }
    CHECK(flags[0] == 1 && flags[1] == 0);
    // the argument errors
    fmpnp_loc_refine_params bad = rp;
    bad.cstride = C - 1;
    CHECK(fmpnp_localize_refine_prep_cpu(pairs.data(), NP, queries, NQ, src.data(), maps, &bad, dtype, &b, probs.data(), fref.data(), flags.data()) == FMPNP_EINVAL);
    bad = rp;
    bad.intrinsics = 2;
    CHECK(fmpnp_localize_refine_prep_cpu(pairs.data(), NP, queries, NQ, src.data(), maps, &bad, dtype, &b, probs.data(), fref.data(), flags.data()) == FMPNP_EINVAL);
    bad = rp;
    bad.n_levels = FMPNP_LOC_REFINE_MAX_LEVELS + 1;
    CHECK(fmpnp_localize_refine_prep_cpu(pairs.data(), NP, queries, NQ, src.data(), maps, &bad, dtype, &b, probs.data(), fref.data(), flags.data()) == FMPNP_EINVAL);
    CHECK(fmpnp_localize_refine_prep_cpu(pairs.data(), NP, queries, NQ, src.data(), maps, &rp, 2, &b, probs.data(), fref.data(), flags.data()) == FMPNP_EINVAL);
    CHECK(fmpnp_localize_refine_prep_cpu(pairs.data(), NP - 1, queries, NQ, src.data(), maps, &rp, dtype, &b, probs.data(), fref.data(), flags.data()) == FMPNP_EINVAL);
    CHECK(fmpnp_localize_refine_prep_cpu(pairs.data(), NP, queries, NQ, nullptr, maps, &rp, dtype, &b, probs.data(), fref.data(), flags.data()) == FMPNP_EINVAL);
    CHECK(fmpnp_localize_refine_prep_cpu(pairs.data(), NP, queries, NQ, src.data(), maps, &rp, dtype, &b, nullptr, fref.data(), flags.data()) == FMPNP_EINVAL);
    CHECK(fmpnp_localize_refine_prep_cpu(nullptr, 0, nullptr, 0, nullptr, nullptr, &rp, dtype, &b, nullptr, nullptr, nullptr) == 0);
}

}  // namespace

int main() {
    for (int n_levels = 0; n_levels <= 2; n_levels += 2)
        for (int intrinsics = 0; intrinsics <= 1; ++intrinsics) {
            run<float>(n_levels, intrinsics, FMPNP_F32);
            run<double>(n_levels, intrinsics, FMPNP_F64);
        }
    if (fails) {
        printf("localize_refine: %d check(s) FAILED\n", fails);
        return 1;
    }
    printf("localize_refine: ok\n");
    return 0;
}
