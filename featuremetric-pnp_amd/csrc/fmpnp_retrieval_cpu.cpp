// fmpnp_retrieval_cpu.cpp -- fmpnp_netvlad_pool_cpu and fmpnp_rank_topn_cpu: the CPU twins of the retrieval
// stage (fmpnp_retrieval.hip) with HOST pointers.
//
// The contract of include/fmpnp.h restated for a CPU core.  Every value outside the products comes from
// csrc/fmpnp_retrieval_impl.h, the header the kernels are built from; the products are explicit fmaf chains
// in the contract's order (what v_mfma_f32_32x32x2_f32 computes), and the unit is built without
// contraction and without -mfma (fmaf is libm's, correctly rounded; where the core has FMA the same loops
// compiled for it run instead: one vfmadd per product, the same value).  So every output is the GPU's bit
// for bit, whatever the thread count: the images (pooling) and the query rows (ranking) are independent and
// are dealt over the host threads.  Explicit CPU entry points -- a parity bridge and a baseline -- never a
// fallback of the HIP entry points.
#include <algorithm>
#include <functional>
#include <memory>
#include <vector>

#include "fmpnp.h"
#include "fmpnp_host.h"
#include "fmpnp_retrieval_impl.h"

namespace {

using namespace fmpnp::rv;

using fmpnp::host::deal;
using fmpnp::host::fmaf_chains;

struct Pool {
    const float *x;
    int C, P, K;
    size_t sb, sc;
    const float *w;
    int ld_w;
    const float *cent;
    int ld_c;
    bool norm;
    float *out;
    size_t ld_out;
};

struct PoolScratch {
    std::vector<float> d, a, xh, xt, V, Vs;
    explicit PoolScratch(const Pool &k)
        : d((size_t)k.P), a((size_t)k.K * (size_t)k.P), xh((size_t)k.C * (size_t)SEG), xt((size_t)SEG * ((size_t)k.C + 1)),
          V((size_t)k.K * ((size_t)k.C + 1)), Vs((size_t)k.C + 1) {}
};

void pool_image(const Pool &k, PoolScratch &t, int b) {
    const int C = k.C, P = k.P, K = k.K;
    const float *xb = k.x + (size_t)b * k.sb;
    const size_t ldv = (size_t)C + 1;
    std::fill(t.V.begin(), t.V.end(), 0.f);
    // a segment at a time: its denominators and x^ (the same values wherever they are formed), its
    // assignments, its partial; then the partial joins the total, in segment order
    for (int ps = 0; ps < P; ps += SEG) {
        const int np = std::min(SEG, P - ps);
        for (int j = 0; j < np; ++j) {
            float dn = 1.f;
            if (k.norm) {
                float s[NORM_CHAINS] = {0.f, 0.f, 0.f, 0.f};
                for (int c = 0; c < C; ++c) s[c % NORM_CHAINS] = square_link(xb[(size_t)c * k.sc + ps + j], s[c % NORM_CHAINS]);
                dn = position_norm(s[0], s[1], s[2], s[3]);
            }
            t.d[(size_t)(ps + j)] = dn;
        }
        for (int c = 0; c < C; ++c)
            for (int j = 0; j < np; ++j) {
                const float v = xb[(size_t)c * k.sc + ps + j];
                const float xv = k.norm ? quotient(v, t.d[(size_t)(ps + j)]) : v;
                t.xh[(size_t)c * SEG + j] = xv;
                t.xt[(size_t)j * ldv + c] = xv;
            }
        for (int j = 0; j < np; ++j) t.xt[(size_t)j * ldv + C] = 1.f;  // the assignment sum's column
        // logits: a chain over c ascending per (cluster, position)
        for (int kk = 0; kk < K; ++kk)
            fmaf_chains(k.w + (size_t)kk * k.ld_w, t.xh.data(), (size_t)SEG, C, np, &t.a[(size_t)kk * P + ps]);
        for (int j = 0; j < np; ++j) {
            float *col = &t.a[(size_t)(ps + j)];
            float m = col[0];
            for (int kk = 1; kk < K; ++kk) m = max_link(m, col[(size_t)kk * P]);
            for (int kk = 0; kk < K; ++kk) col[(size_t)kk * P] = exp_neg(col[(size_t)kk * P] - m);
            float sum = 0.f;
            for (int kk = 0; kk < K; ++kk) sum = sum + col[(size_t)kk * P];
            for (int kk = 0; kk < K; ++kk) col[(size_t)kk * P] = quotient(col[(size_t)kk * P], sum);
        }
        // the segment's partial: a chain over its positions ascending per (cluster, channel)
        for (int kk = 0; kk < K; ++kk) {
            fmaf_chains(&t.a[(size_t)kk * P + ps], t.xt.data(), ldv, np, C + 1, t.Vs.data());
            float *Vk = &t.V[(size_t)kk * ldv];
            for (int c = 0; c <= C; ++c) Vk[c] = Vk[c] + t.Vs[(size_t)c];
        }
    }
    // centroid term, intra-normalisation, final normalisation
    float *o = k.out + (size_t)b * k.ld_out;
    float total = 0.f;
    for (int kk = 0; kk < K; ++kk) {
        const float *Vk = &t.V[(size_t)kk * ldv];
        float *row = o + (size_t)kk * C;
        float ch[ROW_CHAINS];
        auto tree = [&ch]() {
            for (int off = ROW_CHAINS / 2; off > 0; off >>= 1)
                for (int i = 0; i < off; ++i) ch[i] = ch[i] + ch[i + off];
            return ch[0];
        };
        for (int i = 0; i < ROW_CHAINS; ++i) ch[i] = 0.f;
        for (int c = 0; c < C; ++c) {
            row[c] = centroid_term(Vk[c], Vk[C], k.cent[(size_t)kk * k.ld_c + c]);
            ch[c % ROW_CHAINS] = square_link(row[c], ch[c % ROW_CHAINS]);
        }
        const float n = norm_floor(tree());
        for (int i = 0; i < ROW_CHAINS; ++i) ch[i] = 0.f;
        for (int c = 0; c < C; ++c) {
            row[c] = quotient(row[c], n);
            ch[c % ROW_CHAINS] = square_link(row[c], ch[c % ROW_CHAINS]);
        }
        total = total + tree();
    }
    const float n = norm_floor(total);
    for (size_t i = 0; i < (size_t)K * (size_t)C; ++i) o[i] = quotient(o[i], n);
}

}  // namespace

extern "C" int fmpnp_netvlad_pool_cpu(const float *x, int B, int C, int P, long long x_stride_b, long long x_stride_c,
                                      const float *weight, int K, int ld_w, const float *centroids, int ld_c,
                                      int normalize_input, float *out, long long ld_out, int n_threads) {
    if (n_threads < 0) return FMPNP_EINVAL;
    const int rc = pool_args(x, B, C, P, x_stride_b, x_stride_c, weight, K, ld_w, centroids, ld_c, normalize_input, out,
                             ld_out);
    if (rc) return rc;
    if (B == 0) return 0;
    const Pool k{x, C, P, K, (size_t)x_stride_b, (size_t)x_stride_c, weight, ld_w, centroids, ld_c,
                 normalize_input != 0, out, (size_t)ld_out};
    try {  // (nothing throws across the C ABI: an allocation or thread failure is FMPNP_ENOMEM)
        const bool ok = deal(B, n_threads, [&k]() {
            auto scratch = std::make_shared<PoolScratch>(k);
            return [&k, scratch](long long b) { pool_image(k, *scratch, (int)b); };
        });
        return ok ? 0 : FMPNP_ENOMEM;
    } catch (...) {
        return FMPNP_ENOMEM;
    }
}

extern "C" int fmpnp_rank_topn_cpu(const float *qry, int Q, int ld_q, const float *ref_t, int D, int R, int ld_r, int n,
                                   int *idx, float *top, float *scores, int n_threads) {
    if (n_threads < 0) return FMPNP_EINVAL;
    const int rc = rank_args(qry, Q, ld_q, ref_t, D, R, ld_r, n, idx, top);
    if (rc) return rc;
    if (Q == 0) return 0;
    try {
        const bool ok = deal(Q, n_threads, [&]() {
            auto rowbuf = std::make_shared<std::vector<float>>(scores ? 0 : (size_t)R);
            auto words = std::make_shared<std::vector<uint64_t>>((size_t)R);
            return [=](long long q) {
                float *row = scores ? scores + (size_t)q * R : rowbuf->data();
                constexpr int JB = 1024;  // columns per accumulator block (stays in L1)
                for (int j0 = 0; j0 < R; j0 += JB)
                    fmaf_chains(qry + (size_t)q * ld_q, ref_t + j0, (size_t)ld_r, D, std::min(JB, R - j0), row + j0);
                for (int j = 0; j < R; ++j) (*words)[(size_t)j] = rank_word(row[j], (uint32_t)j);
                std::partial_sort(words->begin(), words->begin() + n, words->end(), std::greater<uint64_t>());
                for (int i = 0; i < n; ++i) {
                    const uint32_t j = word_index((*words)[(size_t)i]);
                    idx[(size_t)q * n + i] = (int)j;
                    top[(size_t)q * n + i] = row[j];
                }
            };
        });
        return ok ? 0 : FMPNP_ENOMEM;
    } catch (...) {
        return FMPNP_ENOMEM;
    }
}
