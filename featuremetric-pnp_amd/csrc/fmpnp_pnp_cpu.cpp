// fmpnp_pnp_cpu.cpp -- fmpnp_pnp_ransac_cpu and fmpnp_p3p_cpu: the CPU twin of fmpnp_pnp_ransac
// (s2dhm/pose_prediction/solve_pnp.py:44-69) with HOST pointers.
//
// Every value comes from fmpnp_pnp_impl.h, the header the kernels of fmpnp_pnp.hip are built from, and
// this unit is compiled as host code only, without contraction and without -mfma (fma() is libm's,
// correctly rounded): each + - * / sqrt rounds as the GPU's does, the hypotheses' keys meet in an
// integer maximum and the polish's sums are added in the header's fixed order (256 partial sums, then
// the tree), so every result field and mask byte is the GPU's bit for bit.  An explicit CPU entry
// point -- a parity bridge and a baseline -- never a fallback of the HIP entry points.
#include <string.h>

#include <algorithm>
#include <memory>
#include <mutex>
#include <vector>

#include "fmpnp.h"
#include "fmpnp_host.h"
#include "fmpnp_pnp_impl.h"

namespace {

using namespace fmpnp::pnp;

// the polish's sums in the order of include/fmpnp.h: lane l's inliers l, l + 256, ... then the tree
struct HostEval {
    const Cam &cam;
    const double *p3, *p2;
    const unsigned char *mask;
    int M;
    std::vector<double> &sh;  // [POLISH_LANES][NACC]
    void operator()(const double *R, const double *t, double *S) {
        std::fill(sh.begin(), sh.end(), 0.0);
        for (int l = 0; l < POLISH_LANES && l < M; ++l)
            for (int i = l; i < M; i += POLISH_LANES)
                if (mask[i]) polish_point(cam, R, t, p3 + 3 * (size_t)i, p2 + 2 * (size_t)i, &sh[(size_t)l * NACC]);
        for (int s = POLISH_LANES / 2; s > 0; s >>= 1)
            for (int l = 0; l < s; ++l)
                for (int k = 0; k < NACC; ++k) sh[(size_t)l * NACC + k] = sh[(size_t)l * NACC + k] + sh[(size_t)(l + s) * NACC + k];
        for (int k = 0; k < NACC; ++k) S[k] = sh[k];
    }
};

int pnp_args_cpu(const fmpnp_pnp_problem *probs, int n, size_t mask_bytes) {
    for (int i = 0; i < n; ++i) {
        const fmpnp_pnp_problem &p = probs[i];
        if (p.M < 0 || p.iters < 1 || p.n_dist != 4 || !(p.threshold >= 0.0)) return FMPNP_EINVAL;
        if (p.M < 4) continue;
        if (!p.points3d || !p.points2d) return FMPNP_EINVAL;
        if (p.mask_offset < 0 || (unsigned long long)p.mask_offset + (unsigned long long)p.M > mask_bytes)
            return FMPNP_EINVAL;
    }
    return 0;
}

// the best key of hypotheses [0, iters) of one problem over the host threads, 64 at a time; every thread keeps
// its own maximum, and the maxima are combined after the join (an integer maximum: any split gives the same
// key).  false: a thread or an allocation failed
bool best_key(const fmpnp_pnp_problem &p, const Cam &cam, int n_threads, unsigned long long *key) {
    const double thr2 = p.threshold * p.threshold;
    std::mutex mu;
    std::vector<std::shared_ptr<unsigned long long>> maxima;
    const bool ok = fmpnp::host::deal(p.iters, n_threads, [&]() {
        auto mine = std::make_shared<unsigned long long>(0ull);
        {
            std::lock_guard<std::mutex> lock(mu);
            maxima.push_back(mine);
        }
        return [&p, &cam, thr2, mine](long long h) {
            double R[9], t[3];
            int count = 0;
            if (hypothesis(cam, p.points3d, p.points2d, p.M, p.seed, (unsigned)h, R, t))
                for (int i = 0; i < p.M; ++i)
                    count += is_inlier(cam, R, t, p.points3d + 3 * (size_t)i, p.points2d + 2 * (size_t)i, thr2) ? 1 : 0;
            *mine = std::max(*mine, pack_key(count, (unsigned)h));
        };
    }, 64);
    *key = 0;
    for (const auto &m : maxima) *key = std::max(*key, *m);
    return ok;
}

}  // namespace

extern "C" int fmpnp_pnp_ransac_cpu(const fmpnp_pnp_problem *probs, int n, fmpnp_pnp_result *results,
                                    unsigned char *mask_all, size_t mask_bytes, int n_threads) {
    if (n < 0 || n_threads < 0) return FMPNP_EINVAL;
    if (n == 0) return 0;
    if (!probs || !results) return FMPNP_EINVAL;
    const int rc = pnp_args_cpu(probs, n, mask_all ? mask_bytes : 0);
    if (rc) return rc;
    try {  // (nothing throws across the C ABI: an allocation or thread failure is FMPNP_ENOMEM)
        std::vector<double> sh((size_t)POLISH_LANES * NACC);
        memset(results, 0, sizeof(fmpnp_pnp_result) * (size_t)n);
        if (mask_all && mask_bytes) memset(mask_all, 0, mask_bytes);
        for (int b = 0; b < n; ++b) {
            const fmpnp_pnp_problem &p = probs[b];
            fmpnp_pnp_result &res = results[b];
            if (p.M < 4) {
                res.status = FMPNP_PNP_TOO_FEW;
                continue;
            }
            const Cam cam = make_cam(p.K, p.dist);
            unsigned long long key = 0;
            if (!best_key(p, cam, n_threads, &key)) return FMPNP_ENOMEM;
            unsigned char *mask = mask_all + p.mask_offset;
            if ((int)(key >> 32) == 0) {
                res.best_h = -1;
                res.status = FMPNP_PNP_NO_MODEL;
                continue;
            }
            const unsigned h = ~(unsigned)key;
            const double thr2 = p.threshold * p.threshold;
            double Rh[9], th[3], R[9], t[3], cost;
            hypothesis(cam, p.points3d, p.points2d, p.M, p.seed, h, Rh, th);
            int count = 0;
            for (int i = 0; i < p.M; ++i) {
                const int in = is_inlier(cam, Rh, th, p.points3d + 3 * (size_t)i, p.points2d + 2 * (size_t)i, thr2) ? 1 : 0;
                mask[i] = (unsigned char)in;
                count += in;
            }
            HostEval eval{cam, p.points3d, p.points2d, mask, p.M, sh};
            int iters;
            const bool ok = polish(eval, Rh, th, R, t, cost, iters);
            for (int k = 0; k < 9; ++k) {
                res.R[k] = ok ? R[k] : Rh[k];
                res.R_hyp[k] = Rh[k];
            }
            for (int k = 0; k < 3; ++k) {
                res.t[k] = ok ? t[k] : th[k];
                res.t_hyp[k] = th[k];
            }
            res.cost = cost;
            res.num_inliers = count;
            res.best_h = (int)h;
            res.status = ok ? FMPNP_PNP_OK : FMPNP_PNP_POLISH_FAILED;
            res.polish_iters = iters;
        }
    } catch (...) {
        return FMPNP_ENOMEM;
    }
    return 0;
}

extern "C" int fmpnp_p3p_cpu(const double *bearings, const double *points, double *R_out, double *t_out) {
    if (!bearings || !points || !R_out || !t_out) return FMPNP_EINVAL;
    double y[3][3], x[3][3], R[4][9], t[4][3];
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) {
            y[i][k] = bearings[3 * i + k];
            x[i][k] = points[3 * i + k];
        }
    const int n = p3p(y, x, R, t);
    for (int i = 0; i < n; ++i) {
        for (int k = 0; k < 9; ++k) R_out[9 * i + k] = R[i][k];
        for (int k = 0; k < 3; ++k) t_out[3 * i + k] = t[i][k];
    }
    return n;
}
