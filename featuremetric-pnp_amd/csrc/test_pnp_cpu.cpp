// Stand-alone host program over fmpnp_pnp_ransac_cpu / fmpnp_p3p_cpu (fmpnp_pnp_cpu.cpp linked in), for
// sanitizer runs of the twin outside Python: `make pnp-sanitize` builds it with ASan + UBSan and runs it.
// Without arguments it runs built-in problems (a planted one, M = 3, 4, 5, collinear, non-finite,
// coincident points, a bad coefficient count); with a file it also runs the problems stored there:
// int32 n, then per problem int32 M, iters; double K[9], dist[4], threshold; points3d [M][3], points2d [M][2].
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "fmpnp.h"

namespace {

struct Prob {
    std::vector<double> p3, p2;
    double K[9], dist[4], thr;
    int M, iters;
};

uint64_t rng_state = 0x1234567ull;
double uni() {  // [0, 1)
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(rng_state >> 11) / 9007199254740992.0;
}

Prob planted(int M, double fo, int iters) {
    Prob p;
    const double K[9] = {400, 0, 512, 0, 400, 512, 0, 0, 1};
    memcpy(p.K, K, sizeof K);
    memset(p.dist, 0, sizeof p.dist);
    p.thr = 12.0;
    p.M = M;
    p.iters = iters;
    const double t[3] = {0.3, -0.2, 0.5}, a = 0.2;  // pose: Rz(a), t
    for (int i = 0; i < M; ++i) {
        const double z = 5 + 45 * uni(), x = (uni() * 2 - 1) * z, y = (uni() * 2 - 1) * z;
        const double c[3] = {x - t[0], y - t[1], z - t[2]};  // world = Rz(-a) (P - t)
        p.p3.push_back(cos(a) * c[0] + sin(a) * c[1]);
        p.p3.push_back(-sin(a) * c[0] + cos(a) * c[1]);
        p.p3.push_back(c[2]);
        double u = 400 * x / z + 512, v = 400 * y / z + 512;
        if (uni() < fo) u += 100, v -= 70;
        p.p2.push_back(u);
        p.p2.push_back(v);
    }
    return p;
}

int run(std::vector<Prob> &ps, const char *what) {
    std::vector<fmpnp_pnp_problem> d(ps.size());
    size_t total = 0;
    for (size_t i = 0; i < ps.size(); ++i) {
        memset(&d[i], 0, sizeof d[i]);
        d[i].points3d = ps[i].p3.data();
        d[i].points2d = ps[i].p2.data();
        memcpy(d[i].K, ps[i].K, sizeof d[i].K);
        memcpy(d[i].dist, ps[i].dist, sizeof d[i].dist);
        d[i].threshold = ps[i].thr;
        d[i].seed = 0;
        d[i].mask_offset = (long long)total;
        d[i].M = ps[i].M;
        d[i].iters = ps[i].iters;
        d[i].n_dist = 4;
        total += (size_t)ps[i].M;
    }
    std::vector<fmpnp_pnp_result> res(ps.size());
    std::vector<unsigned char> mask(total + 1);
    for (int nt : {1, 3}) {
        const int rc = fmpnp_pnp_ransac_cpu(d.data(), (int)ps.size(), res.data(), mask.data(), total, nt);
        if (rc) {
            printf("%s: rc %d\n", what, rc);
            return 1;
        }
    }
    for (size_t i = 0; i < ps.size(); ++i)
        printf("%s[%zu]: M %d status %d inliers %d best_h %d polish %d cost %.6g\n", what, i, ps[i].M, res[i].status,
               res[i].num_inliers, res[i].best_h, res[i].polish_iters, res[i].cost);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    std::vector<Prob> ps;
    ps.push_back(planted(200, 0.4, 512));
    ps.push_back(planted(3, 0.0, 16));
    ps.push_back(planted(4, 0.0, 64));
    ps.push_back(planted(5, 0.0, 64));
    Prob line = planted(40, 0.0, 128);  // collinear
    for (int i = 0; i < 40; ++i) {
        line.p3[3 * i] = 1.0 + i;
        line.p3[3 * i + 1] = 2.0 + 2.0 * i;
        line.p3[3 * i + 2] = 30.0 + 4.0 * i;
    }
    ps.push_back(line);
    Prob nonfinite = planted(100, 0.3, 256);
    nonfinite.p3[4] = NAN;
    nonfinite.p2[20] = INFINITY;
    nonfinite.p3[50] = -INFINITY;
    ps.push_back(nonfinite);
    Prob all_nan = planted(50, 0.0, 64);
    for (double &v : all_nan.p3) v = NAN;
    ps.push_back(all_nan);
    Prob same = planted(50, 0.0, 64);
    for (int i = 1; i < 50; ++i) memcpy(&same.p3[3 * i], &same.p3[0], 3 * sizeof(double));
    ps.push_back(same);
    Prob distorted = planted(120, 0.3, 256);
    const double dist[4] = {-0.1, 0.02, 1e-3, -1e-3};
    memcpy(distorted.dist, dist, sizeof dist);
    ps.push_back(distorted);
    int bad = run(ps, "builtin");

    // a bad coefficient count and bad arguments are refused
    fmpnp_pnp_problem d;
    memset(&d, 0, sizeof d);
    d.M = 0;
    d.iters = 1;
    d.n_dist = 5;
    fmpnp_pnp_result r;
    bad |= fmpnp_pnp_ransac_cpu(&d, 1, &r, nullptr, 0, 1) != FMPNP_EINVAL;
    bad |= fmpnp_pnp_ransac_cpu(nullptr, 1, &r, nullptr, 0, 1) != FMPNP_EINVAL;

    // P3P alone: a regular triple, a collinear one, two equal points
    const double tri[3][9] = {{0, 0, 10, 1, 2, 12, -2, 1, 14}, {0, 0, 10, 1, 2, 12, 2, 4, 14}, {0, 0, 10, 0, 0, 10, 2, -1, 14}};
    for (int k = 0; k < 3; ++k) {
        double y[9], R[36], t[12];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) y[3 * i + j] = tri[k][3 * i + j] / tri[k][3 * i + 2];
        const int n = fmpnp_p3p_cpu(y, tri[k], R, t);
        printf("p3p[%d]: %d solutions\n", k, n);
        bad |= n < 0 || n > 4 || (k == 0 && n < 1);
        for (int i = 0; i < 9 * n; ++i) bad |= !(R[i] - R[i] == 0.0);
    }

    if (argc > 1) {
        FILE *f = fopen(argv[1], "rb");
        if (!f) {
            printf("cannot open %s\n", argv[1]);
            return 2;
        }
        int32_t n = 0;
        if (fread(&n, 4, 1, f) != 1 || n < 0 || n > 4096) return 2;
        std::vector<Prob> fs((size_t)n);
        for (Prob &p : fs) {
            int32_t hdr[2];
            if (fread(hdr, 4, 2, f) != 2 || hdr[0] < 0 || hdr[0] > (1 << 20)) return 2;
            p.M = hdr[0];
            p.iters = hdr[1];
            p.p3.resize(3 * (size_t)p.M);
            p.p2.resize(2 * (size_t)p.M);
            if (fread(p.K, 8, 9, f) != 9 || fread(p.dist, 8, 4, f) != 4 || fread(&p.thr, 8, 1, f) != 1) return 2;
            if (fread(p.p3.data(), 8, p.p3.size(), f) != p.p3.size()) return 2;
            if (fread(p.p2.data(), 8, p.p2.size(), f) != p.p2.size()) return 2;
        }
        fclose(f);
        bad |= run(fs, "file");
    }
    printf(bad ? "FAILED\n" : "OK\n");
    return bad;
}
