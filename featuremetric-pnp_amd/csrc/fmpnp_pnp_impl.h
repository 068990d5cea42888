// fmpnp_pnp_impl.h -- the arithmetic of the P3P RANSAC + polish stage (include/fmpnp.h, "initial
// pose"), as __host__ __device__ functions: the camera model, the sampler, Lambda Twist, the point
// test and the polish step.  fmpnp_pnp.hip (the kernels) and fmpnp_pnp_cpu.cpp (the twin) both
// include this file and nothing else computes a value, so the two agree bit for bit as long as each
// operation rounds the same way on both sides: every + - * / sqrt here is one IEEE fp64 operation
// (contraction is off from here to the end of the including unit; the only fused operations are the
// explicit fma() of so3_coeffs_small), and every branch depends on those values alone.
#pragma once
#include "fmpnp_device.h"

#pragma clang fp contract(off)

namespace fmpnp {
namespace pnp {

#define FMPNP_HD __host__ __device__ inline

constexpr int UNDISTORT_ITERS = 10;    // fixed-point iterations of undistort()
constexpr int CUBIC_MIN_ITERS = 7;     // Newton steps on Lambda Twist's cubic: at least, at most
constexpr int CUBIC_MAX_ITERS = 50;
constexpr int LAMBDA_REFINE_ITERS = 5; // Gauss-Newton steps on the three depths
constexpr int POLISH_MAX_ITERS = 100;  // trial poses evaluated by the polish, at most
constexpr int POLISH_LANES = 256;      // partial sums of the polish's reduction (the workgroup size)
constexpr int NACC = 28;               // 21 upper-triangle entries of J^T J, 6 of J^T r, the cost

FMPNP_HD bool finite_d(double x) { return (x - x) == 0.0; }

struct Cam {
    double fx, fy, cx, cy, k1, k2, p1, p2;
    int nodist;  // all four coefficients are zero: distort() is the identity, bit for bit
};

FMPNP_HD Cam make_cam(const double *K, const double *dist) {
    Cam c;
    c.fx = K[0];
    c.fy = K[4];
    c.cx = K[2];
    c.cy = K[5];
    c.k1 = dist[0];
    c.k2 = dist[1];
    c.p1 = dist[2];
    c.p2 = dist[3];
    c.nodist = (c.k1 == 0.0 && c.k2 == 0.0 && c.p1 == 0.0 && c.p2 == 0.0) ? 1 : 0;
    return c;
}

// OpenCV's forward model on normalised coordinates: radial k1, k2 and tangential p1, p2 (ND: the
// caller knows c.nodist at compile time; the values are the same either way)
template <bool ND>
FMPNP_HD void distort_t(const Cam &c, double x, double y, double &xd, double &yd) {
    if (ND) {
        xd = x;
        yd = y;
        return;
    }
    const double r2 = x * x + y * y;
    const double rad = 1.0 + (c.k1 * r2 + (c.k2 * r2) * r2);
    const double xy = x * y;
    xd = x * rad + ((2.0 * c.p1) * xy + c.p2 * (r2 + 2.0 * (x * x)));
    yd = y * rad + (c.p1 * (r2 + 2.0 * (y * y)) + (2.0 * c.p2) * xy);
}
FMPNP_HD void distort(const Cam &c, double x, double y, double &xd, double &yd) {
    if (c.nodist)
        distort_t<true>(c, x, y, xd, yd);
    else
        distort_t<false>(c, x, y, xd, yd);
}

// pixel -> undistorted normalised coordinates: UNDISTORT_ITERS rounds of x <- (x0 - dx(x)) / rad(x)
FMPNP_HD void undistort(const Cam &c, double u, double v, double &x, double &y) {
    const double x0 = (u - c.cx) / c.fx, y0 = (v - c.cy) / c.fy;
    x = x0;
    y = y0;
    if (c.nodist) return;
    for (int it = 0; it < UNDISTORT_ITERS; ++it) {
        const double r2 = x * x + y * y;
        const double icd = 1.0 / (1.0 + (c.k1 * r2 + (c.k2 * r2) * r2));
        const double xy = x * y;
        const double dx = (2.0 * c.p1) * xy + c.p2 * (r2 + 2.0 * (x * x));
        const double dy = c.p1 * (r2 + 2.0 * (y * y)) + (2.0 * c.p2) * xy;
        x = (x0 - dx) * icd;
        y = (y0 - dy) * icd;
    }
}

// ---- sampling ------------------------------------------------------------------------------------
// splitmix64's output function at stream position n of state `seed`
FMPNP_HD unsigned long long mix64(unsigned long long seed, unsigned long long n) {
    unsigned long long z = seed + 0x9E3779B97F4A7C15ull * n;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// Four distinct indices of [0, M), M >= 4: draw j takes r_j = (hi32(mix64(seed, 4 h + j + 1)) * (M - j)) >> 32
// and selects the r_j-th index not yet taken, in ascending order.  Exactly four draws for every M.
FMPNP_HD void sample4(unsigned long long seed, unsigned h, int M, int s[4]) {
    int taken[4];  // ascending
    for (int j = 0; j < 4; ++j) {
        const unsigned long long z = mix64(seed, 4ull * h + (unsigned)j + 1ull);
        int idx = (int)(((z >> 32) * (unsigned long long)(unsigned)(M - j)) >> 32);
        int pos = 0;
        for (int i = 0; i < j; ++i)
            if (idx >= taken[i]) {
                ++idx;
                pos = i + 1;
            }
        s[j] = idx;
        for (int i = j; i > pos; --i) taken[i] = taken[i - 1];
        taken[pos] = idx;
    }
}

// ---- Lambda Twist (Persson & Nordberg, ECCV 2018) ----------------------------------------------
// a real root of x^3 + b x^2 + c x + d by Newton steps from the paper's starting point
FMPNP_HD double cubick(double b, double c, double d) {
    double r0;
    if (b * b >= 3.0 * c) {
        const double v = sqrt(b * b - 3.0 * c);
        const double t1 = (-b - v) / 3.0;
        double k = ((t1 + b) * t1 + c) * t1 + d;
        if (k > 0.0) {
            r0 = t1 - sqrt(-k / (3.0 * t1 + b));
        } else {
            const double t2 = (-b + v) / 3.0;
            k = ((t2 + b) * t2 + c) * t2 + d;
            r0 = t2 + sqrt(-k / (3.0 * t2 + b));
        }
    } else {
        r0 = -b / 3.0;
        if (fabs((3.0 * r0 + 2.0 * b) * r0 + c) < 1e-4) r0 += 1.0;
    }
    for (int cnt = 0; cnt < CUBIC_MAX_ITERS; ++cnt) {
        const double fx = ((r0 + b) * r0 + c) * r0 + d;
        if (cnt < CUBIC_MIN_ITERS || fabs(fx) > 1e-13) {
            const double fpx = (3.0 * r0 + 2.0 * b) * r0 + c;
            r0 -= fx / fpx;
        } else {
            break;
        }
    }
    return r0;
}

// the roots of x^2 + b x + c (both 0.5 b when there is none)
FMPNP_HD bool root2real(double b, double c, double &r1, double &r2) {
    const double v = b * b - 4.0 * c;
    if (v < 0.0) {
        r1 = r2 = 0.5 * b;
        return false;
    }
    const double y = sqrt(v);
    if (b < 0.0) {
        r1 = 0.5 * (-b + y);
        r2 = 0.5 * (-b - y);
    } else {
        r1 = 2.0 * c / (-b + y);
        r2 = 2.0 * c / (-b - y);
    }
    return true;
}

// eigenvalues e1, e2 (|e1| >= |e2|) and unit eigenvectors v1, v2 of a symmetric 3x3 matrix (upper
// triangle x00 .. x22) whose third eigenvalue is 0
FMPNP_HD void eig_known0(double x00, double x01, double x02, double x11, double x12, double x22, double &e1,
                         double &e2, double v1[3], double v2[3]) {
    const double x01s = x01 * x01;
    const double b = -x00 - x11 - x22;
    const double c = -x01s - x02 * x02 - x12 * x12 + x00 * (x11 + x22) + x11 * x22;
    root2real(b, c, e1, e2);
    if (fabs(e1) < fabs(e2)) {
        const double s = e1;
        e1 = e2;
        e2 = s;
    }
    const double mx0011 = -x00 * x11;
    const double prec0 = x01 * x12 - x02 * x11;
    const double prec1 = x01 * x02 - x00 * x12;
    for (int k = 0; k < 2; ++k) {
        const double e = k ? e2 : e1;
        double *v = k ? v2 : v1;
        const double tmp = 1.0 / (e * (x00 + x11) + mx0011 - e * e + x01s);
        double a1 = -(e * x02 + prec0) * tmp;
        double a2 = -(e * x12 + prec1) * tmp;
        const double rn = 1.0 / sqrt(a1 * a1 + a2 * a2 + 1.0);
        v[0] = a1 * rn;
        v[1] = a2 * rn;
        v[2] = rn;
    }
}

FMPNP_HD void refine_lambda(double L[3], double a12, double a13, double a23, double b12, double b13, double b23) {
    for (int i = 0; i < LAMBDA_REFINE_ITERS; ++i) {
        const double l1 = L[0], l2 = L[1], l3 = L[2];
        const double r1 = l1 * l1 + l2 * l2 + b12 * l1 * l2 - a12;
        const double r2 = l1 * l1 + l3 * l3 + b13 * l1 * l3 - a13;
        const double r3 = l2 * l2 + l3 * l3 + b23 * l2 * l3 - a23;
        if (fabs(r1) + fabs(r2) + fabs(r3) < 1e-10) break;
        const double v0 = 2.0 * l1 + b12 * l2, v1 = 2.0 * l2 + b12 * l1;
        const double v3 = 2.0 * l1 + b13 * l3, v5 = 2.0 * l3 + b13 * l1;
        const double v7 = 2.0 * l2 + b23 * l3, v8 = 2.0 * l3 + b23 * l2;
        const double det = 1.0 / (-v0 * v5 * v7 - v1 * v3 * v8);
        const double n1 = l1 - det * ((-v5 * v7) * r1 + (-v1 * v8) * r2 + (v1 * v5) * r3);
        const double n2 = l2 - det * ((-v3 * v8) * r1 + (v0 * v8) * r2 + (-v0 * v5) * r3);
        const double n3 = l3 - det * ((v3 * v7) * r1 + (-v0 * v7) * r2 + (-v1 * v3) * r3);
        const double q1 = n1 * n1 + n2 * n2 + b12 * n1 * n2 - a12;
        const double q2 = n1 * n1 + n3 * n3 + b13 * n1 * n3 - a13;
        const double q3 = n2 * n2 + n3 * n3 + b23 * n2 * n3 - a23;
        if (fabs(q1) + fabs(q2) + fabs(q3) > fabs(r1) + fabs(r2) + fabs(r3)) break;
        L[0] = n1;
        L[1] = n2;
        L[2] = n3;
    }
}

// P3P: bearings yin[3][3] (any positive length; normalised here) of the world points x[3][3].
// Writes the solutions (R row-major, t: lambda_i y_i = R x_i + t) that are finite, have three
// positive depths and an orthonormal R (|R R^T - I| <= 1e-6 entrywise: a degenerate triple's
// "solutions" are not rotations), in the order (+v, tau1), (+v, tau2), (-v, tau1), (-v, tau2).
// Returns their number, 0..4.
FMPNP_HD int p3p(const double yin[3][3], const double x[3][3], double R[4][9], double t[4][3]) {
    double y[3][3];
    for (int i = 0; i < 3; ++i) {
        const double n = 1.0 / sqrt(yin[i][0] * yin[i][0] + yin[i][1] * yin[i][1] + yin[i][2] * yin[i][2]);
        for (int k = 0; k < 3; ++k) y[i][k] = yin[i][k] * n;
    }
    const double b12 = -2.0 * (y[0][0] * y[1][0] + y[0][1] * y[1][1] + y[0][2] * y[1][2]);
    const double b13 = -2.0 * (y[0][0] * y[2][0] + y[0][1] * y[2][1] + y[0][2] * y[2][2]);
    const double b23 = -2.0 * (y[1][0] * y[2][0] + y[1][1] * y[2][1] + y[1][2] * y[2][2]);
    double d12[3], d13[3], d23[3], dx[3];
    for (int k = 0; k < 3; ++k) {
        d12[k] = x[0][k] - x[1][k];
        d13[k] = x[0][k] - x[2][k];
        d23[k] = x[1][k] - x[2][k];
    }
    dx[0] = d12[1] * d13[2] - d12[2] * d13[1];
    dx[1] = d12[2] * d13[0] - d12[0] * d13[2];
    dx[2] = d12[0] * d13[1] - d12[1] * d13[0];
    const double a12 = d12[0] * d12[0] + d12[1] * d12[1] + d12[2] * d12[2];
    const double a13 = d13[0] * d13[0] + d13[1] * d13[1] + d13[2] * d13[2];
    const double a23 = d23[0] * d23[0] + d23[1] * d23[1] + d23[2] * d23[2];

    const double c31 = -0.5 * b13, c23 = -0.5 * b23, c12 = -0.5 * b12;
    const double blob = c12 * c23 * c31 - 1.0;
    const double s31 = 1.0 - c31 * c31, s23 = 1.0 - c23 * c23, s12 = 1.0 - c12 * c12;
    double p3 = a13 * (a23 * s31 - a13 * s23);
    double p2 = 2.0 * blob * a23 * a13 + a13 * (2.0 * a12 + a13) * s23 + a23 * (a23 - a12) * s31;
    double p1 = a23 * (a13 - a23) * s12 - a12 * a12 * s23 - 2.0 * a12 * (blob * a23 + a13 * s23);
    double p0 = a12 * (a12 * s23 - a23 * s12);
    p3 = 1.0 / p3;
    p2 *= p3;
    p1 *= p3;
    p0 *= p3;
    const double g = cubick(p2, p1, p0);

    const double A00 = a23 * (1.0 - g);
    const double A01 = (a23 * b12) * 0.5;
    const double A02 = (a23 * b13 * g) * (-0.5);
    const double A11 = a23 - a12 + a13 * g;
    const double A12 = b23 * (a13 * g - a12) * 0.5;
    const double A22 = g * (a13 - a23) - a12;
    double e1, e2, V0[3], V1[3];
    eig_known0(A00, A01, A02, A11, A12, A22, e1, e2, V0, V1);
    const double q = -e2 / e1;
    const double v = sqrt(q > 0.0 ? q : 0.0);

    double Ls[4][3];
    int cand = 0;
    for (int sgn = 0; sgn < 2; ++sgn) {
        const double s = sgn ? -v : v;
        const double w2 = 1.0 / (s * V1[0] - V0[0]);
        const double w0 = (V0[1] - s * V1[1]) * w2;
        const double w1 = (V0[2] - s * V1[2]) * w2;
        const double a = 1.0 / ((a13 - a12) * w1 * w1 - a12 * b13 * w1 - a12);
        const double b = (a13 * b12 * w1 - a12 * b13 * w0 - 2.0 * w0 * w1 * (a12 - a13)) * a;
        const double c = ((a13 - a12) * w0 * w0 + a13 * b12 * w0 + a13) * a;
        if (b * b - 4.0 * c >= 0.0) {
            double tau[2];
            root2real(b, c, tau[0], tau[1]);
            for (int k = 0; k < 2; ++k) {
                if (tau[k] > 0.0) {
                    const double d = a23 / (tau[k] * (b23 + tau[k]) + 1.0);
                    const double l2 = sqrt(d);
                    const double l3 = tau[k] * l2;
                    const double l1 = w0 * l2 + w1 * l3;
                    if (l1 >= 0.0) {
                        Ls[cand][0] = l1;
                        Ls[cand][1] = l2;
                        Ls[cand][2] = l3;
                        ++cand;
                    }
                }
            }
        }
    }
    if (cand == 0) return 0;

    // X = [d12 d13 d12xd13]^-1 by cofactors
    double Xi[9];
    {
        const double m00 = d12[0], m01 = d13[0], m02 = dx[0];
        const double m10 = d12[1], m11 = d13[1], m12 = dx[1];
        const double m20 = d12[2], m21 = d13[2], m22 = dx[2];
        const double c00 = m11 * m22 - m12 * m21, c01 = m12 * m20 - m10 * m22, c02 = m10 * m21 - m11 * m20;
        const double idet = 1.0 / (m00 * c00 + m01 * c01 + m02 * c02);
        Xi[0] = c00 * idet;
        Xi[1] = (m02 * m21 - m01 * m22) * idet;
        Xi[2] = (m01 * m12 - m02 * m11) * idet;
        Xi[3] = c01 * idet;
        Xi[4] = (m00 * m22 - m02 * m20) * idet;
        Xi[5] = (m02 * m10 - m00 * m12) * idet;
        Xi[6] = c02 * idet;
        Xi[7] = (m01 * m20 - m00 * m21) * idet;
        Xi[8] = (m00 * m11 - m01 * m10) * idet;
    }
    int valid = 0;
    for (int i = 0; i < cand; ++i) {
        refine_lambda(Ls[i], a12, a13, a23, b12, b13, b23);
        if (!(Ls[i][0] > 0.0 && Ls[i][1] > 0.0 && Ls[i][2] > 0.0)) continue;
        double ry1[3], yd1[3], yd2[3], yx[3];
        for (int k = 0; k < 3; ++k) {
            ry1[k] = y[0][k] * Ls[i][0];
            yd1[k] = ry1[k] - y[1][k] * Ls[i][1];
            yd2[k] = ry1[k] - y[2][k] * Ls[i][2];
        }
        yx[0] = yd1[1] * yd2[2] - yd1[2] * yd2[1];
        yx[1] = yd1[2] * yd2[0] - yd1[0] * yd2[2];
        yx[2] = yd1[0] * yd2[1] - yd1[1] * yd2[0];
        double *Ro = R[valid], *to = t[valid];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) Ro[3 * r + c] = yd1[r] * Xi[c] + yd2[r] * Xi[3 + c] + yx[r] * Xi[6 + c];
        bool ok = true;
        for (int r = 0; r < 3; ++r) {
            to[r] = ry1[r] - (Ro[3 * r] * x[0][0] + Ro[3 * r + 1] * x[0][1] + Ro[3 * r + 2] * x[0][2]);
            ok = ok && finite_d(to[r]);
            for (int c = r; c < 3; ++c) {
                const double dot = Ro[3 * r] * Ro[3 * c] + Ro[3 * r + 1] * Ro[3 * c + 1] + Ro[3 * r + 2] * Ro[3 * c + 2];
                ok = ok && fabs(dot - (r == c ? 1.0 : 0.0)) <= 1e-6;  // (false for NaN / Inf)
            }
        }
        if (ok) ++valid;
    }
    return valid;
}

// ---- the point test ------------------------------------------------------------------------------
// squared reprojection error of X under (R, t) with the forward model; false when the depth is not > 0
// (e2 is then meaningless).  Straight-line code: the callers' loops over points unroll.
template <bool ND>
FMPNP_HD bool point_err2_t(const Cam &c, const double *R, const double *t, double X0, double X1, double X2, double u,
                           double v, double &e2) {
    const double P0 = ((R[0] * X0 + R[1] * X1) + R[2] * X2) + t[0];
    const double P1 = ((R[3] * X0 + R[4] * X1) + R[5] * X2) + t[1];
    const double P2 = ((R[6] * X0 + R[7] * X1) + R[8] * X2) + t[2];
    const double iz = 1.0 / P2;
    double xd, yd;
    distort_t<ND>(c, P0 * iz, P1 * iz, xd, yd);
    const double du = (c.fx * xd + c.cx) - u, dv = (c.fy * yd + c.cy) - v;
    e2 = du * du + dv * dv;
    return P2 > 0.0;
}
FMPNP_HD bool point_err2(const Cam &c, const double *R, const double *t, double X0, double X1, double X2, double u,
                         double v, double &e2) {
    return c.nodist ? point_err2_t<true>(c, R, t, X0, X1, X2, u, v, e2)
                    : point_err2_t<false>(c, R, t, X0, X1, X2, u, v, e2);
}
// the point test with c.nodist known at compile time (the hypothesis kernel's loop)
template <bool ND>
FMPNP_HD bool is_inlier_t(const Cam &c, const double *R, const double *t, const double *X, const double *x,
                          double thr2) {
    double e2;
    const bool front = point_err2_t<ND>(c, R, t, X[0], X[1], X[2], x[0], x[1], e2);
    return front & (e2 <= thr2);
}
FMPNP_HD bool is_inlier(const Cam &c, const double *R, const double *t, const double *X, const double *x,
                        double thr2) {
    double e2;
    return point_err2(c, R, t, X[0], X[1], X[2], x[0], x[1], e2) && e2 <= thr2;
}

// Hypothesis h of a problem: sample, P3P on the first three points, the fourth picks the solution
// (the smallest squared reprojection error among those that put it at positive depth; the lowest
// solution index on a tie).  false: no model.
FMPNP_HD bool hypothesis(const Cam &c, const double *p3, const double *p2, int M, unsigned long long seed,
                         unsigned h, double R[9], double t[3]) {
    int s[4];
    sample4(seed, h, M, s);
    double y[3][3], x[3][3];
    for (int i = 0; i < 3; ++i) {
        undistort(c, p2[2 * (size_t)s[i]], p2[2 * (size_t)s[i] + 1], y[i][0], y[i][1]);
        y[i][2] = 1.0;
        for (int k = 0; k < 3; ++k) x[i][k] = p3[3 * (size_t)s[i] + k];
    }
    double Rs[4][9], ts[4][3];
    const int n = p3p(y, x, Rs, ts);
    const double *X4 = p3 + 3 * (size_t)s[3], *x4 = p2 + 2 * (size_t)s[3];
    const double X40 = X4[0], X41 = X4[1], X42 = X4[2], u4 = x4[0], v4 = x4[1];
    double best = __builtin_inf();
    int bi = -1;
    for (int i = 0; i < n; ++i) {
        double e2;
        if (point_err2(c, Rs[i], ts[i], X40, X41, X42, u4, v4, e2) && e2 < best) {
            best = e2;
            bi = i;
        }
    }
    if (bi < 0) return false;
    for (int k = 0; k < 9; ++k) R[k] = Rs[bi][k];
    for (int k = 0; k < 3; ++k) t[k] = ts[bi][k];
    return true;
}

FMPNP_HD unsigned long long pack_key(int count, unsigned h) {
    return ((unsigned long long)(unsigned)count << 32) | (unsigned long long)(unsigned)~h;
}

// ---- polish --------------------------------------------------------------------------------------
// acc += this point's J^T J (upper triangle, row-major: (0,0) (0,1) .. (0,5) (1,1) ..), J^T r and
// |r|^2; parameters (w, dt) of the update R <- exp([w]x) R, t <- t + dt
FMPNP_HD void polish_point(const Cam &c, const double *R, const double *t, const double *X, const double *x,
                           double acc[NACC]) {
    const double Q0 = (R[0] * X[0] + R[1] * X[1]) + R[2] * X[2];
    const double Q1 = (R[3] * X[0] + R[4] * X[1]) + R[5] * X[2];
    const double Q2 = (R[6] * X[0] + R[7] * X[1]) + R[8] * X[2];
    const double P0 = Q0 + t[0], P1 = Q1 + t[1], P2 = Q2 + t[2];
    const double iz = 1.0 / P2;
    const double xn = P0 * iz, yn = P1 * iz;
    double xd, yd, axx = 1.0, axy = 0.0, ayx = 0.0, ayy = 1.0;
    distort(c, xn, yn, xd, yd);
    if (!c.nodist) {
        const double r2 = xn * xn + yn * yn;
        const double rad = 1.0 + (c.k1 * r2 + (c.k2 * r2) * r2);
        const double q2 = 2.0 * (c.k1 + (2.0 * c.k2) * r2);
        const double cross = (q2 * xn) * yn + ((2.0 * c.p1) * xn + (2.0 * c.p2) * yn);
        axx = (rad + (q2 * xn) * xn) + ((2.0 * c.p1) * yn + (6.0 * c.p2) * xn);
        axy = cross;
        ayx = cross;
        ayy = (rad + (q2 * yn) * yn) + ((6.0 * c.p1) * yn + (2.0 * c.p2) * xn);
    }
    const double ru = (c.fx * xd + c.cx) - x[0], rv = (c.fy * yd + c.cy) - x[1];
    // d(u, v) / dP
    const double nx0 = iz, nx2 = -(xn * iz), ny1 = iz, ny2 = -(yn * iz);
    const double ju0 = c.fx * (axx * nx0), ju1 = c.fx * (axy * ny1), ju2 = c.fx * (axx * nx2 + axy * ny2);
    const double jv0 = c.fy * (ayx * nx0), jv1 = c.fy * (ayy * ny1), jv2 = c.fy * (ayx * nx2 + ayy * ny2);
    // dP / dw_j = e_j x Q
    double Ju[6], Jv[6];
    Ju[0] = ju2 * Q1 - ju1 * Q2;
    Ju[1] = ju0 * Q2 - ju2 * Q0;
    Ju[2] = ju1 * Q0 - ju0 * Q1;
    Ju[3] = ju0;
    Ju[4] = ju1;
    Ju[5] = ju2;
    Jv[0] = jv2 * Q1 - jv1 * Q2;
    Jv[1] = jv0 * Q2 - jv2 * Q0;
    Jv[2] = jv1 * Q0 - jv0 * Q1;
    Jv[3] = jv0;
    Jv[4] = jv1;
    Jv[5] = jv2;
    int k = 0;
    for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b, ++k) acc[k] = acc[k] + (Ju[a] * Ju[b] + Jv[a] * Jv[b]);
    for (int a = 0; a < 6; ++a) acc[21 + a] = acc[21 + a] + (Ju[a] * ru + Jv[a] * rv);
    acc[27] = acc[27] + (ru * ru + rv * rv);
}

// (H + lambda diag H) d = -g by Cholesky; false when a pivot is not > 0 or d is not finite
FMPNP_HD bool solve6(const double S[NACC], double lambda, double d[6]) {
    double L[6][6];
    int k = 0;
    for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b, ++k) L[b][a] = S[k];
    for (int a = 0; a < 6; ++a) L[a][a] = L[a][a] + lambda * L[a][a];
    for (int j = 0; j < 6; ++j) {
        double s = L[j][j];
        for (int m = 0; m < j; ++m) s = s - L[j][m] * L[j][m];
        if (!(s > 0.0)) return false;
        const double dj = sqrt(s);
        L[j][j] = dj;
        for (int i = j + 1; i < 6; ++i) {
            double v = L[i][j];
            for (int m = 0; m < j; ++m) v = v - L[i][m] * L[j][m];
            L[i][j] = v / dj;
        }
    }
    double z[6];
    for (int i = 0; i < 6; ++i) {
        double v = -S[21 + i];
        for (int m = 0; m < i; ++m) v = v - L[i][m] * z[m];
        z[i] = v / L[i][i];
    }
    bool ok = true;
    for (int i = 5; i >= 0; --i) {
        double v = z[i];
        for (int m = i + 1; m < 6; ++m) v = v - L[m][i] * d[m];
        d[i] = v / L[i][i];
        ok = ok && finite_d(d[i]);
    }
    return ok;
}

// R' = exp([w]x) R, t' = t + dt; false when |w|^2 > 0.6 (beyond so3_coeffs_small's range)
FMPNP_HD bool apply_step(const double *R, const double *t, const double d[6], double Rn[9], double tn[3]) {
    const double z = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
    if (!(z <= 0.6)) return false;
    double cz, az, bz;
    so3_coeffs_small(z, cz, az, bz);
    double E[9];
    E[0] = cz + bz * (d[0] * d[0]);
    E[1] = bz * (d[0] * d[1]) - az * d[2];
    E[2] = bz * (d[0] * d[2]) + az * d[1];
    E[3] = bz * (d[1] * d[0]) + az * d[2];
    E[4] = cz + bz * (d[1] * d[1]);
    E[5] = bz * (d[1] * d[2]) - az * d[0];
    E[6] = bz * (d[2] * d[0]) - az * d[1];
    E[7] = bz * (d[2] * d[1]) + az * d[0];
    E[8] = cz + bz * (d[2] * d[2]);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) Rn[3 * r + c] = (E[3 * r] * R[c] + E[3 * r + 1] * R[3 + c]) + E[3 * r + 2] * R[6 + c];
    for (int k = 0; k < 3; ++k) tn[k] = t[k] + d[3 + k];
    return true;
}

// The polish: Levenberg-Marquardt on the fixed inlier set from (Rh, th).  eval(R, t, S) fills S with
// the NACC sums over the inliers in the fixed order of include/fmpnp.h; every caller of one problem
// (the lanes of a workgroup, or the twin's one thread) runs this same sequence.  lambda starts at
// 1e-3; an accepted step (strictly smaller finite cost) divides it by 10 (not below 1e-15), a
// rejected or unsolvable one multiplies it by 10.  Stop: |d|^2 <= 1e-24 before the step is tried,
// lambda > 1e12, or POLISH_MAX_ITERS trial evaluations.  Returns false (the caller reports
// FMPNP_PNP_POLISH_FAILED and the hypothesis) when the cost at (Rh, th) is not finite or the damped
// system stays unsolvable up to lambda = 1e12.
template <class Eval>
__host__ __device__ inline bool polish(Eval &eval, const double Rh[9], const double th[3], double R[9], double t[3],
                                       double &cost, int &iters) {
    double S[NACC], Sn[NACC], Rn[9], tn[3], d[6];
    for (int k = 0; k < 9; ++k) R[k] = Rh[k];
    for (int k = 0; k < 3; ++k) t[k] = th[k];
    eval(R, t, S);
    const double cost0 = S[27];
    cost = cost0;
    iters = 0;
    if (!finite_d(cost0)) return false;
    double lam = 1e-3;
    while (iters < POLISH_MAX_ITERS) {
        if (!solve6(S, lam, d)) {
            lam = lam * 10.0;
            if (lam > 1e12) {
                cost = cost0;
                return false;
            }
            continue;
        }
        double n2 = 0.0;
        for (int k = 0; k < 6; ++k) n2 = n2 + d[k] * d[k];
        if (n2 <= 1e-24) break;
        bool better = false;
        if (apply_step(R, t, d, Rn, tn)) {
            ++iters;
            eval(Rn, tn, Sn);
            better = Sn[27] < S[27];
        }
        if (better) {
            for (int k = 0; k < NACC; ++k) S[k] = Sn[k];
            for (int k = 0; k < 9; ++k) R[k] = Rn[k];
            for (int k = 0; k < 3; ++k) t[k] = tn[k];
            lam = lam * 0.1;
            if (lam < 1e-15) lam = 1e-15;
        } else {
            lam = lam * 10.0;
            if (lam > 1e12) break;
        }
    }
    cost = S[27];
    return true;
}

}  // namespace pnp
}  // namespace fmpnp
