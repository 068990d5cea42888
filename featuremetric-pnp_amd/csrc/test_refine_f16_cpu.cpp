// Stand-alone host program over the binary16 storage of the refiner's CPU twin (fmpnp_cpu.cpp linked in), for
// sanitizer runs outside Python: `make refine-f16-sanitize` builds it with ASan + UBSan and runs it.
//   1. fmpnp::host::half_bits_to_float (fmpnp_host.h) on all 65 536 bit patterns against the compiler's own
//      _Float16 -> float conversion (bit for bit; NaNs by class, sign and payload).
//   2. fmpnp_refine_batch_cpu with FMPNP_F16 on one tiny problem in exactly-sized heap buffers (a read one
//      element outside the map or the descriptors is an ASan report): its results equal, field for field, the
//      FMPNP_F32 twin's on the same values widened (the twin's channel sums run in one order for every storage
//      type); a channel range that starts off a multiple of 8; compute_cost; and the argument errors.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "fmpnp.h"
#include "fmpnp_host.h"

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

uint16_t narrow(float v) {  // the compiler's fp32 -> binary16 (round to nearest even)
    const _Float16 h = (_Float16)v;
    uint16_t b;
    memcpy(&b, &h, 2);
    return b;
}

void sweep_widening() {
    int bad = 0;
    for (uint32_t b = 0; b < 65536; ++b) {
        const uint16_t hb = (uint16_t)b;
        _Float16 h;
        memcpy(&h, &hb, 2);
        const float want = (float)h, got = fmpnp::host::half_bits_to_float(hb);
        uint32_t wb, gb;
        memcpy(&wb, &want, 4);
        memcpy(&gb, &got, 4);
        if (wb != gb && ++bad < 8) printf("  pattern %04x: %08x, expected %08x\n", b, gb, wb);
    }
    CHECK(bad == 0);
}

constexpr int C = 13, CS = 16, HF = 6, WF = 8, N = 9, IM_W = 32, IM_H = 24, ITERS = 8;

struct Case {
    std::vector<uint16_t> map16, ref16;
    std::vector<float> map32, ref32;
    std::vector<double> pts;
    fmpnp_problem p16, p32;
};

void make_case(Case &c) {
    c.map16.assign((size_t)HF * WF * 3 * CS, 0);
    c.map32.assign(c.map16.size(), 0.f);
    c.ref16.assign((size_t)N * CS, 0);
    c.ref32.assign(c.ref16.size(), 0.f);
    for (int t = 0; t < HF * WF; ++t)
        for (int pl = 0; pl < 3; ++pl)
            for (int ch = 0; ch < C; ++ch) {
                // f in [0, 1), gradients in [-4, 4); a few subnormal and zero values
                double v = pl == 0 ? uni() : 8.0 * uni() - 4.0;
                if ((t + ch) % 17 == 0) v *= 1e-6;
                const size_t at = ((size_t)t * 3 + pl) * CS + ch;
                c.map16[at] = narrow((float)v);
                c.map32[at] = fmpnp::host::half_bits_to_float(c.map16[at]);
            }
    for (int i = 0; i < N; ++i)
        for (int ch = 0; ch < C; ++ch) {
            c.ref16[(size_t)i * CS + ch] = narrow((float)uni());
            c.ref32[(size_t)i * CS + ch] = fmpnp::host::half_bits_to_float(c.ref16[(size_t)i * CS + ch]);
        }
    c.pts.resize(3 * (size_t)N);
    for (int i = 0; i < N; ++i) {
        c.pts[3 * i] = 1.6 * uni() - 0.8;
        c.pts[3 * i + 1] = 1.2 * uni() - 0.6;
        c.pts[3 * i + 2] = 2.0 + uni();
    }
    fmpnp_problem p;
    memset(&p, 0, sizeof(p));
    p.pts3d = c.pts.data();
    p.N = N;
    p.Hf = HF;
    p.Wf = WF;
    p.cstride = CS;
    p.ld_ref = CS;
    p.c_begin = 0;
    p.c_end = C;
    p.im_width = IM_W;
    p.im_height = IM_H;
    const double K[9] = {20.0, 0.0, 16.0, 0.0, 20.0, 12.0, 0.0, 0.0, 1.0};
    const double R0[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t0[3] = {0.05, -0.04, 0.1};
    memcpy(p.K, K, sizeof(K));
    memcpy(p.R0, R0, sizeof(R0));
    memcpy(p.t0, t0, sizeof(t0));
    c.p16 = c.p32 = p;
    c.p16.feat = c.map16.data();
    c.p16.fref = c.ref16.data();
    c.p32.feat = c.map32.data();
    c.p32.fref = c.ref32.data();
}

fmpnp_options options(int dtype, int mode, int loss, int ratio) {
    fmpnp_options o;
    memset(&o, 0, sizeof(o));
    o.mode = mode;
    o.n_iters = ITERS;
    o.lambda0 = 0.01;
    o.use_ratio = ratio;
    o.ratio_threshold = 0.8;
    o.loss = loss;
    o.sampling = FMPNP_NEAREST;
    o.dtype = dtype;
    o.layout = FMPNP_LAYOUT_FGRAD;
    return o;
}

bool same_bits(double a, double b) { return memcmp(&a, &b, 8) == 0; }

void compare(const Case &c, int mode, int loss, int ratio, int cb, int ce) {
    fmpnp_problem a = c.p16, b = c.p32;
    a.c_begin = b.c_begin = cb;
    a.c_end = b.c_end = ce;
    const fmpnp_options o16 = options(FMPNP_F16, mode, loss, ratio), o32 = options(FMPNP_F32, mode, loss, ratio);
    fmpnp_result r16, r32;
    std::vector<fmpnp_trace_entry> t16(ITERS + 1), t32(ITERS + 1);
    CHECK(fmpnp_refine_batch_cpu(&a, 1, &o16, &r16, t16.data(), ITERS + 1, 1) == 0);
    CHECK(fmpnp_refine_batch_cpu(&b, 1, &o32, &r32, t32.data(), ITERS + 1, 1) == 0);
    CHECK(r16.n_evals == r32.n_evals && r16.n_steps == r32.n_steps && r16.n_accepted == r32.n_accepted);
    CHECK(r16.status == r32.status && r16.best_num_inliers == r32.best_num_inliers);
    CHECK(r16.texel_gathers == r32.texel_gathers && r16.n_evals >= 1);
    CHECK(same_bits(r16.initial_cost, r32.initial_cost) && same_bits(r16.best_cost, r32.best_cost));
    for (int k = 0; k < 9; ++k) CHECK(same_bits(r16.R[k], r32.R[k]));
    for (int k = 0; k < 3; ++k) CHECK(same_bits(r16.t[k], r32.t[k]));
    if (mode == FMPNP_MODE_FORWARD)
        for (int e = 0; e < r16.n_evals; ++e)
            CHECK(same_bits(t16[e].cost, t32[e].cost) && t16[e].n_supported == t32[e].n_supported &&
                  t16[e].n_kept == t32[e].n_kept);
}

void errors(const Case &c) {
    fmpnp_result r;
    fmpnp_options o = options(FMPNP_F16, FMPNP_MODE_FORWARD, FMPNP_GEMAN_MCCLURE, 0);
    o.sampling = FMPNP_BILINEAR;
    CHECK(fmpnp_refine_batch_cpu(&c.p16, 1, &o, &r, nullptr, 0, 1) == FMPNP_EINVAL);
    o.sampling = FMPNP_NEAREST;
    o.layout = FMPNP_LAYOUT_F;
    CHECK(fmpnp_refine_batch_cpu(&c.p16, 1, &o, &r, nullptr, 0, 1) == FMPNP_EINVAL);
    o.layout = FMPNP_LAYOUT_FGRAD;
    fmpnp_problem p = c.p16;
    p.cstride = 12;  // (never read: the strides are checked first)
    p.c_end = 12;
    CHECK(fmpnp_refine_batch_cpu(&p, 1, &o, &r, nullptr, 0, 1) == FMPNP_EALIGN);
    p = c.p16;
    p.ld_ref = 20;
    CHECK(fmpnp_refine_batch_cpu(&p, 1, &o, &r, nullptr, 0, 1) == FMPNP_EALIGN);
    o.dtype = 3;
    CHECK(fmpnp_refine_batch_cpu(&c.p16, 1, &o, &r, nullptr, 0, 1) == FMPNP_EINVAL);
}

}  // namespace

int main() {
    sweep_widening();
    Case c;
    make_case(c);
    compare(c, FMPNP_MODE_FORWARD, FMPNP_GEMAN_MCCLURE, 0, 0, C);
    compare(c, FMPNP_MODE_FORWARD, FMPNP_CAUCHY, 1, 0, C);
    compare(c, FMPNP_MODE_FORWARD, FMPNP_GEMAN_MCCLURE, 0, 3, 11);  // a range that starts off a multiple of 8
    compare(c, FMPNP_MODE_COMPUTE_COST, FMPNP_SQUARED, 0, 0, C);
    errors(c);
    if (fails) {
        printf("test_refine_f16_cpu: %d check(s) FAILED\n", fails);
        return 1;
    }
    printf("test_refine_f16_cpu: OK (65536 widenings, 4 twin runs, argument errors)\n");
    return 0;
}
