// fmpnp_host.h -- the plumbing the CPU twins share: dealing work over host threads, and the fp32 fmaf chains
// of the correlation-like products.  Plain C++17, no HIP headers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <functional>
#include <thread>
#include <vector>

namespace fmpnp {
namespace host {

// Items [0, n) over host threads, `chunk` consecutive items at a time from one atomic counter.  n_threads == 0:
// hardware_concurrency(); the count is clamped to [1, chunks].  Every thread (the caller is one of them) builds
// its own state with make_worker() -- so per-thread buffers are allocated inside the guard -- and calls the
// returned body(i) for each item it draws.  A thread that cannot be spawned is skipped: the items are dealt by
// the counter, so fewer threads do the same work.  Any exception stops that thread and sets the failure flag;
// every thread is joined.  false: a thread or an allocation failed (the twins' FMPNP_ENOMEM), and some items
// may not have been visited.  Nothing throws.
template <class F>
bool deal(long long n, int n_threads, F &&make_worker, long long chunk = 1) {
    const long long chunks = (n + chunk - 1) / chunk;
    int nt = n_threads > 0 ? n_threads : (int)std::thread::hardware_concurrency();
    nt = (int)std::max<long long>(1, std::min<long long>(nt, chunks));
    std::atomic<long long> next(0);
    std::atomic<bool> failed(false);
    auto guarded = [&]() {
        try {
            auto body = make_worker();
            for (long long c = next.fetch_add(1); c < chunks; c = next.fetch_add(1))
                for (long long i = c * chunk, end = std::min(n, i + chunk); i < end; ++i) body(i);
        } catch (...) {
            failed = true;
        }
    };
    std::vector<std::thread> threads;
    try {
        threads.reserve((size_t)nt - 1);
        for (int t = 1; t < nt; ++t) threads.emplace_back(guarded);
    } catch (...) {  // (a thread that cannot start: the ones that did, and the caller, do the work)
    }
    guarded();
    for (auto &t : threads) t.join();
    return !failed;
}

// An IEEE binary16 bit pattern widened to fp32 (exact: every binary16 value is an fp32 value; (double) of the
// result is exact too).  Bit-level, because the twins are built by the host compiler without a half type
// (-mf16c is not assumed).  Subnormals are normalised, Inf stays Inf, a NaN keeps its sign and its payload in
// the top mantissa bits (a signalling pattern is not quieted, as the compiler's own software widening leaves
// it; the arithmetic that follows only asks whether a value is NaN).
inline float half_bits_to_float(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
    uint32_t exp = (h >> 10) & 0x1fu, man = h & 0x3ffu, bits;
    if (exp == 0x1fu) {
        bits = sign | 0x7f800000u | (man << 13);
    } else if (exp == 0) {
        if (man == 0) {
            bits = sign;
        } else {  // subnormal: value = man * 2^-24; shift the leading one up to bit 10
            int e = -1;
            do {
                man <<= 1;
                ++e;
            } while (!(man & 0x400u));
            bits = sign | (uint32_t)(127 - 15 - e) << 23 | ((man & 0x3ffu) << 13);
        }
    } else {
        bits = sign | (exp + (127 - 15)) << 23 | (man << 13);
    }
    float f;
    static_assert(sizeof(f) == sizeof(bits), "fp32 is 32 bits");
    __builtin_memcpy(&f, &bits, sizeof(f));
    return f;
}
// a binary16 texel in host memory (FMPNP_F16 storage): converts like any other storage type
struct Half {
    uint16_t bits;
    explicit operator double() const { return (double)half_bits_to_float(bits); }
};
static_assert(sizeof(Half) == 2, "binary16 storage is two bytes");

// fl16(x) as an fp32 value: IEEE binary16, round-to-nearest-even; NaN and +-Inf kept, |x| >= 65520 -> +-Inf,
// fp16 subnormals (multiples of 2^-24 below 2^-14) kept.  The operand rounding of the fp16 precisions (the match
// stage's and the encoder's, include/fmpnp.h).
inline float fl16(float x) {
    unsigned u;
    __builtin_memcpy(&u, &x, 4);
    const unsigned sign = u & 0x80000000u;
    unsigned a = u & 0x7fffffffu;
    if (a > 0x7f800000u) return x;                      // NaN
    if (a >= 0x477ff000u) a = 0x7f800000u;              // 65520 and above (Inf included): Inf
    else if (a >= 0x38800000u) {                        // normal in fp16: 13 significand bits go, ties to even
        a += 0xfffu + ((a >> 13) & 1u);
        a &= ~0x1fffu;
    } else {                                            // below 2^-14: the nearest multiple of 2^-24, ties to even
        float m;
        __builtin_memcpy(&m, &a, 4);
        volatile float t = m + 0.5f;                    // (fp32's ulp in [0.5, 1) is 2^-24; the unit is built
        t = t - 0.5f;                                   //  without fast-math, and the sum rounds to nearest-even)
        m = t;
        __builtin_memcpy(&a, &m, 4);
    }
    a |= sign;
    float r;
    __builtin_memcpy(&r, &a, 4);
    return r;
}
// the binary16 bit pattern of fl16(x) (what v_cvt_f16_f32 stores for a value that is not a NaN; a NaN becomes a
// quiet one of the same sign)
inline uint16_t float_to_half_bits(float x) {
    const float r = fl16(x);
    uint32_t u;
    __builtin_memcpy(&u, &r, 4);
    const uint16_t sign = (uint16_t)((u >> 16) & 0x8000u);
    const uint32_t a = u & 0x7fffffffu;
    if (a > 0x7f800000u) return (uint16_t)(sign | 0x7e00u | ((a >> 13) & 0x3ffu));
    if (a == 0x7f800000u) return (uint16_t)(sign | 0x7c00u);
    if (a >= 0x38800000u) return (uint16_t)(sign | ((a - 0x38000000u) >> 13));  // (the low 13 bits are zero)
    float m;
    __builtin_memcpy(&m, &a, 4);
    return (uint16_t)(sign | (uint32_t)(m * 16777216.0f));  // a multiple of 2^-24 below 2^-14: its count
}

// acc[j] = fmaf(s[i], m[i * ld + j], acc[j]) for i = 0 .. ni-1 ascending from acc[j] = +0: every j < nj is its own
// chain (what v_mfma_f32_32x32x2_f32 computes per output).  The loop order is the contract: nothing here blocks
// or reorders; callers block their columns themselves.  The twins are built without contraction and without
// -mfma, so the first version's fmaf is libm's (correctly rounded in software where the core has no FMA); the
// second is the same loop compiled for cores with FMA: one vfmadd per product, the same value.
__attribute__((always_inline)) inline void fmaf_chains_body(const float *s, const float *m, size_t ld, int ni, int nj,
                                                            float *acc) {
    for (int j = 0; j < nj; ++j) acc[j] = 0.f;
    for (int i = 0; i < ni; ++i) {
        const float si = s[i];
        const float *row = m + (size_t)i * ld;
        for (int j = 0; j < nj; ++j) acc[j] = __builtin_fmaf(si, row[j], acc[j]);
    }
}
inline void fmaf_chains_libm(const float *s, const float *m, size_t ld, int ni, int nj, float *acc) {
    fmaf_chains_body(s, m, ld, ni, nj, acc);
}
typedef void (*fmaf_chains_fn)(const float *, const float *, size_t, int, int, float *);
#if defined(__x86_64__)
__attribute__((target("avx2,fma"))) inline void fmaf_chains_fma(const float *s, const float *m, size_t ld, int ni, int nj,
                                                                float *acc) {
    fmaf_chains_body(s, m, ld, ni, nj, acc);
}
inline bool have_fma() { return __builtin_cpu_supports("fma") && __builtin_cpu_supports("avx2"); }
inline fmaf_chains_fn pick_fmaf_chains() { return have_fma() ? fmaf_chains_fma : fmaf_chains_libm; }
#else
inline bool have_fma() { return false; }
inline fmaf_chains_fn pick_fmaf_chains() { return fmaf_chains_libm; }
#endif
// the version for this core, resolved once
inline void fmaf_chains(const float *s, const float *m, size_t ld, int ni, int nj, float *acc) {
    static const fmaf_chains_fn fn = pick_fmaf_chains();
    fn(s, m, ld, ni, nj, acc);
}

// ---- the match stage's row reduction (select_kernel of fmpnp_match.hip, restated for a CPU core) ----
// the order-preserving key: every NaN is the greatest key, -0 counts as +0
inline unsigned score_key(float x) {
    if (x != x) return 0xffffffffu;
    const float y = x + 0.f;
    unsigned u;
    __builtin_memcpy(&u, &y, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
inline float key_score(unsigned key) {
    unsigned u = key == 0xffffffffu ? 0x7fc00000u : (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key;
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}
// one row's argmax (the lowest index among equal maxima), d1, the exact top_k-th largest value and the mask
// (one fp32 product; the twins are built without contraction).  keys: [WH] scratch
inline void select_row(const float *row, int WH, int top_k, float ratio2, unsigned *keys, int *argmax, float *top,
                       float *kth, unsigned char *mask) {
    unsigned best = 0;
    int best_j = 0;
    for (int j = 0; j < WH; ++j) {
        const unsigned key = keys[j] = score_key(row[j]);
        if (j == 0 || key > best) {
            best = key;
            best_j = j;
        }
    }
    std::nth_element(keys, keys + (top_k - 1), keys + WH, std::greater<unsigned>());
    const float d1 = key_score(best), dk = key_score(keys[top_k - 1]);
    *argmax = best_j;
    *top = d1;
    *kth = dk;
    const volatile float prod = ratio2 * d1;
    *mask = prod >= dk ? 1 : 0;
}

}  // namespace host
}  // namespace fmpnp
