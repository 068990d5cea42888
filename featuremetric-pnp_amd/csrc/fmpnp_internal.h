// fmpnp_internal.h -- launch-side definitions shared by the fmpnp HIP sources.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <mutex>

#include "fmpnp.h"

// Speculative next-texel gathers (fmpnp_lm_impl.h spec_pass; variants VAR_*_SPEC), on the waves
// without an LM-tail role (waves >= spec_w0 = 3: the later wave of each SIMD, which finishes its
// point phase after its SIMD partner, and wave 3, idle in the tail) and at most spec_cap = 2 per
// wave per evaluation, which fit in wave 0's LM tail (round 3, B=128: spec_w0 3 / 4 / 5 / 6
// 0.331 / 0.333 / 0.337 / 0.342 ms; cap 2 0.332 ms, cap 1 / 3 / 4 0.341 / 0.344 / 0.340; every
// wave speculating, the tail waves' blocks adopted by waves 3, 5, 6: 0.385 -- DESIGN.md §4.1.1).
// Build with -DFMPNP_SPEC=0 to compile them out.
#ifndef FMPNP_SPEC
#define FMPNP_SPEC 1
#endif

namespace fmpnp {

constexpr int NT = 512;         // threads per workgroup of the LM kernel (8 waves)
constexpr int CH = 64;          // points per reduction chunk = one wave block (fixed: results do not depend on G)
constexpr int NV = 32;          // reduced vector: 21 H + 6 g + rho + kept + supported + 2 pad
constexpr int NSTAMP = 13;      // debug phase-stamp slots: 8 phases + eval-0 proj/gather/loss/contrib + wave 0 speculation
constexpr int RECW = 8;         // per-point record: 6 channel sums + rho + rho'
constexpr int MAX_G = 64;       // workgroups per problem
// LM kernel builds: WPS_LATENCY = one 512-thread workgroup (8 waves) per problem and per CU;
// WPS_THROUGHPUT = 256-thread workgroups (4 waves, two 64-point blocks per wave at N=512),
// two resident per CU, so one problem's serial LM tail overlaps the other's point work
// (batches of >= 2 problems per CU).  Both keep 2 waves per SIMD: up to 256 VGPRs.
constexpr int WPS_LATENCY = FMPNP_BUILD_LATENCY, WPS_THROUGHPUT = FMPNP_BUILD_THROUGHPUT;
constexpr int NT_THROUGHPUT = 256;
// WPS_WIDE = 256-thread workgroups, one wave per SIMD: up to 512 registers per lane (VGPRs +
// AGPRs), for the bilinear cell memo (its LDS allows one workgroup per CU anyway)
constexpr int WPS_WIDE = FMPNP_BUILD_WIDE;

// Kernel arguments (by value).
struct LaunchArgs {
    const fmpnp_problem *probs;   // device descriptors
    int n;
    fmpnp_options opt;
    fmpnp_result *results;        // device
    fmpnp_trace_entry *trace;     // device or null
    int trace_stride;
    int G, teams, nc_max, gw;     // gw: teams per XCD-mapping group (8, or fewer teams)
    unsigned *counters;           // [teams_pad][16], zeroed every launch
    double *partials;             // [teams][2][nc_max][NV]
    double *maxslots;             // [teams][2][G]
    int mmax;                     // max points per workgroup (multiple of CH): dynamic LDS carve
    unsigned long long *stamps;   // debug: [grid][8 waves][NSTAMP] phase cycle totals, or null
    int wps;                      // occupancy variant (WPS_LATENCY / WPS_THROUGHPUT)
    int spec;                     // speculative next-texel gathers (memoised nearest modes)
    int spec_cap;                 // at most this many speculative gathers per wave per evaluation
    int spec_w0;                  // waves >= spec_w0 speculate (the later wave of each SIMD: 4)
    int dbg;                      // debug knob (FMPNP_DBG): bit 2 per-evaluation stamps, bit 3 helpers
                                  // never publish (exercises the main workgroups' bounded wait)
    // first-evaluation helpers (small batches, one workgroup per problem): workgroups
    // grid_main .. grid_main + n * helpers - 1 gather the initial pose's records of their
    // problem's blocks into hrec and publish each block with a tagged flag (lm_kernel)
    int helpers, grid_main;
    unsigned long long htag;      // this launch's flag value (a process-wide sequence + a magic)
    double *hrec;                 // [n][nc_max * CH][HREC] (six sums, then the texel offset)
    unsigned long long *hflag;    // [n][nc_max]
};
constexpr int HREC = 7;

// Fixed LDS head: the LM state + per-problem context (sized generously, 16-B aligned).
// Debug instrumentation (phase stamps, per-evaluation stamps, the evaluation timeline) exists only
// in a diagnostics build (-DFMPNP_STAMPS=1 on every unit, tools/build_ab.sh); its LDS arrays then
// enlarge the head below, so every unit must see the same value.
#ifndef FMPNP_STAMPS
#define FMPNP_STAMPS 0
#endif
// LDS head of the LM kernel (LMState, fmpnp_lm_impl.h): 2 KB in the product build
__host__ __device__ constexpr int lds_fixed_bytes() { return FMPNP_STAMPS ? 4608 : 2304; }
// row stride (doubles) of the LM kernel's structure-of-arrays LDS records: odd, so the
// writers of one point's fields fall in distinct banks (fmpnp_lm_impl.h lds_X / lds_rec)
__host__ __device__ constexpr int lds_rs(int mmax) { return mmax + 1; }
// speculative next-texel records (fmpnp_lm_impl.h lds_rec2 ...): rec2[6][rs] doubles, and
// 32-bit words for tex, tex2, spec, slot, qp[2] per point (16-B padded); without speculation
// only tex
__host__ __device__ constexpr int lds_spec_doubles(int mmax, bool spec) { return spec ? 6 * lds_rs(mmax) : 0; }
__host__ __device__ constexpr int lds_words(int mmax, bool spec) { return ((spec ? 6 : 1) * mmax + 3) / 4 * 4; }
// bilinear cell memo (fmpnp_lm_impl.h eval_pass_bil): per point the Bernstein coefficients of
// the six channel sums as functions of the position inside the point's 2x2 cell, memo[BIL_NB][rs]
// doubles after the partials.  It bounds a workgroup to BIL_MAX_M points (four 64-point blocks).
constexpr int BIL_NB = 54;
constexpr int BIL_MAX_M = 256;
size_t lm_dyn_lds_bytes(int mmax, int nc_max, bool spec, bool bil_memo = false);

// var: the plan's variant (spec_variant / help_variant already applied)
hipError_t launch_lm(const LaunchArgs &a, int dtype, int var, int grid, size_t lds, hipStream_t stream);
// LM kernel variants (fmpnp_lm_impl.h lm_kernel<T, WPS, TEAM, RATIO, VAR>); the values are the public
// FMPNP_VAR_* codes of fmpnp_launch_info.  A variant is a kind and five independent flags, stated once in
// VAR_TABLE below: the planner's mappers, the kernel's compile-time constants and the set of kernels that is
// built (lm_built, lm_pick) all read that table.
constexpr int VAR_NEAREST = FMPNP_VAR_NEAREST, VAR_GM = FMPNP_VAR_GM, VAR_BILINEAR = FMPNP_VAR_BILINEAR,
              VAR_F_NEAREST = FMPNP_VAR_F_NEAREST, VAR_F_GM = FMPNP_VAR_F_GM, VAR_BIL_DIRECT = FMPNP_VAR_BIL_DIRECT,
              VAR_GM_SPEC = FMPNP_VAR_GM_SPEC, VAR_NEAREST_SPEC = FMPNP_VAR_NEAREST_SPEC,
              VAR_GM_SPEC_H = FMPNP_VAR_GM_SPEC_H, VAR_NEAREST_SPEC_H = FMPNP_VAR_NEAREST_SPEC_H,
              VAR_GM_H = FMPNP_VAR_GM_H, VAR_NEAREST_H = FMPNP_VAR_NEAREST_H,
              VAR_GM_SPEC_512 = FMPNP_VAR_GM_SPEC_512, VAR_GM_SPEC_H_512 = FMPNP_VAR_GM_SPEC_H_512,
              VAR_GM_W = FMPNP_VAR_GM_W, VAR_NEAREST_W = FMPNP_VAR_NEAREST_W, VAR_GM_H_W = FMPNP_VAR_GM_H_W,
              VAR_NEAREST_H_W = FMPNP_VAR_NEAREST_H_W;
constexpr int N_VAR = FMPNP_VAR_NEAREST_H_W + 1, MMAX_512 = 512;
// kind: nearest sampling of the packed f, gx, gy planes (the hot path); nearest sampling of FMPNP_LAYOUT_F maps
// (fp32 only); bilinear sampling with the cell memo; bilinear sampling without it (no_memo = 1: every supported
// point sampled at every evaluation)
enum VarKind { KIND_PACKED, KIND_F, KIND_BIL_MEMO, KIND_BIL_DIRECT };
enum : unsigned { FLAG_SPEC = 1, FLAG_HELP = 2, FLAG_M512 = 4, FLAG_WIN = 8 };
struct VarTraits {
    VarKind kind;
    bool gm;    // the loss constant-folded to Geman-McClure (forward); otherwise any loss / mode
    bool spec;  // the speculative next-texel gathers compiled in (the planner's P.spec); the other variants are
                // built without them, so their code does not pay for speculation they do not run
    bool help;  // the first-evaluation helpers' hand-off compiled in (small batches: LaunchArgs::helpers; the
                // headline-size batches run without it and without its code)
    bool win;   // the packed-window check compiled in (a window on the f, gx, gy planes: fmpnp_feature_pnp's
                // windowed packs); without a window the check's code alone cost the non-speculating variants up
                // to 6 %, so the other variants do not carry it
    bool m512;  // compiled for one 512-point workgroup (mmax = 512 at compile time: the LDS carve's offsets are
                // immediates, ~25 fewer scalar registers spilled)
    // the flags as bits, in the order the planner applies them (make_plan: spec, help, m512, win)
    constexpr unsigned mask() const { return spec * FLAG_SPEC | help * FLAG_HELP | m512 * FLAG_M512 | win * FLAG_WIN; }
};
constexpr VarTraits VAR_TABLE[N_VAR] = {
    //  kind             gm     spec   help   win    m512
    {KIND_PACKED,     false, false, false, false, false},  //  0 NEAREST
    {KIND_PACKED,     true,  false, false, false, false},  //  1 GM
    {KIND_BIL_MEMO,   false, false, false, false, false},  //  2 BILINEAR
    {KIND_F,          false, false, false, false, false},  //  3 F_NEAREST
    {KIND_F,          true,  false, false, false, false},  //  4 F_GM
    {KIND_BIL_DIRECT, false, false, false, false, false},  //  5 BIL_DIRECT
    {KIND_PACKED,     true,  true,  false, false, false},  //  6 GM_SPEC
    {KIND_PACKED,     false, true,  false, false, false},  //  7 NEAREST_SPEC
    {KIND_PACKED,     true,  true,  true,  false, false},  //  8 GM_SPEC_H
    {KIND_PACKED,     false, true,  true,  false, false},  //  9 NEAREST_SPEC_H
    {KIND_PACKED,     true,  false, true,  false, false},  // 10 GM_H
    {KIND_PACKED,     false, false, true,  false, false},  // 11 NEAREST_H
    {KIND_PACKED,     true,  true,  false, false, true},   // 12 GM_SPEC_512
    {KIND_PACKED,     true,  true,  true,  false, true},   // 13 GM_SPEC_H_512
    {KIND_PACKED,     true,  false, false, true,  false},  // 14 GM_W
    {KIND_PACKED,     false, false, false, true,  false},  // 15 NEAREST_W
    {KIND_PACKED,     true,  false, true,  true,  false},  // 16 GM_H_W
    {KIND_PACKED,     false, false, true,  true,  false},  // 17 NEAREST_H_W
};
constexpr VarTraits var_traits(int var) { return VAR_TABLE[var]; }
// var with one more flag: the variant whose row is var's with `flag` set, or var where there is none.  (A
// variant that has the flag, or one the planner applies later, is left alone, as the planner never asks.)
constexpr int with_flag(int var, unsigned flag) {
    if (var < 0 || var >= N_VAR || VAR_TABLE[var].mask() >= flag) return var;
    for (int v = 0; v < N_VAR; ++v)
        if (VAR_TABLE[v].kind == VAR_TABLE[var].kind && VAR_TABLE[v].gm == VAR_TABLE[var].gm &&
            VAR_TABLE[v].mask() == (VAR_TABLE[var].mask() | flag))
            return v;
    return var;
}
constexpr int spec_variant(int var) { return with_flag(var, FLAG_SPEC); }
constexpr int help_variant(int var) { return with_flag(var, FLAG_HELP); }
constexpr int m512_variant(int var) { return with_flag(var, FLAG_M512); }
constexpr int win_variant(int var) { return with_flag(var, FLAG_WIN); }
// (the planner's choices must not move with an edit of the table: the four mappers' values for the codes 0 .. 17)
constexpr bool maps_to(int (*f)(int), const int (&want)[N_VAR]) {
    for (int v = 0; v < N_VAR; ++v)
        if (f(v) != want[v]) return false;
    return true;
}
static_assert(maps_to(spec_variant, {7, 6, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17}), "spec_variant");
static_assert(maps_to(help_variant, {11, 10, 2, 3, 4, 5, 8, 9, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17}), "help_variant");
static_assert(maps_to(m512_variant, {0, 1, 2, 3, 4, 5, 12, 7, 13, 9, 10, 11, 12, 13, 14, 15, 16, 17}), "m512_variant");
static_assert(maps_to(win_variant, {15, 14, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17, 12, 13, 14, 15, 16, 17}), "win_variant");
// Whether lm_kernel<texels of dtype, wps, team, *, var> is built (with and without the ratio test alike):
//  * the wide build holds the bilinear cell memo only, and nothing else holds it (fp32 and fp64);
//  * the throughput build (one workgroup per problem, never a team) holds the plain packed variants and the
//    direct bilinear one;
//  * the latency build holds the rest; speculation, the helpers and the 512-point carve without a team only
//    (one workgroup per problem), so the window variants without helpers are the only flagged ones with a team;
//  * FMPNP_LAYOUT_F and the 512-point carve: fp32 texels only; binary16 texels: the packed kinds only.
constexpr bool lm_built(int dtype, int wps, bool team, int var) {
    if (var < 0 || var >= N_VAR) return false;
    const VarTraits v = VAR_TABLE[var];
    if ((v.kind == KIND_F || v.m512) && dtype != FMPNP_F32) return false;
    if (v.kind != KIND_PACKED && dtype == FMPNP_F16) return false;
    if (wps == WPS_WIDE || v.kind == KIND_BIL_MEMO) return wps == WPS_WIDE && v.kind == KIND_BIL_MEMO;
    const bool flagged = v.spec || v.help || v.win || v.m512;
    if (wps == WPS_THROUGHPUT) return !team && !flagged && v.kind != KIND_F;
    return wps == WPS_LATENCY && !(team && (v.spec || v.help || v.m512));
}
// Scratch of the synchronous entry points, one per (entry point, device, stream): SURVEY.md 8b asks for calls
// that are thread-safe across distinct streams and devices, so calls on different streams (or devices) use
// different buffers and run concurrently, and calls on one stream serialise on the entry's mutex.  Growing
// frees only the entry's own buffer, stream-ordered on its own stream (no device-wide synchronisation, never
// another device's memory).  An entry is used through a SyncCall (below), which holds the mutex until the
// call's stream has drained, so no copy or kernel of an earlier call still reads the buffers.
struct StreamScratch {
    std::mutex mu;
    unsigned char *dev = nullptr;   // device memory of the entry's device
    size_t dev_bytes = 0;
    unsigned char *host = nullptr;  // pinned staging
    size_t host_bytes = 0;
    // fmpnp_feature_pnp's second stream on the entry's device (the channels the first level does not read
    // are packed there, under the first level's LM launch) and its two fences; created on first use
    hipStream_t side = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
};
enum { SCRATCH_REFINE = 0, SCRATCH_QUERY = 1, SCRATCH_MATCH = 2, SCRATCH_PNP = 3, SCRATCH_NETVLAD = 4, SCRATCH_RANK = 5,
       SCRATCH_LOCALIZE = 6, SCRATCH_SUPERPOINT = 7, SCRATCH_SP_COUNTS = 8, SCRATCH_IMAGE = 9 };
// the carves' unit: every piece of a scratch buffer starts on a 256-byte boundary
inline size_t align256(size_t x) { return (x + 255) / 256 * 256; }
// One synchronous call on the scratch of (pool, current device, stream): the constructor finds the entry, locks
// it for the call's lifetime and grows it to dev_bytes of device memory (at least dev_min when it allocates) and
// host_bytes of pinned memory; error() is then 0, FMPNP_ENODEV or FMPNP_ENOMEM.  finish() waits for the stream
// and returns its error: the success path's return value.  (Not for the entry's side stream: a call that used it
// has fenced its work into the stream before the last launch, and a second wait per call cost fmpnp_feature_pnp
// 3 us, profiles/sync_guard_ab.json.)  A return without finish() waits in the destructor, for the stream and
// for the side stream when one was created, so every return after construction drains both before the next
// call on the stream can reuse the buffers.
class SyncCall {
public:
    SyncCall(int pool, hipStream_t s, size_t dev_bytes, size_t host_bytes, size_t dev_min = (size_t)1 << 20);
    ~SyncCall();
    SyncCall(const SyncCall &) = delete;
    SyncCall &operator=(const SyncCall &) = delete;
    int error() const { return err_; }
    int finish();
    // more work follows a finish() within the same call (fmpnp_feature_pnp's re-run after a window miss, the
    // SuperPoint calls that read a count before they queue the rows' copy)
    void resume() { queued_ = true; }
    // an asynchronous entry point's use of the entry (the image front end): everything the call queues, the growth
    // included, is ordered on the stream, and the entry's next use is ordered on the same stream behind it, so
    // nothing is waited for; the mutex is still held until the call returns
    void detach() { queued_ = false; }
    StreamScratch *sc = nullptr;
    unsigned char *dev = nullptr, *host = nullptr;  // the entry's buffers (sc->dev_bytes, sc->host_bytes)

private:
    std::unique_lock<std::mutex> lock_;
    hipStream_t s_;
    int err_ = 0;
    bool queued_ = false;
};
// the entry's side stream and events (within a SyncCall, on the entry's device); 0 or a hipError_t
int scratch_side(StreamScratch &c);
// dense exhaustive matching's argument checks, fp32 precision (fmpnp_match.hip)
int dense_match_args(const void *sparse, int N, int ld_sparse, const void *dense, int C, int WH, int ld_dense, int top_k,
                     double ratio, const void *argmax, const void *top, const void *kth, const void *mask);
int lm_variant(const fmpnp_options &o);
const void *lm_kernel_ptr(int dtype, int wps, bool team, bool ratio, int var);

hipError_t launch_pack(const void *chw, const void *gx, const void *gy, int dtype_in, int C, int H, int W, void *out,
                       int dtype_out, int cs, int normalized, int replicate, hipStream_t stream, int planes = 3);
hipError_t launch_gather_ref(const void *ref, int dtype_in, int C, int H, int W, const double *inl, int N, int img0,
                             int img1, void *out, int dtype_out, int ld_out, int *err, hipStream_t stream);
// the window map of n problems ([2][Hf][Wf] bytes at fmpnp_problem.window): cleared, then every point's
// square of `radius` texels around its texel at (R0, t0) marked in plane 0 (radius - 1 in plane 1)
hipError_t launch_win_mark(const fmpnp_problem *probs_dev, int n, int radius, int max_n, long max_hw, hipStream_t stream);
// fused Sobel + channels-last pack of the texels marked in win ([H][W] bytes, plane 0) only
hipError_t launch_pack_win(const void *chw, int dtype_in, int C, int H, int W, void *out, int dtype_out, int cs,
                           int normalized, int replicate, const unsigned char *win, hipStream_t stream);
// n f-only packs (FMPNP_LAYOUT_F, fp32 out) in ceil(n / 32) launches; shape[4i..] = C, H, W, cstride
hipError_t launch_pack_f_batch(int n, const void *const *chw, void *const *out, const int *shape, int dtype_in,
                               hipStream_t stream);
// windowed f-only packs of n problems (fmpnp_pack_features_f_window_batch): clear the window maps,
// mark each point's initial texel neighbourhood, pack the marked texels
hipError_t launch_pack_f_window(const fmpnp_problem *probs_dev, const fmpnp_problem *probs_host, int n,
                                const void *const *chw, int dtype_in, int radius, int max_n, long max_hw,
                                hipStream_t stream);
// n gathers in ceil(n / 32) launches (item table in the kernel arguments); err: [n] device flags
hipError_t launch_gather_ref_batch(int n, const void *const *ref, const int *ref_shape, const double *const *inl,
                                   const int *n_inl, int img0, int img1, void *const *out, const int *ld_out,
                                   int dtype_in, int dtype_out, int *err, hipStream_t stream);

// per-point 0.5 ||f(p_i) - fref_i||^2 and support at the descriptor's pose (fmpnp_point_costs)
hipError_t launch_point_costs(const fmpnp_problem &p, int layout, int dtype, double *cost, int *supported,
                              hipStream_t stream);
// compute_cost (model.py:216-243) at the descriptor's pose: point costs into cost / supported (device,
// [N] each), then one fixed-order reduction into *out (device): initial_cost, NO_SUPPORT status
hipError_t launch_compute_cost(const fmpnp_problem &p, int layout, int dtype, int use_ratio, double thr,
                               double *cost, int *supported, fmpnp_result *out, hipStream_t stream);
hipError_t launch_cost_mean(const fmpnp_problem &p, int use_ratio, double thr, const double *cost,
                            const int *supported, fmpnp_result *out, hipStream_t stream);
// compute_cost of n problems whose descriptors (N included) are in DEVICE memory: the same two kernels' bodies
// over a grid sized from max_cap (the largest capacity), problem i's costs at cost + offset_i where offset_i is
// the long long at offsets_dev + i * offsets_stride bytes, its result at out[i * out_stride]
hipError_t launch_compute_cost_batch(const fmpnp_problem *probs_dev, int n, int max_cap, const long long *offsets_dev,
                                     long long offsets_stride, int layout, int dtype, int use_ratio, double thr,
                                     double *cost, int *supported, fmpnp_result *out, int out_stride,
                                     hipStream_t stream);
// the body of fmpnp_localize_ex; refine: NULL, or the batched refinement stage queued behind the pick
// (fmpnp_localize_refined, fmpnp_localize_refine.hip)
struct LocalizeRefine {
    const fmpnp_loc_refine_source *sources;  // HOST [n_pairs]
    const int *query_hw;                     // HOST [n_queries][2]
    const fmpnp_loc_refine_params *params;
    const fmpnp_options *opt;
    fmpnp_result *results;                   // HOST [n_queries][n_res]
    int *flags;                              // HOST [n_queries]
};
// fmpnp_localize_refine_workspace_size with the reason it is 0: 0, FMPNP_EINVAL, FMPNP_ETOOBIG or a hipError_t
int localize_refine_workspace(const fmpnp_loc_query *queries_host, int n_queries, const fmpnp_loc_refine_map *maps_host,
                              const fmpnp_loc_refine_params *params, const fmpnp_options *opt, size_t *bytes);

// dense exhaustive matching (fmpnp_match.hip): the fp32 MFMA correlation of N rows into scores
// ([N][ld_scores]), the per-row argmax / d1 / d_k / ratio mask, and the nearest-cell descriptor gather
hipError_t launch_corr(const float *sparse, int N, int ld_sparse, const float *dense, int C, int WH, int ld_dense,
                       float *scores, size_t ld_scores, hipStream_t s);
hipError_t launch_select(const float *scores, size_t ld_scores, int N, int WH, int top_k, float ratio2, int *argmax,
                         float *top, float *kth, unsigned char *mask, hipStream_t s);
hipError_t launch_gather_sparse(const float *chw, int C, int D1, int D2, const double *pts, int N, double cell0,
                                double cell1, float *out, int ld_out, hipStream_t s);

// hypercolumn assembly (fmpnp_hypercolumn.hip): validated arguments (fmpnp_hypercolumn_impl.h check_args; C
// the channel total) -> one kernel on the stream; 0, FMPNP_ETOOBIG or a hipError_t
int launch_hypercolumn(const fmpnp_hc_layer *layers, int L, int B, float *out, int H, int W, long long osb,
                       long long osc, long long osy, long long C, int flags, hipStream_t stream);

// sparse hypercolumns (fmpnp_hypercolumn_sparse.hip): validated arguments (fmpnp_hypercolumn_impl.h
// check_sparse_args; C the channel total) -> one kernel on the stream (none for N = 0); 0 or a hipError_t
int launch_hypercolumn_sparse(const fmpnp_hc_layer *layers, int L, int B, int H, int W, const void *points,
                              const int *item, int N, int at, double p0, double p1, void *out, int dtype_out,
                              long long ld_out, long long C, int flags, int *err_flag, hipStream_t stream);

// fused hypercolumn pack (fmpnp_hypercolumn_pack.hip), validated arguments (fmpnp_hypercolumn_pack_impl.h
// check_pack_args; C the channel total); 0, FMPNP_ETOOBIG or a hipError_t.  launch_hc_norm: every texel's norm
// over all C channels into norm ([H][W] fp32, hc_pack_workspace_bytes; with marks only where a mark lies within
// one texel).  launch_hc_pack: channels [c_begin, c_end) of the marked texels (marks NULL: all) into the packed
// map; norm NULL: no normalisation
size_t hc_pack_workspace_bytes(int H, int W);
int launch_hc_norm(const fmpnp_hc_layer *layers, int L, int item, int H, int W, long long C, float *norm,
                   const unsigned char *marks, hipStream_t stream);
int launch_hc_pack(const fmpnp_hc_layer *layers, int L, int item, int H, int W, long long C, int c_begin, int c_end,
                   int layout, int dtype_out, int cs, int sobel_normalized, int replicate, const unsigned char *marks,
                   const float *norm, void *out, hipStream_t stream);

// retrieval (fmpnp_retrieval.hip), validated arguments (fmpnp_retrieval_impl.h pool_args / rank_args): the
// NetVLAD pooling's four kernels per round of images (0, FMPNP_ETOOBIG or a hipError_t) over a workspace of
// netvlad_workspace_bytes, and the top-n selection over Q rows of a score map
size_t netvlad_workspace_bytes(int B, int K, int C, int P);
int launch_netvlad_pool(const float *x, int B, int C, int P, long long sb, long long sc, const float *w, int K, int ld_w,
                        const float *cent, int ld_c, int normalize, float *out, long long ld_out, void *workspace,
                        hipStream_t s);
hipError_t launch_rank(const float *scores, size_t ld_scores, int Q, int R, int n, int *idx, float *top, hipStream_t s);

}  // namespace fmpnp
