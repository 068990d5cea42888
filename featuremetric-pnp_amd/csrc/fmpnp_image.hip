// fmpnp_image.hip -- the image front end (include/fmpnp.h, "image front end"): Pillow's 8-bit Lanczos resampling and
// the value transforms of the reference's three loaders (s2dhm/network/images_from_list.py:57-103,
// s2dhm/d2net_utils/extract_dense_features.py:27-45, s2dhm/superpoint/detect_and_compute_superpoint.py:6-10), from
// decoded uint8 [B][H][W][3] pixels to the bytes or the planar float32 tensor the networks take.
//
//   hpass_kernel   the horizontal pass: uint8 rows of W pixels -> uint8 rows of w pixels.  A workgroup owns 64 output
//                  columns of H_ROWS rows; the 64 columns' coefficient rows and bounds go to LDS once (row stride ksize,
//                  which is odd: the lanes' reads fall in distinct banks), or stay in global memory where they would
//                  not fit (ksize above 190: a shrink beyond 31x).  One thread forms one output pixel: three int32 accumulators.
//   vpass_kernel   the vertical pass and every epilogue.  A workgroup owns 256 pixels of four output rows, one row
//                  per wave; a thread owns four pixels, that is 12 consecutive bytes of every source row: three dword
//                  loads where the source is 4-byte aligned, byte loads otherwise and in a row's ragged tail.  A row's
//                  coefficients are uniform over its wave (scalar loads).  RESIZE = false takes the bytes as they are: the transform alone,
//                  or the pass-through copy.  The epilogue stores the 12 bytes (MODE_U8), or looks each byte up in a
//                  3 x 256 float table that the workgroup fills in LDS with img::value_of -- true fp32 divisions, as the
//                  twin's -- and stores one float4 per plane (MODE_F32: three planes; MODE_GRAY: one, of the integer
//                  gray value).
//
// The intermediate between the passes is uint8, as Pillow's: its rounding is part of the result.  It lives in the
// stream's scratch with its rows padded to 4 bytes.  The tables come from img::build_table on the host, the twin's own,
// and are cached per (device, stream): TABLE_SLOTS axis tables in the scratch's device buffer, each with a pinned
// staging slot and an event that says when the slot's last upload has been read.  Everything a call queues -- the
// scratch's growth, a table's upload, the launches -- is ordered on the caller's stream.
//
// Built with -ffp-contract=off.  Plain loads and stores, no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <map>
#include <memory>
#include <vector>

#include "fmpnp.h"
#include "fmpnp_image_impl.h"
#include "fmpnp_internal.h"

namespace fmpnp {
namespace {

using namespace img;

constexpr int NT_IMG = 256;
constexpr int H_COLS = 64, H_ROWS = 16;             // the horizontal pass's tile: 64 columns x 16 rows, 4 rows per thread
constexpr int V_PIX = 4, V_COLS = 64 * V_PIX, V_ROWS = NT_IMG / 64;  // the vertical pass's: 256 pixels x 4 rows, a row per wave
constexpr size_t H_LDS_MAX = 48 * 1024;
enum { MODE_U8 = 0, MODE_F32 = 1, MODE_GRAY = 2 };

struct HArgs {
    const uint8_t *src;
    long long src_is, src_rs;  // bytes
    uint8_t *dst;
    long long dst_is, dst_rs;
    const int32_t *table;  // bounds[w][2], k[w][ksize]
    int H, w, ksize;
};

template <bool LDS>
__global__ __launch_bounds__(NT_IMG) void hpass_kernel(const HArgs a) {
    extern __shared__ int32_t h_lds[];  // bounds[64][2], k[64][ksize]
    const int col0 = (int)blockIdx.x * H_COLS;
    const int ncols = min(H_COLS, a.w - col0);
    const int32_t *gb = a.table + 2 * (size_t)col0;
    const int32_t *gk = a.table + 2 * (size_t)a.w + (size_t)col0 * (size_t)a.ksize;
    if (LDS) {
        for (int i = (int)threadIdx.x; i < 2 * ncols; i += NT_IMG) h_lds[i] = gb[i];
        for (int i = (int)threadIdx.x; i < ncols * a.ksize; i += NT_IMG) h_lds[2 * H_COLS + i] = gk[i];
        __syncthreads();
    }
    const int lc = (int)(threadIdx.x & (H_COLS - 1)), lr = (int)(threadIdx.x / H_COLS);
    if (lc >= ncols) return;
    const int32_t *bounds = LDS ? h_lds + 2 * lc : gb + 2 * lc;
    const int32_t *k = LDS ? h_lds + 2 * H_COLS + mul_small(lc, a.ksize) : gk + (size_t)lc * (size_t)a.ksize;
    const int xmin = bounds[0], xmax = bounds[1];
    const int row0 = (int)blockIdx.y * H_ROWS + lr;
    const uint8_t *s = a.src + (long long)blockIdx.z * a.src_is + (long long)row0 * a.src_rs + 3 * (long long)xmin;
    uint8_t *d = a.dst + (long long)blockIdx.z * a.dst_is + (long long)row0 * a.dst_rs + 3 * (long long)(col0 + lc);
    constexpr int STEP = NT_IMG / H_COLS;
    const int nrows = min(H_ROWS, a.H - (int)blockIdx.y * H_ROWS);
    for (int r = lr; r < nrows; r += STEP, s += STEP * a.src_rs, d += STEP * a.dst_rs) {
        int a0 = ROUND, a1 = ROUND, a2 = ROUND;
        for (int x = 0; x < xmax; ++x) {
            const int kx = k[x];
            a0 = tap(a0, s[3 * x], kx);
            a1 = tap(a1, s[3 * x + 1], kx);
            a2 = tap(a2, s[3 * x + 2], kx);
        }
        d[0] = (uint8_t)finish(a0);
        d[1] = (uint8_t)finish(a1);
        d[2] = (uint8_t)finish(a2);
    }
}

struct VArgs {
    const uint8_t *src;
    long long src_is, src_rs;  // bytes
    void *dst;                 // uint8 [B][h][w][3] or float [B][C][h][w], contiguous
    const int32_t *table;      // bounds[h][2], k[h][ksize] (RESIZE)
    int h, w, ksize;
    int src_aligned;           // src, src_is and src_rs are multiples of 4
    int dst_aligned;           // MODE_U8: dst and 3 w are multiples of 4; floats: dst of 16 and w of 4
    int kind, rev;             // the value table's kind; channels reversed (gray: a is the source's channel 2)
    float mean[3], stdv[3];
};

template <bool RESIZE, int MODE>
__global__ __launch_bounds__(NT_IMG) void vpass_kernel(const VArgs a) {
    constexpr int NB = 3 * V_PIX;
    constexpr int CH = MODE == MODE_F32 ? 3 : 1;
    __shared__ float lut[MODE == MODE_U8 ? 1 : CH][256];
    if (MODE != MODE_U8) {
        for (int c = 0; c < CH; ++c) lut[c][threadIdx.x] = value_of(a.kind, (int)threadIdx.x, a.mean[c], a.stdv[c]);
        __syncthreads();
    }
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int yy = (int)blockIdx.y * V_ROWS + wave, b = (int)blockIdx.z;
    const int px0 = ((int)blockIdx.x * 64 + (int)(threadIdx.x & 63u)) * V_PIX;
    const int npx = min(V_PIX, a.w - px0);
    if (yy >= a.h || npx <= 0) return;
    const bool full = npx == V_PIX;
    const int nbytes = 3 * npx;

    int ymin = yy, ymax = 1;
    const int32_t *k = nullptr;
    if (RESIZE) {
        ymin = a.table[2 * yy];
        ymax = a.table[2 * yy + 1];
        k = a.table + 2 * (size_t)a.h + (size_t)yy * (size_t)a.ksize;
    }
    const uint8_t *s = a.src + (long long)b * a.src_is + (long long)ymin * a.src_rs + 3 * (long long)px0;
    int acc[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) acc[j] = RESIZE ? ROUND : 0;
    const bool wide = full && a.src_aligned;
    for (int y = 0; y < ymax; ++y, s += a.src_rs) {
        const int ky = RESIZE ? k[y] : 1;
        if (wide) {
            const uint32_t *s4 = (const uint32_t *)s;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const uint32_t v = s4[q];
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[4 * q + j] = tap(acc[4 * q + j], (int)((v >> (8 * j)) & 0xffu), ky);
            }
        } else {
#pragma unroll
            for (int j = 0; j < NB; ++j)
                if (j < nbytes) acc[j] = tap(acc[j], s[j], ky);
        }
    }
    int p[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) p[j] = RESIZE ? finish(acc[j]) : acc[j];

    if (MODE == MODE_U8) {
        uint8_t *d = (uint8_t *)a.dst + (((size_t)b * (size_t)a.h + (size_t)yy) * (size_t)a.w + (size_t)px0) * 3;
        if (full && a.dst_aligned) {
#pragma unroll
            for (int q = 0; q < 3; ++q)
                ((uint32_t *)d)[q] = (uint32_t)p[4 * q] | (uint32_t)p[4 * q + 1] << 8 | (uint32_t)p[4 * q + 2] << 16 |
                                     (uint32_t)p[4 * q + 3] << 24;
        } else {
#pragma unroll
            for (int j = 0; j < NB; ++j)
                if (j < nbytes) d[j] = (uint8_t)p[j];
        }
    } else {
        const size_t plane = (size_t)a.h * (size_t)a.w;
        float *d = (float *)a.dst + (size_t)b * (size_t)CH * plane + (size_t)yy * (size_t)a.w + (size_t)px0;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            float v[V_PIX];
#pragma unroll
            for (int i = 0; i < V_PIX; ++i) {
                const int c0 = a.rev ? p[3 * i + 2] : p[3 * i], c2 = a.rev ? p[3 * i] : p[3 * i + 2];
                int idx;
                if (MODE == MODE_GRAY) idx = gray_of(c0, p[3 * i + 1], c2);
                else idx = c == 0 ? c0 : c == 1 ? p[3 * i + 1] : c2;
                v[i] = lut[c][idx & 255];
            }
            float *dc = d + (size_t)c * plane;
            if (full && a.dst_aligned) {
                *(float4 *)dc = make_float4(v[0], v[1], v[2], v[3]);
            } else {
#pragma unroll
                for (int i = 0; i < V_PIX; ++i)
                    if (i < npx) dc[i] = v[i];
            }
        }
    }
}

// ---- the table cache of one (device, stream): guarded by the scratch entry's mutex ----
constexpr int TABLE_SLOTS = 4;
struct Slot {
    int n_in = 0, n_out = 0;
    unsigned long long stamp = 0;
    hipEvent_t ev = nullptr;  // recorded behind the slot's last upload
    bool pending = false;
};
struct TableCache {
    const unsigned char *dev = nullptr;  // the scratch buffer the slots' device copies live in
    size_t dev_bytes = 0;
    unsigned long long clock = 0;
    Slot slots[TABLE_SLOTS];
};
TableCache *cache_of(StreamScratch *sc) {
    static std::mutex mu;
    static std::map<StreamScratch *, std::unique_ptr<TableCache>> caches;
    std::lock_guard<std::mutex> lock(mu);  // (the lookup only)
    std::unique_ptr<TableCache> &e = caches[sc];
    if (!e) e.reset(new TableCache());
    return e.get();
}

// the device table of (n_in -> n_out), uploaded on s when the cache does not hold it; 0 or an error
int get_table(SyncCall &call, TableCache &tc, int n_in, int n_out, hipStream_t s, const int32_t **table) {
    if (tc.dev != call.dev || tc.dev_bytes != call.sc->dev_bytes) {  // (the buffer was regrown: its tables are gone)
        for (Slot &sl : tc.slots) sl.n_in = sl.n_out = 0;
        tc.dev = call.dev;
        tc.dev_bytes = call.sc->dev_bytes;
    }
    int pick = 0;
    for (int i = 0; i < TABLE_SLOTS; ++i) {
        if (tc.slots[i].n_in == n_in && tc.slots[i].n_out == n_out) {
            tc.slots[i].stamp = ++tc.clock;
            *table = (const int32_t *)(call.dev + (size_t)i * TABLE_MAX_BYTES);
            return 0;
        }
        if (tc.slots[i].stamp < tc.slots[pick].stamp) pick = i;
    }
    Slot &sl = tc.slots[pick];  // (the least recently used: never the call's other axis, which holds the latest stamp)
    hipError_t e = hipSuccess;
    if (!sl.ev) e = hipEventCreateWithFlags(&sl.ev, hipEventDisableTiming);
    if (e == hipSuccess && sl.pending) e = hipEventSynchronize(sl.ev);  // (the staging slot's last upload was read)
    if (e != hipSuccess) return (int)e;
    sl.pending = false;
    sl.n_in = sl.n_out = 0;
    int32_t *host = (int32_t *)(call.host + (size_t)pick * TABLE_MAX_BYTES);
    std::vector<double> w((size_t)ksize_of(n_in, n_out));
    build_table(n_in, n_out, host, w.data());
    unsigned char *dev = call.dev + (size_t)pick * TABLE_MAX_BYTES;
    e = hipMemcpyAsync(dev, host, table_words(n_in, n_out) * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipEventRecord(sl.ev, s);
    if (e != hipSuccess) return (int)e;
    sl.pending = true;
    sl.n_in = n_in;
    sl.n_out = n_out;
    sl.stamp = ++tc.clock;
    *table = (const int32_t *)dev;
    return 0;
}

bool aligned_to(const void *p, size_t n) { return ((uintptr_t)p & (n - 1)) == 0; }

template <int MODE>
void launch_v(bool resize, dim3 grid, hipStream_t s, const VArgs &v) {
    if (resize) hipLaunchKernelGGL((vpass_kernel<true, MODE>), grid, dim3(NT_IMG), 0, s, v);
    else hipLaunchKernelGGL((vpass_kernel<false, MODE>), grid, dim3(NT_IMG), 0, s, v);
}

// validated arguments -> at most two launches on s
int run(const uint8_t *src, long long src_is, long long src_rs, int B, int H, int W, int h, int w, int mode,
        const Transform *t, void *dst, hipStream_t s) {
    const bool need_h = w != W, need_v = h != H;
    const bool use_mid = need_h && (need_v || mode != MODE_U8);
    const long long mid_rs = (3LL * w + 3) / 4 * 4, mid_is = mid_rs * H;
    const size_t tables = (size_t)TABLE_SLOTS * TABLE_MAX_BYTES;
    const size_t need = tables + (use_mid ? (size_t)mid_is * (size_t)B : 0);
    // (no resize: the transform alone or the pass-through copy, one launch that touches the caller's memory only)
    std::unique_ptr<SyncCall> guard;
    TableCache *tc = nullptr;
    uint8_t *mid = nullptr;
    if (need_h || need_v) {
        guard.reset(new SyncCall(SCRATCH_IMAGE, s, need, tables, need));
        if (guard->error()) return guard->error();
        // (asynchronous use of the entry: the growth, the uploads and the launches are ordered on s, and so is the
        // next call's use of the same buffers; nothing is waited for)
        guard->detach();
        tc = cache_of(guard->sc);
        mid = guard->dev + tables;
    }

    if (need_h) {
        const int32_t *table = nullptr;
        const int rc = get_table(*guard, *tc, W, w, s, &table);
        if (rc) return rc;
        HArgs a = {};
        a.src = src;
        a.src_is = src_is;
        a.src_rs = src_rs;
        a.dst = use_mid ? mid : (uint8_t *)dst;
        a.dst_rs = use_mid ? mid_rs : 3LL * w;
        a.dst_is = a.dst_rs * H;
        a.table = table;
        a.H = H;
        a.w = w;
        a.ksize = ksize_of(W, w);
        const dim3 grid((unsigned)((w + H_COLS - 1) / H_COLS), (unsigned)((H + H_ROWS - 1) / H_ROWS), (unsigned)B);
        const size_t lds = (size_t)(2 * H_COLS + H_COLS * a.ksize) * 4;
        if (lds <= H_LDS_MAX) hipLaunchKernelGGL((hpass_kernel<true>), grid, dim3(NT_IMG), lds, s, a);
        else hipLaunchKernelGGL((hpass_kernel<false>), grid, dim3(NT_IMG), 0, s, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
        if (!use_mid) return 0;
        src = mid;
        src_is = mid_is;
        src_rs = mid_rs;
    }
    VArgs v = {};
    v.src = src;
    v.src_is = src_is;
    v.src_rs = src_rs;
    v.dst = dst;
    v.h = h;
    v.w = w;
    if (need_v) {
        const int rc = get_table(*guard, *tc, H, h, s, &v.table);
        if (rc) return rc;
        v.ksize = ksize_of(H, h);
    }
    v.src_aligned = aligned_to(src, 4) && src_rs % 4 == 0 && (B == 1 || src_is % 4 == 0);
    v.dst_aligned = mode == MODE_U8 ? aligned_to(dst, 4) && (3LL * w) % 4 == 0 : aligned_to(dst, 16) && w % 4 == 0;
    if (t) {
        v.kind = t->kind;
        v.rev = t->src_c[0] == 2;
        for (int c = 0; c < 3; ++c) {
            v.mean[c] = t->mean[c];
            v.stdv[c] = t->stdv[c];
        }
    }
    const dim3 grid((unsigned)((w + V_COLS - 1) / V_COLS), (unsigned)((h + V_ROWS - 1) / V_ROWS), (unsigned)B);
    if (mode == MODE_U8) launch_v<MODE_U8>(need_v, grid, s, v);
    else if (mode == MODE_F32) launch_v<MODE_F32>(need_v, grid, s, v);
    else launch_v<MODE_GRAY>(need_v, grid, s, v);
    return (int)hipGetLastError();
}

}  // namespace
}  // namespace fmpnp

using namespace fmpnp;

extern "C" {

int fmpnp_image_resize_u8_async(const unsigned char *src, long long image_stride, long long row_stride, int B, int H,
                                int W, int h, int w, unsigned char *dst, void *hip_stream) {
    const int rc = img::check_args(src, image_stride, row_stride, B, H, W, h, w, dst, 1, 3);
    if (rc) return rc;
    try {  // (nothing throws across the C ABI)
        return run(src, B > 1 ? image_stride : 0, row_stride, B, H, W, h, w, MODE_U8, nullptr, dst,
                   (hipStream_t)hip_stream);
    } catch (...) {
        return FMPNP_ENOMEM;
    }
}

int fmpnp_image_resize_u8(const unsigned char *src, long long image_stride, long long row_stride, int B, int H, int W,
                          int h, int w, unsigned char *dst, void *hip_stream) {
    const int rc = fmpnp_image_resize_u8_async(src, image_stride, row_stride, B, H, W, h, w, dst, hip_stream);
    if (rc) return rc;
    return (int)hipStreamSynchronize((hipStream_t)hip_stream);
}

int fmpnp_image_to_tensor_async(const unsigned char *src, long long image_stride, long long row_stride, int B, int H,
                                int W, int h, int w, int mode, int flags, const float *mean, const float *stdv,
                                float *dst, void *hip_stream) {
    img::Transform t;
    int rc = img::make_transform(mode, flags, mean, stdv, &t);
    if (rc) return rc;
    rc = img::check_args(src, image_stride, row_stride, B, H, W, h, w, dst, 4, t.channels);
    if (rc) return rc;
    try {
        return run(src, B > 1 ? image_stride : 0, row_stride, B, H, W, h, w, t.gray ? MODE_GRAY : MODE_F32, &t, dst,
                   (hipStream_t)hip_stream);
    } catch (...) {
        return FMPNP_ENOMEM;
    }
}

int fmpnp_image_to_tensor(const unsigned char *src, long long image_stride, long long row_stride, int B, int H, int W,
                          int h, int w, int mode, int flags, const float *mean, const float *stdv, float *dst,
                          void *hip_stream) {
    const int rc = fmpnp_image_to_tensor_async(src, image_stride, row_stride, B, H, W, h, w, mode, flags, mean, stdv,
                                               dst, hip_stream);
    if (rc) return rc;
    return (int)hipStreamSynchronize((hipStream_t)hip_stream);
}

}  // extern "C"
