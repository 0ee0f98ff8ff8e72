// Weak-view geometry on the device: detectron2's ResizeShortestEdge + horizontal RandomFlip of a uint8
// image, i.e. Pillow's `Image.resize(BILINEAR)` -- integer fixed point, horizontal pass first and ROUNDED TO UINT8, then the
// vertical pass -- with the flip as an index reversal at the store.  The per-axis coefficient and bounds tables are built on the
// host in doubles, in Pillow's operation order (aldi_amd/aug.py resize_tables); the kernels only do
//     out = clip(((1 << 21) + sum_t in[xmin + t] * k[t]) >> 22, 0, 255)          (int32: 255 * (2^22 + ksize / 2) + 2^21 < 2^31)
// so the bytes equal Pillow's (tests/test_weak_aug_gpu.py against tests/golden/pil_bilinear.npz).
//
// One batch = one table of aldi_geom_desc in device memory, images of any sizes.  Two arms, chosen per image by aldi_geom_plan:
//   * fused (one launch): a 16 x 64 output tile per workgroup.  The input rows the tile's vertical taps touch are resampled
//     horizontally into LDS as uint8 (at most ALDI_GEOM_LDS_ROWS rows x 64 px x 3 = 18 KiB), the vertical pass reads them there;
//   * two-pass (two launches, one thread per pixel): horizontal into a uint8 HWC scratch image, then vertical.  Takes the heavy
//     downscales, whose row window (~ 16 * scale + 2 * ceil(scale) + 1 rows) does not fit, and is the plain reference arm.
// Every source index is clamped into [0, insz) by axis_taps whatever the tables say; an LDS row outside the staged window is
// skipped.
//
// The full mapper chain: detectron2's RandomCrop slices the decoded array BEFORE the resize, so a cropped view is
// the same resize of a window of the raw image.  The descriptor's tail (src_h, src_w, y0, x0) says where the h x w window lies; all three
// kernels read the source through it (window_of), the tables are those of the window's sizes, and axis_taps clamps every tap into the
// window, so nothing outside the window is read, let alone outside the image; a window that is not inside the raw image makes every
// kernel return for that image.  The vertical flip and the R <-> B exchange are per-pixel permutations that commute with the resize:
// they sit at the store, next to the horizontal flip.
#include "common.h"

static_assert(sizeof(aldi_geom_desc) == 3 * sizeof(void*) + 18 * sizeof(int), "aldi_geom_desc: aldi_amd/aug.py _GeomDesc mirrors this layout");

namespace {

constexpr int kTH = ALDI_GEOM_TH, kTW = ALDI_GEOM_TW, kRows = ALDI_GEOM_LDS_ROWS;
constexpr int kHalf = 1 << 21, kShift = 22;

// the image that owns block b: the last i with begin(i) <= b (begins are non-decreasing; an image without blocks in this
// launch shares its successor's begin and is never chosen)
template <typename F>
__device__ __forceinline__ int owner(int n, int b, F begin) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (begin(mid) <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// one axis of one image: coefficient rows k[outsz][ks], bounds b[outsz][2] = (first input index, tap count); ks == 0: the axis
// keeps its size and Pillow skips the pass (one tap of weight 1, which the fixed-point form reproduces exactly)
struct Axis {
    const int* k;
    const int* b;
    int ks, insz;
};

__device__ __forceinline__ Axis axis_of(const int* tab, int k_off, int b_off, int ks, int insz) {
    return Axis{tab + k_off, tab + b_off, ks, insz};
}

// taps of output index o: first input index, count, coefficient row; clamped so that [mn, mn + cnt) lies inside [0, insz)
__device__ __forceinline__ void axis_taps(const Axis& a, int o, int& mn, int& cnt, const int*& k) {
    if (a.ks <= 0) {
        mn = o < a.insz ? o : a.insz - 1;
        cnt = 1;
        k = nullptr;
        return;
    }
    mn = a.b[2 * o];
    cnt = a.b[2 * o + 1];
    mn = mn < 0 ? 0 : (mn > a.insz ? a.insz : mn);
    const int room = a.insz - mn < a.ks ? a.insz - mn : a.ks;
    cnt = cnt < 0 ? 0 : (cnt > room ? room : cnt);
    k = a.k + (long)o * a.ks;
}

__device__ __forceinline__ int coef(const int* k, int t) { return k ? k[t] : (1 << kShift); }

__device__ __forceinline__ uint8_t fix_u8(int acc) {
    acc >>= kShift;
    return (uint8_t)(acc < 0 ? 0 : (acc > 255 ? 255 : acc));
}

// the source window of one image inside its raw image (the descriptor's tail; all zero = the window is the whole image): pixel
// (r, c) of the window is raw pixel base + r * stride + c, a CHW plane is `plane` pixels.  ok = false: the window is not inside the
// raw image and nothing of it may be read.
struct Window {
    long base, plane;
    int stride;
    bool ok;
};

__host__ __device__ __forceinline__ Window window_of(const aldi_geom_desc& d) {
    if (!(d.src_h | d.src_w | d.y0 | d.x0)) return Window{0, (long)d.h * d.w, d.w, d.h > 0 && d.w > 0};
    const bool ok = d.h > 0 && d.w > 0 && d.x0 >= 0 && d.y0 >= 0 && (long)d.x0 + d.w <= d.src_w && (long)d.y0 + d.h <= d.src_h;
    return Window{(long)d.y0 * d.src_w + d.x0, (long)d.src_h * d.src_w, d.src_w, ok};
}

// pixel (r, mn + t), t < cnt, of a source window weighted along its row
__device__ __forceinline__ void hpass_px(const uint8_t* __restrict__ src, bool chw, const Window& win, int r, int mn, int cnt, const int* k,
                                         uint8_t out[3]) {
    int a0 = kHalf, a1 = kHalf, a2 = kHalf;
    const long o = win.base + (long)r * win.stride + mn, plane = win.plane;
    if (chw) {
        for (int t = 0; t < cnt; ++t) {
            const int c = coef(k, t);
            a0 += (int)src[o + t] * c;
            a1 += (int)src[o + t + plane] * c;
            a2 += (int)src[o + t + 2 * plane] * c;
        }
    } else {
        for (int t = 0; t < cnt; ++t) {
            const int c = coef(k, t);
            const uint8_t* p = src + (o + t) * 3;
            a0 += (int)p[0] * c;
            a1 += (int)p[1] * c;
            a2 += (int)p[2] * c;
        }
    }
    out[0] = fix_u8(a0); out[1] = fix_u8(a1); out[2] = fix_u8(a2);
}

__device__ __forceinline__ void store_px(const aldi_geom_desc& d, int y, int x, const uint8_t v[3]) {
    const int xo = (d.flags & ALDI_GEOM_HFLIP) ? d.new_w - 1 - x : x, yo = (d.flags & ALDI_GEOM_VFLIP) ? d.new_h - 1 - y : y;
    const long px = (long)yo * d.new_w + xo, plane = (long)d.new_h * d.new_w;
    const bool swap = d.flags & ALDI_GEOM_SWAP_RB;
    const uint8_t c0 = swap ? v[2] : v[0], c2 = swap ? v[0] : v[2];
    if (d.flags & ALDI_GEOM_CHW_OUT) { d.dst[px] = c0; d.dst[px + plane] = v[1]; d.dst[px + 2 * plane] = c2; }
    else { d.dst[px * 3] = c0; d.dst[px * 3 + 1] = v[1]; d.dst[px * 3 + 2] = c2; }
}

__global__ __launch_bounds__(256) void resize_fused_kernel(const aldi_geom_desc* __restrict__ desc, int n, const int* __restrict__ tab) {
    __shared__ uint8_t s_rows[kRows * kTW * 3];          // horizontally resampled input rows of this tile, uint8 as Pillow keeps them
    const int i = owner(n, (int)blockIdx.x, [&](int k) { return desc[k].tile_begin; });
    const aldi_geom_desc& d = desc[i];
    if (!(d.flags & ALDI_GEOM_FUSED)) return;
    const int tiles_x = (d.new_w + kTW - 1) / kTW, t = (int)blockIdx.x - d.tile_begin;
    const int y0 = (t / tiles_x) * kTH, x0 = (t % tiles_x) * kTW;
    const Window win = window_of(d);
    if (!win.ok || y0 >= d.new_h) return;
    const int th = d.new_h - y0 < kTH ? d.new_h - y0 : kTH, tw = d.new_w - x0 < kTW ? d.new_w - x0 : kTW;
    const Axis X = axis_of(tab, d.xk_off, d.xb_off, d.xks, d.w), Y = axis_of(tab, d.yk_off, d.yb_off, d.yks, d.h);
    int r0, c0, r1, c1;
    const int* kk;
    axis_taps(Y, y0, r0, c0, kk);
    axis_taps(Y, y0 + th - 1, r1, c1, kk);
    const int nrows = r1 + c1 - r0;                      // bounds are non-decreasing: [r0, r1 + c1) covers every row of the tile
    if (nrows <= 0 || nrows > kRows) return;             // (aldi_geom_plan sends such an image through the two-pass arm)
    const bool chw = d.flags & ALDI_GEOM_CHW_IN;
    for (int q = threadIdx.x; q < nrows * tw; q += 256) {
        const int lr = q / tw, lc = q - lr * tw;
        int mn, cnt;
        axis_taps(X, x0 + lc, mn, cnt, kk);
        uint8_t v[3];
        hpass_px(d.src, chw, win, r0 + lr, mn, cnt, kk, v);
        uint8_t* s = s_rows + (lr * kTW + lc) * 3;
        s[0] = v[0]; s[1] = v[1]; s[2] = v[2];
    }
    __syncthreads();
    for (int p = threadIdx.x; p < kTH * kTW; p += 256) {
        const int r = p / kTW, c = p - r * kTW;
        if (r >= th || c >= tw) continue;
        int mn, cnt;
        axis_taps(Y, y0 + r, mn, cnt, kk);
        int a0 = kHalf, a1 = kHalf, a2 = kHalf;
        for (int tt = 0; tt < cnt; ++tt) {
            const int lr = mn - r0 + tt;
            if ((unsigned)lr >= (unsigned)nrows) continue;
            const int cf = coef(kk, tt);
            const uint8_t* s = s_rows + (lr * kTW + c) * 3;
            a0 += (int)s[0] * cf; a1 += (int)s[1] * cf; a2 += (int)s[2] * cf;
        }
        const uint8_t v[3] = {fix_u8(a0), fix_u8(a1), fix_u8(a2)};
        store_px(d, y0 + r, x0 + c, v);
    }
}

// two-pass arm, launch 1: scratch[h][new_w][3] = horizontal pass of src (a copy into HWC when the width stays)
__global__ __launch_bounds__(256) void resize_h_kernel(const aldi_geom_desc* __restrict__ desc, int n, const int* __restrict__ tab) {
    const int i = owner(n, (int)blockIdx.x, [&](int k) { return desc[k].h_begin; });
    const aldi_geom_desc& d = desc[i];
    if ((d.flags & ALDI_GEOM_FUSED) || !d.tmp) return;
    const long p = ((long)blockIdx.x - d.h_begin) * 256 + threadIdx.x;
    const Window win = window_of(d);
    if (!win.ok || p >= (long)d.h * d.new_w) return;
    const int r = (int)(p / d.new_w), x = (int)(p - (long)r * d.new_w);
    const Axis X = axis_of(tab, d.xk_off, d.xb_off, d.xks, d.w);
    int mn, cnt;
    const int* kk;
    axis_taps(X, x, mn, cnt, kk);
    uint8_t v[3];
    hpass_px(d.src, d.flags & ALDI_GEOM_CHW_IN, win, r, mn, cnt, kk, v);
    uint8_t* o = d.tmp + p * 3;
    o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
}

// two-pass arm, launch 2: dst = vertical pass of the scratch image, flipped / laid out at the store
__global__ __launch_bounds__(256) void resize_v_kernel(const aldi_geom_desc* __restrict__ desc, int n, const int* __restrict__ tab) {
    const int i = owner(n, (int)blockIdx.x, [&](int k) { return desc[k].v_begin; });
    const aldi_geom_desc& d = desc[i];
    if ((d.flags & ALDI_GEOM_FUSED) || !d.tmp) return;
    const long p = ((long)blockIdx.x - d.v_begin) * 256 + threadIdx.x;
    if (!window_of(d).ok || p >= (long)d.new_h * d.new_w) return;   // (the scratch image of such a window was never written)
    const int y =(int)(p / d.new_w), x = (int)(p - (long)y * d.new_w);
    const Axis Y = axis_of(tab, d.yk_off, d.yb_off, d.yks, d.h);
    int mn, cnt;
    const int* kk;
    axis_taps(Y, y, mn, cnt, kk);
    int a0 = kHalf, a1 = kHalf, a2 = kHalf;
    for (int t = 0; t < cnt; ++t) {
        const int cf = coef(kk, t);
        const uint8_t* s = d.tmp + ((long)(mn + t) * d.new_w + x) * 3;
        a0 += (int)s[0] * cf; a1 += (int)s[1] * cf; a2 += (int)s[2] * cf;
    }
    const uint8_t v[3] = {fix_u8(a0), fix_u8(a1), fix_u8(a2)};
    store_px(d, y, x, v);
}

}  // namespace

extern "C" int aldi_geom_plan(const int* ybounds, int h, int new_h, int* fused) {
    if (!fused || h <= 0 || new_h <= 0 || (h != new_h && !ybounds)) return aldi_set_error_msg(ALDI_ERR_ARG, "geom_plan: bad args");
    *fused = 0;
    if (!aldi_tuning().resize_fused) return ALDI_OK;
    if (h != new_h) {
        for (int y0 = 0; y0 < new_h; y0 += kTH) {
            const int y1 = (y0 + kTH < new_h ? y0 + kTH : new_h) - 1;
            if (ybounds[2 * y1] + ybounds[2 * y1 + 1] - ybounds[2 * y0] > kRows) return ALDI_OK;
        }
    }
    *fused = 1;
    return ALDI_OK;
}

extern "C" int aldi_geom_window(const aldi_geom_desc* desc, long* base, long* plane, int* stride, int* inside) {
    if (!desc || !base || !plane || !stride || !inside) return aldi_set_error_msg(ALDI_ERR_ARG, "geom_window: bad args");
    const Window win = window_of(*desc);
    *base = win.base; *plane = win.plane; *stride = win.stride; *inside = win.ok ? 1 : 0;
    return ALDI_OK;
}

extern "C" int aldi_geom_batch_resize(const aldi_geom_desc* desc, int n, const int* tables, int ntiles, int nh_blocks, int nv_blocks,
                                      aldi_stream_t stream) {
    if (!desc || n <= 0 || ntiles < 0 || nh_blocks < 0 || nv_blocks < 0 || (nh_blocks > 0) != (nv_blocks > 0))
        return aldi_set_error_msg(ALDI_ERR_ARG, "geom_batch_resize: bad args");
    if (!tables) return aldi_set_error_msg(ALDI_ERR_ARG, "geom_batch_resize: null tables");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (ntiles) hipLaunchKernelGGL(resize_fused_kernel, dim3((unsigned)ntiles), dim3(256), 0, st, desc, n, tables);
    if (nh_blocks) {
        hipLaunchKernelGGL(resize_h_kernel, dim3((unsigned)nh_blocks), dim3(256), 0, st, desc, n, tables);
        hipLaunchKernelGGL(resize_v_kernel, dim3((unsigned)nv_blocks), dim3(256), 0, st, desc, n, tables);
    }
    ALDI_CHECK_LAUNCH();
    return ALDI_OK;
}
