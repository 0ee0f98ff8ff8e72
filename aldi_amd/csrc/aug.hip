// Strong augmentation on the device: the reference builds the strong view of every image on
// the CPU with numpy / scipy (aldi/aug.py:39-60 colour blend chain, :80-91 Gaussian blur, :103-138 random erase, :149-171 MIC
// block mask; a 2048x1024 Cityscapes frame costs tens of ms per image in scipy's gaussian_filter alone).  Here the weak
// view already sits in HBM as HWC uint8 and the strong view is derived from it by these kernels; all RANDOM DRAWS stay on
// the host (aldi_amd/aug.py consumes the numpy / python generators in the reference's order), the kernels get parameters.
//
// Results are bit-identical to the numpy/scipy arithmetic (tests/test_aug_gpu.py vs golden g9 and vs the oracle):
//   * blends: numpy-2 promotion -- a float64 scalar/array times-and-plus a float32 image is evaluated in double
//     (contrast, saturation), a python-float weight on a float32 image stays float32 (brightness); no FMA contraction
//     (-ffp-contract=off), except the 3-term BGR dot of RandomSaturation, which the BLAS behind ndarray.dot evaluates as
//     fma(c2, w2, fma(c1, w1, c0 * w0));
//   * blur: scipy.ndimage.gaussian_filter over all THREE axes of the HWC float32 image (channel axis included), each axis
//     NI_Correlate1D's symmetric form in double -- tmp = x[l]*w0; for j = -r..-1: tmp += (x[l+j] + x[l-j]) * w[j] -- with
//     'reflect' borders, rounded to float32 after every axis;
//   * every op ends with clip(0, 255) and a truncating uint8 cast.
#include "common.h"

namespace {

__device__ __forceinline__ uint8_t clip_u8(double v) { v = v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v); return (uint8_t)v; }
__device__ __forceinline__ uint8_t clip_u8f(float v) { v = v < 0.f ? 0.f : (v > 255.f ? 255.f : v); return (uint8_t)v; }

__global__ __launch_bounds__(256) void sum_u8_kernel(const uint8_t* __restrict__ img, long n, unsigned long long* __restrict__ sum) {
    unsigned long long acc = 0;
    const long n16 = n / 16;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n16; i += (long)gridDim.x * blockDim.x) {
        const uint4 v = reinterpret_cast<const uint4*>(img)[i];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) acc += (w[k] & 0xff) + ((w[k] >> 8) & 0xff) + ((w[k] >> 16) & 0xff) + (w[k] >> 24);
    }
    if (blockIdx.x == 0)
        for (long i = n16 * 16 + threadIdx.x; i < n; i += blockDim.x) acc += img[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0 && acc) atomicAdd(sum, acc);
}

// mode 0: contrast (src = image mean), 1: brightness (src = 0), 2: saturation (src = BGR dot [0.299, 0.587, 0.114])
__global__ __launch_bounds__(256) void blend_kernel(uint8_t* __restrict__ img, long npix, int mode, double w, const unsigned long long* __restrict__ sum) {
    const long p = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (p >= npix) return;
    uint8_t* px = img + p * 3;
    const float w32 = (float)w;                       // python float * float32 array: the product is a float32 product
    const double sw = 1.0 - w;
    if (mode == 1) {
        const float s = (float)(sw * 0.0);            // src_weight * 0 -> python float 0.0, added in float32
#pragma unroll
        for (int c = 0; c < 3; ++c) px[c] = clip_u8f(s + w32 * (float)px[c]);
        return;
    }
    double src;
    if (mode == 0) src = sw * ((double)*sum / (double)(npix * 3));
    else src = sw * fma((double)px[2], 0.114, fma((double)px[1], 0.587, (double)px[0] * 0.299));
#pragma unroll
    for (int c = 0; c < 3; ++c) px[c] = clip_u8(src + (double)(w32 * (float)px[c]));
}

__device__ __forceinline__ int reflect(int i, int n) {
    int p = i % (2 * n);
    if (p < 0) p += 2 * n;
    return p >= n ? 2 * n - 1 - p : p;
}

// one axis of gaussian_filter: `len` elements `stride` apart per line; IN is uint8 (first axis) or float (later axes)
template <typename IN>
__global__ __launch_bounds__(256) void blur_axis_kernel(const IN* __restrict__ in, float* __restrict__ out, long total, int len, long stride,
                                                        const double* __restrict__ wts, int r) {
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= total) return;
    // element index along the axis and the base offset of its line
    const long l = (i / stride) % len;               // position along the filtered axis
    const long base = i - l * stride;
    double tmp = (double)(float)in[i] * wts[r];
    if (l >= r && l + r < len) {                       // interior: no border arithmetic (the reflect() modulo dominated the kernel)
        for (int j = -r; j < 0; ++j) {
            const double a = (double)(float)in[i + (long)j * stride];
            const double b = (double)(float)in[i - (long)j * stride];
            tmp += (a + b) * wts[j + r];
        }
    } else {
        for (int j = -r; j < 0; ++j) {
            const double a = (double)(float)in[base + (long)reflect((int)l + j, len) * stride];
            const double b = (double)(float)in[base + (long)reflect((int)l - j, len) * stride];
            tmp += (a + b) * wts[j + r];
        }
    }
    out[i] = (float)tmp;
}

__global__ __launch_bounds__(256) void f32_to_u8_kernel(const float* __restrict__ in, uint8_t* __restrict__ out, long n) {
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i < n) out[i] = clip_u8f(in[i]);
}

__global__ __launch_bounds__(256) void erase_kernel(uint8_t* __restrict__ img, int W, int h0, int w0, int h, int w, const float* __restrict__ fill) {
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= (long)h * w * 3) return;
    const int c = (int)(i % 3);
    const long q = i / 3;
    const int x = (int)(q % w), y = (int)(q / w);
    img[((long)(h0 + y) * W + (w0 + x)) * 3 + c] = clip_u8f(fill[i] * 255.0f);
}

__global__ __launch_bounds__(256) void mic_kernel(uint8_t* __restrict__ img, int H, int W, const uint8_t* __restrict__ mask, int mh, int mw) {
    const long p = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (p >= (long)H * W) return;
    const int x = (int)(p % W), y = (int)(p / W);
    // cv2.resize INTER_NEAREST: src = min(floor(dst * (src_size / dst_size)), src_size - 1), scale in double
    int sy = (int)floor((double)y * ((double)mh / (double)H)), sx = (int)floor((double)x * ((double)mw / (double)W));
    sy = sy < mh - 1 ? sy : mh - 1;
    sx = sx < mw - 1 ? sx : mw - 1;
    if (!mask[sy * mw + sx]) { img[p * 3] = 0; img[p * 3 + 1] = 0; img[p * 3 + 2] = 0; }
}

__global__ __launch_bounds__(256) void hwc_to_chw_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, long npix) {
    const long p = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (p >= npix) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c * npix + p] = in[p * 3 + c];
}


// ------------------------------------------------------------------------------------------------ batched strong views
// Three launches per batch, each driven by the aldi_aug_desc / aldi_aug_fill_job tables (include/aldi_hip.h):
//   1. batch_sums_kernel: the contrast means' exact byte sums (sum_u8_kernel's integer sum, 32 KiB per workgroup);
//   2. fill_kernel: erase fills replayed from numpy's own MT19937 stream (a snapshot per segment, state refills in LDS);
//   3. view_kernel: a 16 x 64 pixel tile per workgroup -- the halo'd tile goes through the colour chain on load (pointwise,
//      so exact on the reflected halo too), then the three gaussian_filter axes (rows, columns from LDS; channels in
//      registers), the erase rects (bytes from the arena), the MIC mask, the store in the output layout.
constexpr int kSumChunk = 32768;                     // bytes per workgroup of batch_sums_kernel
constexpr int kTH = 16, kTW = 64, kHalo = ALDI_AUG_HALO;
constexpr int kPitch = (kTW + 2 * kHalo) * 3;        // floats per LDS row: 80 pixels x 3 channels (stride 3 per lane: no bank conflicts)

// the image that owns block b: the last i with begin(i) <= b (begins are non-decreasing; empty images share their successor's)
template <typename F>
__device__ __forceinline__ int owner(int n, int b, F begin) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (begin(mid) <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(256) void batch_sums_kernel(aldi_aug_desc* __restrict__ desc, int n) {
    const int i = owner(n, (int)blockIdx.x, [&](int k) { return desc[k].sum_begin; });
    const uint8_t* src = desc[i].src;
    const long nbytes = (long)desc[i].H * desc[i].W * 3;
    const long beg = (long)((int)blockIdx.x - desc[i].sum_begin) * kSumChunk;
    const long end = beg + kSumChunk < nbytes ? beg + kSumChunk : nbytes;
    unsigned long long acc = 0;
    long tail = beg;
    if ((reinterpret_cast<uintptr_t>(src) & 15) == 0) {
        tail = beg + (end - beg) / 16 * 16;
        for (long o = beg + threadIdx.x * 16L; o < tail; o += 256L * 16) {
            const uint4 v = *reinterpret_cast<const uint4*>(src + o);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) acc += (w[k] & 0xff) + ((w[k] >> 8) & 0xff) + ((w[k] >> 16) & 0xff) + (w[k] >> 24);
        }
    }
    for (long o = tail + threadIdx.x; o < end; o += 256) acc += src[o];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0 && acc) atomicAdd(&desc[i].sum, acc);
}

__device__ __forceinline__ uint32_t mt_temper(uint32_t y) {
    y ^= (y >> 11);
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    return y ^ (y >> 18);
}
__device__ __forceinline__ uint32_t mt_twist(uint32_t u, uint32_t v) {
    return (((u & 0x80000000u) | (v & 0x7fffffffu)) >> 1) ^ ((v & 1u) ? 0x9908b0dfu : 0u);
}
// MT19937 state refill in LDS by 256 threads.  Element i reads s[i + 1] (old), and s[i + 397] (old, i < 227) or s[i - 227]
// (already rewritten, i >= 227): the runs [0, 227), [227, 454), [454, 623) are each independent, then 623 (reads the new s[0]).
__device__ __forceinline__ void mt_refill(uint32_t* s) {
    const int t = threadIdx.x;
    uint32_t v = 0;
    if (t < 227) v = s[t + 397] ^ mt_twist(s[t], s[t + 1]);
    __syncthreads();
    if (t < 227) s[t] = v;
    __syncthreads();
    if (t < 227) v = s[t] ^ mt_twist(s[t + 227], s[t + 228]);
    __syncthreads();
    if (t < 227) s[t + 227] = v;
    __syncthreads();
    if (t < 169) v = s[t + 227] ^ mt_twist(s[t + 454], s[t + 455]);
    __syncthreads();
    if (t < 169) s[t + 454] = v;
    __syncthreads();
    if (t == 0) s[623] = s[396] ^ mt_twist(s[623], s[0]);
    __syncthreads();
}

// numpy random_sample(): ((a >> 5) * 2^26 + (b >> 6)) / 2^53 from two consecutive outputs; stored as erase_kernel stores the
// float32 cast of it (the reference's assignment into the float32 image) times 255
__global__ __launch_bounds__(256) void fill_kernel(const aldi_aug_fill_job* __restrict__ jobs, uint8_t* __restrict__ arena) {
    __shared__ uint32_t s[624];
    __shared__ uint32_t carry;                        // raw last word of the previous state: first half of a straddling pair
    const aldi_aug_fill_job jb = jobs[blockIdx.x];
    for (int i = threadIdx.x; i < 624; i += 256) s[i] = jb.snap[i];
    __syncthreads();
    int lo = jb.pos;
    if (lo >= 624) { mt_refill(s); lo = 0; }
    const long nw = 2L * jb.ndoubles;
    long kbase = -(long)lo;                           // output k of the job is s[k - kbase] of the current state
    uint8_t* out = arena + jb.out_off;
    for (;;) {
        for (int idx = lo + (int)threadIdx.x; idx < 624; idx += 256) {
            const long k = idx + kbase;               // k odd: the second word of pair k >> 1 (its first: idx - 1, or carry at idx 0)
            if ((k & 1) && k < nw) {
                const uint32_t a = mt_temper(idx == 0 ? carry : s[idx - 1]) >> 5, b = mt_temper(s[idx]) >> 6;
                const double d = ((double)a * 67108864.0 + (double)b) / 9007199254740992.0;
                out[k >> 1] = clip_u8f((float)d * 255.0f);
            }
        }
        if (kbase + 624 >= nw) break;
        __syncthreads();
        if (threadIdx.x == 0) carry = s[623];
        mt_refill(s);
        kbase += 624;
        lo = 0;
    }
}

// blend_kernel's arithmetic on one pixel (mode 0 contrast with the image mean, 1 brightness, 2 saturation)
__device__ __forceinline__ void blend_px(uint8_t p[3], int mode, double w, double mean) {
    const float w32 = (float)w;
    const double sw = 1.0 - w;
    if (mode == 1) {
        const float s = (float)(sw * 0.0);
#pragma unroll
        for (int c = 0; c < 3; ++c) p[c] = clip_u8f(s + w32 * (float)p[c]);
        return;
    }
    const double src = mode == 0 ? sw * mean : sw * fma((double)p[2], 0.114, fma((double)p[1], 0.587, (double)p[0] * 0.299));
#pragma unroll
    for (int c = 0; c < 3; ++c) p[c] = clip_u8(src + (double)(w32 * (float)p[c]));
}

__device__ __forceinline__ float pick3(int i, float v0, float v1, float v2) { return i == 0 ? v0 : (i == 1 ? v1 : v2); }

__global__ __launch_bounds__(256) void view_kernel(const aldi_aug_desc* __restrict__ desc, int n, const uint8_t* __restrict__ arena) {
    __shared__ float s_in[(kTH + 2 * kHalo) * kPitch];   // colour-chained input tile + halo (30 KiB)
    __shared__ float s_h[kTH * kPitch];                  // after the row axis (15 KiB)
    const int i = owner(n, (int)blockIdx.x, [&](int k) { return desc[k].tile_begin; });
    const aldi_aug_desc& d = desc[i];
    const int H = d.H, W = d.W, flags = d.flags;
    const bool blur = flags & ALDI_AUG_BLUR;
    int R = blur ? d.radius : 0;
    R = R < 0 ? 0 : (R > kHalo ? kHalo : R);
    const int tiles_x = (W + kTW - 1) / kTW, t = (int)blockIdx.x - d.tile_begin;
    const int y0 = (t / tiles_x) * kTH, x0 = (t % tiles_x) * kTW;
    const long plane = (long)H * W;
    const uint8_t* src = d.src;
    const bool chw_in = flags & ALDI_AUG_CHW_IN;
    const double mean = (flags & ALDI_AUG_COLOUR) ? (double)d.sum / (double)(plane * 3) : 0.0;

    // load + colour chain, halo rows / columns through scipy's 'reflect' index
    const int LW = kTW + 2 * R, LH = kTH + 2 * R;
    for (int q = threadIdx.x; q < LH * LW; q += 256) {
        const int lr = q / LW, lc = q - lr * LW;
        const long o = (long)reflect(y0 - R + lr, H) * W + reflect(x0 - R + lc, W);
        uint8_t p[3];
        if (chw_in) { p[0] = src[o]; p[1] = src[o + plane]; p[2] = src[o + 2 * plane]; }
        else { p[0] = src[o * 3]; p[1] = src[o * 3 + 1]; p[2] = src[o * 3 + 2]; }
        if (flags & ALDI_AUG_COLOUR) {
            blend_px(p, 0, d.wc, mean);
            blend_px(p, 1, d.wb, 0.0);
            blend_px(p, 2, d.ws, 0.0);
        }
        if (flags & ALDI_AUG_GRAY) blend_px(p, 2, d.wg, 0.0);
        float* dst = s_in + lr * kPitch + lc * 3;
        dst[0] = (float)p[0]; dst[1] = (float)p[1]; dst[2] = (float)p[2];
    }
    __syncthreads();

    double w[kHalo + 1];
#pragma unroll
    for (int k = 0; k <= kHalo; ++k) w[k] = d.taps[k];
    const double wc = blur ? d.taps[R] : 1.0;
    if (blur) {                                          // axis 0 (rows): NI_Correlate1D's symmetric form in double, f32 result
        for (int q = threadIdx.x; q < kTH * LW; q += 256) {
            const int r = q / LW, cc = q - r * LW;
            const float* x = s_in + (r + R) * kPitch + cc * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                double tmp = (double)x[c] * wc;
                for (int k = 0; k < R; ++k) {
                    const int j = (R - k) * kPitch;
                    tmp += ((double)x[c - j] + (double)x[c + j]) * w[k];
                }
                s_h[r * kPitch + cc * 3 + c] = (float)tmp;
            }
        }
        __syncthreads();
    }

    for (int p = threadIdx.x; p < kTH * kTW; p += 256) {
        const int r = p / kTW, c = p - r * kTW, y = y0 + r, x = x0 + c;
        if (y >= H || x >= W) continue;
        uint8_t o[3];
        if (blur) {
            float v[3];
            const float* hx = s_h + r * kPitch + (c + R) * 3;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {                 // axis 1 (columns)
                double tmp = (double)hx[ch] * wc;
                for (int k = 0; k < R; ++k) {
                    const int j = (R - k) * 3;
                    tmp += ((double)hx[ch - j] + (double)hx[ch + j]) * w[k];
                }
                v[ch] = (float)tmp;
            }
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {                 // axis 2 (channels), reflected over length 3
                double tmp = (double)v[ch] * wc;
                for (int k = 0; k < R; ++k) {
                    const int j = k - R;
                    tmp += ((double)pick3(reflect(ch + j, 3), v[0], v[1], v[2]) + (double)pick3(reflect(ch - j, 3), v[0], v[1], v[2])) * w[k];
                }
                o[ch] = clip_u8f((float)tmp);
            }
        } else {
            const float* sx = s_in + r * kPitch + c * 3;
            o[0] = (uint8_t)sx[0]; o[1] = (uint8_t)sx[1]; o[2] = (uint8_t)sx[2];
        }
        for (int e = 0; e < d.nerase; ++e) {                 // a later rect overwrites an earlier one
            const int ry = y - d.rect[e][0], rx = x - d.rect[e][1];
            if ((unsigned)ry < (unsigned)d.rect[e][2] && (unsigned)rx < (unsigned)d.rect[e][3]) {
                const uint8_t* f = arena + d.fill_off[e] + ((long)ry * d.rect[e][3] + rx) * 3;
                o[0] = f[0]; o[1] = f[1]; o[2] = f[2];
            }
        }
        if (d.mask) {                                        // mic_kernel's cv2.resize INTER_NEAREST index
            const int mh = d.mh, mw = d.mw;
            int sy = (int)floor((double)y * ((double)mh / (double)H)), sx = (int)floor((double)x * ((double)mw / (double)W));
            sy = sy < mh - 1 ? sy : mh - 1;
            sx = sx < mw - 1 ? sx : mw - 1;
            if (!d.mask[sy * mw + sx]) { o[0] = 0; o[1] = 0; o[2] = 0; }
        }
        const long px = (long)y * W + x;
        if (flags & ALDI_AUG_CHW_OUT) { d.dst[px] = o[0]; d.dst[px + plane] = o[1]; d.dst[px + 2 * plane] = o[2]; }
        else { d.dst[px * 3] = o[0]; d.dst[px * 3 + 1] = o[1]; d.dst[px * 3 + 2] = o[2]; }
    }
}

inline dim3 grid1(long n) { return dim3((unsigned)((n + 255) / 256)); }

}  // namespace

extern "C" int aldi_aug_sum_u8(const unsigned char* img, long n, unsigned long long* sum, aldi_stream_t stream) {
    if (!img || !sum || n <= 0) return aldi_set_error_msg(ALDI_ERR_ARG, "aug_sum_u8: bad args");
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemsetAsync(sum, 0, 8, st);
    if (e != hipSuccess) return aldi_set_error(e, __FILE__, __LINE__);
    long blocks = (n / 16 + 255) / 256;
    blocks = blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks);
    hipLaunchKernelGGL(sum_u8_kernel, dim3((unsigned)blocks), dim3(256), 0, st, img, n, sum);
    ALDI_CHECK_LAUNCH();
    return ALDI_OK;
}

extern "C" int aldi_aug_blend(unsigned char* img, int H, int W, int mode, double w, const unsigned long long* sum, aldi_stream_t stream) {
    if (!img || H <= 0 || W <= 0 || mode < 0 || mode > 2 || (mode == 0 && !sum)) return aldi_set_error_msg(ALDI_ERR_ARG, "aug_blend: bad args");
    const long npix = (long)H * W;
    hipLaunchKernelGGL(blend_kernel, grid1(npix), dim3(256), 0, static_cast<hipStream_t>(stream), img, npix, mode, w, sum);
    ALDI_CHECK_LAUNCH();
    return ALDI_OK;
}

extern "C" int aldi_aug_blur(const unsigned char* img, unsigned char* out, float* tmp0, float* tmp1, int H, int W, const double* weights, int radius,
                             aldi_stream_t stream) {
    if (!img || !out || !tmp0 || !tmp1 || !weights || H <= 0 || W <= 0 || radius < 0 || radius > 64) return aldi_set_error_msg(ALDI_ERR_ARG, "aug_blur: bad args");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long n = (long)H * W * 3;
    hipLaunchKernelGGL(blur_axis_kernel<unsigned char>, grid1(n), dim3(256), 0, st, img, tmp0, n, H, (long)W * 3, weights, radius);     // axis 0 (rows)
    hipLaunchKernelGGL(blur_axis_kernel<float>, grid1(n), dim3(256), 0, st, (const float*)tmp0, tmp1, n, W, 3L, weights, radius);        // axis 1 (columns)
    hipLaunchKernelGGL(blur_axis_kernel<float>, grid1(n), dim3(256), 0, st, (const float*)tmp1, tmp0, n, 3, 1L, weights, radius);        // axis 2 (channels)
    hipLaunchKernelGGL(f32_to_u8_kernel, grid1(n), dim3(256), 0, st, (const float*)tmp0, out, n);
    ALDI_CHECK_LAUNCH();
    return ALDI_OK;
}

extern "C" int aldi_aug_erase(unsigned char* img, int H, int W, int h0, int w0, int h, int w, const float* fill, aldi_stream_t stream) {
    if (!img || !fill || h0 < 0 || w0 < 0 || h <= 0 || w <= 0 || h0 + h > H || w0 + w > W) return aldi_set_error_msg(ALDI_ERR_ARG, "aug_erase: rectangle outside the image");
    hipLaunchKernelGGL(erase_kernel, grid1((long)h * w * 3), dim3(256), 0, static_cast<hipStream_t>(stream), img, W, h0, w0, h, w, fill);
    ALDI_CHECK_LAUNCH();
    return ALDI_OK;
}

extern "C" int aldi_aug_mic(unsigned char* img, int H, int W, const unsigned char* mask, int mh, int mw, aldi_stream_t stream) {
    if (!img || !mask || H <= 0 || W <= 0 || mh <= 0 || mw <= 0) return aldi_set_error_msg(ALDI_ERR_ARG, "aug_mic: bad args");
    hipLaunchKernelGGL(mic_kernel, grid1((long)H * W), dim3(256), 0, static_cast<hipStream_t>(stream), img, H, W, mask, mh, mw);
    ALDI_CHECK_LAUNCH();
    return ALDI_OK;
}

extern "C" int aldi_aug_hwc_to_chw(const unsigned char* in, unsigned char* out, int H, int W, aldi_stream_t stream) {
    if (!in || !out || H <= 0 || W <= 0) return aldi_set_error_msg(ALDI_ERR_ARG, "aug_hwc_to_chw: bad args");
    hipLaunchKernelGGL(hwc_to_chw_kernel, grid1((long)H * W), dim3(256), 0, static_cast<hipStream_t>(stream), in, out, (long)H * W);
    ALDI_CHECK_LAUNCH();
    return ALDI_OK;
}

extern "C" int aldi_aug_batch_sums(aldi_aug_desc* desc, int n, int nblocks, aldi_stream_t stream) {
    if (!desc || n <= 0 || nblocks < 0) return aldi_set_error_msg(ALDI_ERR_ARG, "aug_batch_sums: bad args");
    if (nblocks == 0) return ALDI_OK;
    hipLaunchKernelGGL(batch_sums_kernel, dim3((unsigned)nblocks), dim3(256), 0, static_cast<hipStream_t>(stream), desc, n);
    ALDI_CHECK_LAUNCH();
    return ALDI_OK;
}

extern "C" int aldi_aug_batch_fills(const aldi_aug_fill_job* jobs, int njobs, unsigned char* arena, aldi_stream_t stream) {
    if (njobs < 0 || (njobs > 0 && (!jobs || !arena))) return aldi_set_error_msg(ALDI_ERR_ARG, "aug_batch_fills: bad args");
    if (njobs == 0) return ALDI_OK;
    hipLaunchKernelGGL(fill_kernel, dim3((unsigned)njobs), dim3(256), 0, static_cast<hipStream_t>(stream), jobs, arena);
    ALDI_CHECK_LAUNCH();
    return ALDI_OK;
}

extern "C" int aldi_aug_batch_view(const aldi_aug_desc* desc, int n, int ntiles, const unsigned char* arena, aldi_stream_t stream) {
    if (!desc || n <= 0 || ntiles <= 0) return aldi_set_error_msg(ALDI_ERR_ARG, "aug_batch_view: bad args");
    hipLaunchKernelGGL(view_kernel, dim3((unsigned)ntiles), dim3(256), 0, static_cast<hipStream_t>(stream), desc, n, arena);
    ALDI_CHECK_LAUNCH();
    return ALDI_OK;
}
