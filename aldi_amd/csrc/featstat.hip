// Feature-space statistics for the domain-gap diagnostic (aldi_amd/featurespace.py; reference tools/visualize_featurespace.py):
//   aldi_pool_rows[_counted]  one pooled fp32 vector per image (p6) / per proposal (the 7x7x256 RoIAlign output), compacted by the
//                             device proposal counts
//   aldi_moments_accum        fp64 first and second moments of those vectors, ordered reduction (no floating-point atomics)
//   aldi_project2             the 2-component projection of the kept vectors
// The pooled maps never leave HBM: the host sees a C x C matrix per level.
#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------------ pool_rows
// One workgroup per input row [S][C].  A thread owns 16 bytes of the channel axis (8 bf16 / 4 fp32) and every G-th position of S
// (G = 256 / (C / V) thread groups); the G partial vectors meet in the LDS and are combined in group order.  C / V > 256 (C > 2048 bf16):
// the channel axis is walked in slices of 256 lanes.  HBM traffic: x once, out once.
constexpr int kPoolThreads = 256;
constexpr long kMaxGrid = 0xffffffL;             // workgroups of 256 threads per launch (grid x block below 2^32 work-items)

template <typename T> struct PoolVec;
template <> struct PoolVec<float> {
    static constexpr int V = 4;
    __device__ static __forceinline__ void ld(const float* p, float v[4]) { load4(p, v); }
};
template <> struct PoolVec<bf16_t> {
    static constexpr int V = 8;
    __device__ static __forceinline__ void ld(const bf16_t* p, float v[8]) {
        uint4 t = *reinterpret_cast<const uint4*>(p);
        v[0] = __uint_as_float(t.x << 16); v[1] = __uint_as_float(t.x & 0xffff0000u);
        v[2] = __uint_as_float(t.y << 16); v[3] = __uint_as_float(t.y & 0xffff0000u);
        v[4] = __uint_as_float(t.z << 16); v[5] = __uint_as_float(t.z & 0xffff0000u);
        v[6] = __uint_as_float(t.w << 16); v[7] = __uint_as_float(t.w & 0xffff0000u);
    }
};

template <typename T, bool MAX>
__global__ __launch_bounds__(kPoolThreads) void pool_rows_kernel(const T* __restrict__ x, int P, int S, int C, const int* __restrict__ count,
                                                                 int N, float* __restrict__ out, long row_off, long out_rows,
                                                                 int* __restrict__ total) {
    constexpr int V = PoolVec<T>::V;
    __shared__ float red[kPoolThreads * V];
    const long r = blockIdx.x;
    long dst = r;
    if (count) {                                   // compaction: the prefix of the (clamped) counts of the images before this one
                                                   // (N is a batch: at most 16 images in this engine, so every workgroup sums the counts itself)
        const int n = (int)(r / P), p = (int)(r % P);
        int base = 0, mine = 0, all = 0;
        for (int i = 0; i < N; ++i) {
            int c = count[i];
            c = c < 0 ? 0 : (c > P ? P : c);
            if (i < n) base += c;
            if (i == n) mine = c;
            all += c;
        }
        if (r == 0 && threadIdx.x == 0 && total) *total = all;
        if (p >= mine) return;                     // (uniform over the workgroup)
        dst = base + p;
    }
    dst += row_off;
    if (dst < 0 || dst >= out_rows) return;
    const int lanesC = C / V;
    const int lc = lanesC < kPoolThreads ? lanesC : kPoolThreads;
    const int G = kPoolThreads / lc;
    const int tid = threadIdx.x;
    const int g = tid / lc, l = tid - g * lc;
    const bool active = g < G;
    const T* xr = x + (size_t)r * S * C;
    float* orow = out + (size_t)dst * C;
    for (int c0 = 0; c0 < lanesC; c0 += lc) {      // (one pass unless C / V > 256)
        const int cl = c0 + l;
        float acc[V];
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] = MAX ? -INFINITY : 0.f;
        if (active && cl < lanesC) {
            const T* px = xr + (size_t)cl * V;
#pragma unroll 4
            for (int s = g; s < S; s += G) {
                float v[V];
                PoolVec<T>::ld(px + (size_t)s * C, v);
#pragma unroll
                for (int j = 0; j < V; ++j) acc[j] = MAX ? fmaxf(acc[j], v[j]) : acc[j] + v[j];
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < V; ++j) red[tid * V + j] = acc[j];
        __syncthreads();
        const int width = lc * V;                  // floats of this channel slice; group g's partial vector starts at g * width
        for (int e = tid; e < width; e += kPoolThreads) {
            if (c0 * V + e >= C) continue;
            float v = red[e];
            for (int q = 1; q < G; ++q) v = MAX ? fmaxf(v, red[q * width + e]) : v + red[q * width + e];
            orow[c0 * V + e] = MAX ? v : v / (float)S;
        }
    }
}

template <typename T>
int launch_pool(const void* x, long rows, int P, int S, int C, int mode, const int* count, int N, float* out, long row_off, long out_rows,
                int* total, hipStream_t st) {
    dim3 grid((unsigned)rows), block(kPoolThreads);
    if (mode == ALDI_POOL_MAX)
        hipLaunchKernelGGL((pool_rows_kernel<T, true>), grid, block, 0, st, (const T*)x, P, S, C, count, N, out, row_off, out_rows, total);
    else
        hipLaunchKernelGGL((pool_rows_kernel<T, false>), grid, block, 0, st, (const T*)x, P, S, C, count, N, out, row_off, out_rows, total);
    ALDI_CHECK_LAUNCH();
    return ALDI_OK;
}

int pool_args_ok(const void* x, long rows, int S, int C, int dtype, int mode, const float* out, long row_off) {
    if (!x || !out || rows < 0 || rows > kMaxGrid || S <= 0 || C <= 0 || C % 8 || row_off < 0) return 0;
    if (dtype != ALDI_F32 && dtype != ALDI_BF16) return 0;
    return mode == ALDI_POOL_AVG || mode == ALDI_POOL_MAX;
}

// ------------------------------------------------------------------------------------------------ moments_accum
// gram = X^T X over 64 x 64 tiles of the upper triangle (tile row <= tile column; the finalize launch mirrors them) x at most 32 row
// ranges.  A workgroup (256 threads, 4 x 4 outputs each in fp64) walks its range in slabs of 16 rows staged in the LDS as fp32 and adds
// the rows in order; rows past the range and columns past C are staged as zeros.  The diagonal tiles also sum their 64 columns.
constexpr int kMT = 64, kMRows = 16, kMSlots = 32, kMThreads = 256;

__host__ __device__ inline int moments_rows_per_slot(int n) {
    int per = (n + kMSlots - 1) / kMSlots;
    per = (per + 63) / 64 * 64;
    return per < 64 ? 64 : per;
}
__host__ __device__ inline int moments_tiles(int C) { return (C + kMT - 1) / kMT; }

__device__ __forceinline__ int moments_n(int n, const int* n_dev, int n_cap) {
    if (!n_dev) return n;
    int v = *n_dev;
    return v < 0 ? 0 : (v > n_cap ? n_cap : v);
}

__device__ __forceinline__ void upper_tile(int t, int T, int& ti, int& tj) {
    ti = 0;
    while (t >= T - ti) { t -= T - ti; ++ti; }
    tj = ti + t;
}

__global__ __launch_bounds__(kMThreads) void moments_part_kernel(const float* __restrict__ X, int n_host, const int* __restrict__ n_dev, int n_cap,
                                                                 int C, double* __restrict__ part, double* __restrict__ psum) {
    __shared__ __attribute__((aligned(16))) float sA[kMRows][kMT];
    __shared__ __attribute__((aligned(16))) float sB[kMRows][kMT];
    const int n = moments_n(n_host, n_dev, n_cap);
    const int per = moments_rows_per_slot(n);
    const int slot = blockIdx.y;
    const long r0 = (long)slot * per;
    if (r0 >= n) return;
    const long r1 = r0 + per < n ? r0 + per : n;
    const int T = moments_tiles(C);
    int ti, tj;
    upper_tile(blockIdx.x, T, ti, tj);
    const int tid = threadIdx.x;
    const int tx = tid & 15, ty = tid >> 4;
    const int lrow = tid >> 4, lcol = (tid & 15) * 4;        // staging: one float4 of each operand slab per thread
    const int ca = ti * kMT + lcol, cb = tj * kMT + lcol;
    double acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
    double colsum = 0.0;
    for (long rb = r0; rb < r1; rb += kMRows) {
        const long row = rb + lrow;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
        if (row < r1) {
            if (ca < C) a = *reinterpret_cast<const float4*>(X + (size_t)row * C + ca);      // C % 8 == 0: a float4 never straddles C
            if (cb < C) b = *reinterpret_cast<const float4*>(X + (size_t)row * C + cb);
        }
        __syncthreads();
        *reinterpret_cast<float4*>(&sA[lrow][lcol]) = a;
        *reinterpret_cast<float4*>(&sB[lrow][lcol]) = b;
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < kMRows; ++k) {
            const float4 av = *reinterpret_cast<const float4*>(&sA[k][ty * 4]);
            const float4 bv = *reinterpret_cast<const float4*>(&sB[k][tx * 4]);
            const double ad[4] = {(double)av.x, (double)av.y, (double)av.z, (double)av.w};
            const double bd[4] = {(double)bv.x, (double)bv.y, (double)bv.z, (double)bv.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_fma(ad[i], bd[j], acc[i][j]);
        }
        if (ti == tj && tid < kMT) {
#pragma unroll 4
            for (int k = 0; k < kMRows; ++k) colsum += (double)sA[k][tid];
        }
    }
    double* pt = part + ((size_t)slot * gridDim.x + blockIdx.x) * (kMT * kMT);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) pt[(ty * 4 + i) * kMT + tx * 4 + j] = acc[i][j];
    if (ti == tj && tid < kMT && ti * kMT + tid < C) psum[(size_t)slot * C + ti * kMT + tid] = colsum;
}

// grid (upper tiles, 16): a thread adds one tile element's range partials in range order, then into the accumulator (and its mirror)
__global__ __launch_bounds__(kMThreads) void moments_finish_kernel(int n_host, const int* __restrict__ n_dev, int n_cap, int C,
                                                                   const double* __restrict__ part, const double* __restrict__ psum,
                                                                   double* __restrict__ sum, double* __restrict__ gram, double* __restrict__ count) {
    const int n = moments_n(n_host, n_dev, n_cap);
    if (n <= 0) return;                            // accumulators stay bit-unchanged
    const int per = moments_rows_per_slot(n);
    const int slots = (n + per - 1) / per;
    const int T = moments_tiles(C);
    int ti, tj;
    upper_tile(blockIdx.x, T, ti, tj);
    const int e = blockIdx.y * kMThreads + threadIdx.x;
    const int i = e / kMT, j = e % kMT;
    const int gi = ti * kMT + i, gj = tj * kMT + j;
    if (gi < C && gj < C) {
        const double* p = part + (size_t)blockIdx.x * (kMT * kMT) + e;
        const size_t stride = (size_t)gridDim.x * (kMT * kMT);
        double v = p[0];
        for (int s = 1; s < slots; ++s) v += p[s * stride];
        gram[(size_t)gi * C + gj] += v;
        if (ti != tj) gram[(size_t)gj * C + gi] += v;
    }
    if (ti == tj && blockIdx.y == 0 && threadIdx.x < kMT && ti * kMT + (int)threadIdx.x < C) {
        const int c = ti * kMT + threadIdx.x;
        double v = psum[c];
        for (int s = 1; s < slots; ++s) v += psum[(size_t)s * C + c];
        sum[c] += v;
    }
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) count[0] += (double)n;
}

// ------------------------------------------------------------------------------------------------ project2
// one wave per row: lane l takes channels l, l + 64, ...; the two fp64 dot products meet in a butterfly (same order every run)
__global__ __launch_bounds__(256) void project2_kernel(const float* __restrict__ X, long n, int C, const double* __restrict__ mean,
                                                       const double* __restrict__ comp, float* __restrict__ Y) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;                          // (uniform over the wave)
    const float* xr = X + (size_t)row * C;
    double a0 = 0.0, a1 = 0.0;
    for (int c = lane; c < C; c += 64) {
        const double d = (double)xr[c] - mean[c];
        a0 = __builtin_fma(d, comp[c], a0);
        a1 = __builtin_fma(d, comp[C + c], a1);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a0 += __shfl_xor(a0, o, 64);
        a1 += __shfl_xor(a1, o, 64);
    }
    if (lane == 0) {
        Y[row * 2] = (float)a0;
        Y[row * 2 + 1] = (float)a1;
    }
}

}  // namespace

extern "C" int aldi_pool_rows(const void* x, long rows, int S, int C, int dtype, int mode, float* out, long row_off, long out_rows,
                              aldi_stream_t stream) {
    if (!pool_args_ok(x, rows, S, C, dtype, mode, out, row_off)) return aldi_set_error_msg(ALDI_ERR_ARG, "pool_rows: bad args (C % 8 == 0, S >= 1, dtype, mode)");
    if (row_off + rows > out_rows) return aldi_set_error_msg(ALDI_ERR_ARG, "pool_rows: row_off + rows exceeds out_rows");
    if (rows == 0) return ALDI_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return dtype == ALDI_BF16 ? launch_pool<bf16_t>(x, rows, 1, S, C, mode, nullptr, 0, out, row_off, out_rows, nullptr, st)
                              : launch_pool<float>(x, rows, 1, S, C, mode, nullptr, 0, out, row_off, out_rows, nullptr, st);
}

extern "C" int aldi_pool_rows_counted(const void* x, int N, int P, int S, int C, int dtype, int mode, const int* count, float* out, long row_off,
                                      long out_rows, int* total, aldi_stream_t stream) {
    if (N <= 0 || P <= 0 || !count || !total || !pool_args_ok(x, (long)N * P, S, C, dtype, mode, out, row_off))
        return aldi_set_error_msg(ALDI_ERR_ARG, "pool_rows_counted: bad args (N, P >= 1, C % 8 == 0, S >= 1, count and total on the device)");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long rows = (long)N * P;
    return dtype == ALDI_BF16 ? launch_pool<bf16_t>(x, rows, P, S, C, mode, count, N, out, row_off, out_rows, total, st)
                              : launch_pool<float>(x, rows, P, S, C, mode, count, N, out, row_off, out_rows, total, st);
}

extern "C" size_t aldi_moments_workspace(int C) {
    if (C <= 0) return 0;
    const size_t T = (size_t)moments_tiles(C), upper = T * (T + 1) / 2;
    return (size_t)kMSlots * (upper * kMT * kMT + (size_t)C) * sizeof(double);
}

extern "C" int aldi_moments_accum(const float* X, int n, const int* n_dev, int n_cap, int C, double* sum, double* gram, double* count,
                                  void* workspace, aldi_stream_t stream) {
    if (!sum || !gram || !count || !workspace || C <= 0 || C % 8 || n < 0 || n_cap < 0)
        return aldi_set_error_msg(ALDI_ERR_ARG, "moments_accum: bad args (C % 8 == 0, accumulators and workspace required)");
    const int cap = n_dev ? n_cap : n;             // the most rows the launch can touch
    if (cap == 0) return ALDI_OK;
    if (!X) return aldi_set_error_msg(ALDI_ERR_ARG, "moments_accum: X is null");
    const int T = moments_tiles(C), upper = T * (T + 1) / 2;
    double* part = static_cast<double*>(workspace);
    double* psum = part + (size_t)kMSlots * upper * kMT * kMT;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // a row range holds at least 64 rows: no more than ceil(cap / 64) of the 32 ranges can be occupied (the image level adds a batch of 1-2 rows)
    const int ranges = cap / 64 + 1 < kMSlots ? cap / 64 + 1 : kMSlots;
    hipLaunchKernelGGL(moments_part_kernel, dim3(upper, ranges), dim3(kMThreads), 0, st, X, n, n_dev, cap, C, part, psum);
    ALDI_CHECK_LAUNCH();
    hipLaunchKernelGGL(moments_finish_kernel, dim3(upper, kMT * kMT / kMThreads), dim3(kMThreads), 0, st, n, n_dev, cap, C, (const double*)part,
                       (const double*)psum, sum, gram, count);
    ALDI_CHECK_LAUNCH();
    return ALDI_OK;
}

extern "C" int aldi_project2(const float* X, long n, int C, const double* mean, const double* comp, float* Y, aldi_stream_t stream) {
    if (n < 0 || C <= 0 || !mean || !comp) return aldi_set_error_msg(ALDI_ERR_ARG, "project2: bad args");
    if (n == 0) return ALDI_OK;
    if (!X || !Y || (n + 3) / 4 > kMaxGrid) return aldi_set_error_msg(ALDI_ERR_ARG, "project2: bad args");
    hipLaunchKernelGGL(project2_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), X, n, C, mean, comp, Y);
    ALDI_CHECK_LAUNCH();
    return ALDI_OK;
}
