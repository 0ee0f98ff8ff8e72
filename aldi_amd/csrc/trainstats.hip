// Training metrics on the device (aldi_amd/events.py; detectron2's EventStorage writers and _log_classification_stats):
//   aldi_metrics_record     one row of a device ring per iteration: the step's loss scalars and head counters, copied bit for bit
//   aldi_box_cls_stats      the five counts of FastRCNNOutputLayers' classification statistics per row range
//   aldi_rpn_label_counts   positive / negative anchors of the sampled RPN labels
// Latency kernels: a handful of workgroups, integer sums only (wave shuffles, then int32 atomics: the result does not depend on the order).
#include "common.h"

namespace {

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ------------------------------------------------------------------------------------------------ metrics_record
// The source pointers travel in the launch's arguments (eager-mode losses are fresh allocations every step: nothing to upload).
struct RecordArgs {
    const uint32_t* f[ALDI_METRICS_MAX_FLOATS];
    int* i[ALDI_METRICS_MAX_INTS];
};

__global__ __launch_bounds__(64) void metrics_record_kernel(RecordArgs A, int nf, int ni, int clear_i, uint32_t* __restrict__ ring_f,
                                                            int* __restrict__ ring_i, int* __restrict__ ring_iter, int slot, int iteration,
                                                            int* __restrict__ first_bad_iter) {
    const int t = threadIdx.x;                       // one wave: lane t owns float column t and (t < 32) counter column t
    uint32_t bits = 0;
    if (t < nf) bits = *A.f[t];
    ring_f[(size_t)slot * ALDI_METRICS_MAX_FLOATS + t] = bits;
    const bool bad = (bits & 0x7f800000u) == 0x7f800000u;      // exponent all ones: +-inf or NaN
    const unsigned long long any_bad = __ballot(bad);
    if (t < ALDI_METRICS_MAX_INTS) {
        int v = 0;
        if (t < ni) {
            v = *A.i[t];
            if (clear_i) *A.i[t] = 0;
        }
        ring_i[(size_t)slot * ALDI_METRICS_MAX_INTS + t] = v;
    }
    if (t == 0) {
        ring_iter[slot] = iteration;
        if (any_bad != 0ull && *first_bad_iter == -1) *first_bad_iter = iteration;
    }
}

// ------------------------------------------------------------------------------------------------ box_cls_stats
// 16 lanes per row: lane l reads columns l, l + 16, ... of 0 .. K (one 64-byte segment per step), the 16 candidates meet in four
// shuffle steps.  Order of two candidates: a NaN beats a number, a larger number beats a smaller one, otherwise the lower column.
constexpr int kStatThreads = 256, kRowLanes = 16, kRowsPerBlock = kStatThreads / kRowLanes;
struct StatRanges {
    int n;
    int r0[ALDI_STATS_MAX_RANGES], r1[ALDI_STATS_MAX_RANGES];
    int* out[ALDI_STATS_MAX_RANGES];
};

__device__ __forceinline__ bool better(float av, int ai, float bv, int bi) {
    const bool an = av != av, bn = bv != bv;
    if (an != bn) return an;
    if (!an && av != bv) return av > bv;
    return ai < bi;
}

template <typename T>
__global__ __launch_bounds__(kStatThreads) void box_cls_stats_kernel(const T* __restrict__ pred, int Cp, int K, const int* __restrict__ cls,
                                                                     StatRanges A) {
    __shared__ int red[kStatThreads / 64][5];
    const int ri = blockIdx.y;                       // (uniform: kernel-argument arrays indexed by a scalar)
    const int r0 = A.r0[ri], r1 = A.r1[ri];
    if (r1 <= r0) return;
    const int tid = threadIdx.x, l = tid & (kRowLanes - 1), g = tid / kRowLanes;
    int cnt[5] = {0, 0, 0, 0, 0};
    for (int rb = r0 + blockIdx.x * kRowsPerBlock; rb < r1; rb += gridDim.x * kRowsPerBlock) {   // (uniform bounds: every lane shuffles)
        const int r = rb + g;
        const bool live = r < r1;
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        if (live) {
            const T* row = pred + (size_t)r * Cp;
            for (int j = l; j <= K; j += kRowLanes) {
                const float v = Elem<T>::ld(row + j);
                if (better(v, j, bv, bi)) { bv = v; bi = j; }
            }
        }
#pragma unroll
        for (int o = kRowLanes / 2; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        if (live && l == 0) {
            const int c = cls[r];
            const bool fg = c >= 0 && c < K;
            cnt[0] += 1;
            cnt[1] += bi == c;
            cnt[2] += fg;
            cnt[3] += fg && bi == c;
            cnt[4] += fg && bi == K;
        }
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const int s = wave_sum_i(cnt[k]);
        if ((tid & 63) == 0) red[tid >> 6][k] = s;
    }
    __syncthreads();
    if (tid < 5) {
        int s = 0;
#pragma unroll
        for (int w = 0; w < kStatThreads / 64; ++w) s += red[w][tid];
        if (s) atomicAdd(A.out[ri] + tid, s);
    }
}

// ------------------------------------------------------------------------------------------------ rpn_label_counts
constexpr int kCountThreads = 256;

__global__ __launch_bounds__(kCountThreads) void rpn_label_counts_kernel(const int* __restrict__ labels, long total, int* __restrict__ out) {
    __shared__ int red[kCountThreads / 64][2];
    const long tid = (long)blockIdx.x * kCountThreads + threadIdx.x, nthr = (long)gridDim.x * kCountThreads;
    // 16-byte loads over the aligned body, scalar loads for the (at most 3 + 3) elements around it
    long head = (long)((16 - (reinterpret_cast<uintptr_t>(labels) & 15)) & 15) / 4;
    if (head > total) head = total;
    const long nvec = (total - head) / 4;
    int pos = 0, neg = 0;
    const int4* body = reinterpret_cast<const int4*>(labels + head);
    for (long i = tid; i < nvec; i += nthr) {
        const int4 v = body[i];
        pos += (v.x == 1) + (v.y == 1) + (v.z == 1) + (v.w == 1);
        neg += (v.x == 0) + (v.y == 0) + (v.z == 0) + (v.w == 0);
    }
    const long tail0 = head + nvec * 4;
    const long nedge = head + (total - tail0);
    if (tid < nedge) {
        const int v = labels[tid < head ? tid : tail0 + (tid - head)];
        pos += v == 1;
        neg += v == 0;
    }
    pos = wave_sum_i(pos);
    neg = wave_sum_i(neg);
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = pos; red[threadIdx.x >> 6][1] = neg; }
    __syncthreads();
    if (threadIdx.x < 2) {
        int s = 0;
#pragma unroll
        for (int w = 0; w < kCountThreads / 64; ++w) s += red[w][threadIdx.x];
        if (s) atomicAdd(out + threadIdx.x, s);
    }
}

}  // namespace

extern "C" int aldi_metrics_record(const float* const* src_f, int nf, int* const* src_i, int ni, int clear_i, float* ring_f, int* ring_i,
                                   int* ring_iter, int slot, int slots, int iteration, int* first_bad_iter, aldi_stream_t stream) {
    if (!ring_f || !ring_i || !ring_iter || !first_bad_iter) return aldi_set_error_msg(ALDI_ERR_ARG, "metrics_record: null pointer");
    if (nf < 0 || nf > ALDI_METRICS_MAX_FLOATS || ni < 0 || ni > ALDI_METRICS_MAX_INTS)
        return aldi_set_error_msg(ALDI_ERR_ARG, "metrics_record: at most 64 float sources and 32 counters");
    if (slots < 1 || slot < 0 || slot >= slots) return aldi_set_error_msg(ALDI_ERR_ARG, "metrics_record: slot outside the ring");
    if ((nf && !src_f) || (ni && !src_i)) return aldi_set_error_msg(ALDI_ERR_ARG, "metrics_record: null source table");
    RecordArgs A;
    for (int j = 0; j < ALDI_METRICS_MAX_FLOATS; ++j) {
        A.f[j] = j < nf ? reinterpret_cast<const uint32_t*>(src_f[j]) : nullptr;
        if (j < nf && !A.f[j]) return aldi_set_error_msg(ALDI_ERR_ARG, "metrics_record: null float source");
    }
    for (int j = 0; j < ALDI_METRICS_MAX_INTS; ++j) {
        A.i[j] = j < ni ? src_i[j] : nullptr;
        if (j < ni && !A.i[j]) return aldi_set_error_msg(ALDI_ERR_ARG, "metrics_record: null counter source");
    }
    hipLaunchKernelGGL(metrics_record_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), A, nf, ni, clear_i,
                       reinterpret_cast<uint32_t*>(ring_f), ring_i, ring_iter, slot, iteration, first_bad_iter);
    ALDI_CHECK_LAUNCH();
    return ALDI_OK;
}

extern "C" int aldi_box_cls_stats(const void* pred, int Cp, int K, int R, const int* cls, const int* r0, const int* r1, int* const* out,
                                  int nranges, int dtype, aldi_stream_t stream) {
    if (!pred || !cls || !r0 || !r1 || !out) return aldi_set_error_msg(ALDI_ERR_ARG, "box_cls_stats: null pointer");
    if (nranges < 1 || nranges > ALDI_STATS_MAX_RANGES || K < 1 || Cp <= K || R < 0)
        return aldi_set_error_msg(ALDI_ERR_ARG, "box_cls_stats: 1 .. 8 ranges, K >= 1, Cp > K");
    if (dtype != ALDI_F32 && dtype != ALDI_BF16) return aldi_set_error_msg(ALDI_ERR_ARG, "box_cls_stats: dtype");
    StatRanges A;
    A.n = nranges;
    int longest = 0;
    for (int i = 0; i < ALDI_STATS_MAX_RANGES; ++i) {
        A.r0[i] = A.r1[i] = 0;
        A.out[i] = nullptr;
        if (i >= nranges) continue;
        if (r0[i] < 0 || r1[i] > R || !out[i]) return aldi_set_error_msg(ALDI_ERR_ARG, "box_cls_stats: range outside [0, R] or null counters");
        A.r0[i] = r0[i], A.r1[i] = r1[i], A.out[i] = out[i];
        if (r1[i] - r0[i] > longest) longest = r1[i] - r0[i];
    }
    if (longest <= 0) return ALDI_OK;
    int bx = cdiv(longest, 4 * kRowsPerBlock);       // four rows per 16-lane group, at most 8 workgroups per range
    bx = bx < 1 ? 1 : (bx > 8 ? 8 : bx);
    const dim3 grid(bx, nranges);
    if (dtype == ALDI_F32)
        hipLaunchKernelGGL(box_cls_stats_kernel<float>, grid, dim3(kStatThreads), 0, static_cast<hipStream_t>(stream),
                           static_cast<const float*>(pred), Cp, K, cls, A);
    else
        hipLaunchKernelGGL(box_cls_stats_kernel<bf16_t>, grid, dim3(kStatThreads), 0, static_cast<hipStream_t>(stream),
                           static_cast<const bf16_t*>(pred), Cp, K, cls, A);
    ALDI_CHECK_LAUNCH();
    return ALDI_OK;
}

extern "C" int aldi_rpn_label_counts(const int* labels, int N, int L, int* out, aldi_stream_t stream) {
    if (!labels || !out) return aldi_set_error_msg(ALDI_ERR_ARG, "rpn_label_counts: null pointer");
    if (N < 0 || L < 0) return aldi_set_error_msg(ALDI_ERR_ARG, "rpn_label_counts: negative size");
    const long total = (long)N * L;
    if (total == 0) return ALDI_OK;
    int blocks = cdiv(total, (long)kCountThreads * 4 * 8);   // eight 16-byte loads per thread, at most 64 workgroups
    blocks = blocks < 1 ? 1 : (blocks > 64 ? 64 : blocks);
    hipLaunchKernelGGL(rpn_label_counts_kernel, dim3(blocks), dim3(kCountThreads), 0, static_cast<hipStream_t>(stream), labels, total, out);
    ALDI_CHECK_LAUNCH();
    return ALDI_OK;
}
