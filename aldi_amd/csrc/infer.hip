// Inference-side box geometry: detections back to the original image (aldi_detector_postprocess) and the class-wise merge of the
// detections of several test-time views (aldi_tta_merge).  Both sit beside the training step: nothing here is on its launch sequence.
//
// PARITY UNPINNED: the arithmetic restates detectron2 v0.6 -- detector_postprocess (Boxes.scale / clip / nonempty), TransformList.inverse()
// .apply_box on a float32 array (flip, scale, min / max over the corners) and GeneralizedRCNNWithTTA._merge_detections =
// fast_rcnn_inference_single_image over the union of the views -- in float32, one operation per stage, in that order.  The file is built
// with -ffp-contract=off, so no multiply is fused with the flip's subtract.
#include "nms.h"
#include "sortscan.h"
#include "../../include/aldi_hip.h"

namespace {

constexpr int kMergeCap = 8192;   // candidates per original image: the LDS sort's 64 KiB and nms_scan_launch's 128 words

// flip, two scale stages, corner min / max, clamp -- aldi_box_tfm's order (include/aldi_hip.h)
__device__ __forceinline__ float4 tfm_box(float x1, float y1, float x2, float y2, const aldi_box_tfm t) {
    if (t.flip_w >= 0.f) { x1 = t.flip_w - x1; x2 = t.flip_w - x2; }
    x1 = x1 * t.sx0; y1 = y1 * t.sy0; x2 = x2 * t.sx0; y2 = y2 * t.sy0;
    x1 = x1 * t.sx1; y1 = y1 * t.sy1; x2 = x2 * t.sx1; y2 = y2 * t.sy1;
    float4 o = make_float4(fminf(x1, x2), fminf(y1, y2), fmaxf(x1, x2), fmaxf(y1, y2));
    o.x = fminf(fmaxf(o.x, 0.f), t.clip_w); o.y = fminf(fmaxf(o.y, 0.f), t.clip_h);
    o.z = fminf(fmaxf(o.z, 0.f), t.clip_w); o.w = fminf(fmaxf(o.w, 0.f), t.clip_h);
    return o;
}

// (boxes of the public interface are read and written as four floats: a caller's [.][4] view need not be 16-byte aligned)
__device__ __forceinline__ float4 load_box(const float* p) { return make_float4(p[0], p[1], p[2], p[3]); }
__device__ __forceinline__ void store_box(float* p, const float4 b) { p[0] = b.x; p[1] = b.y; p[2] = b.z; p[3] = b.w; }

// one wave per image, 64 rows per round: transform, drop the empty boxes, compact stably (ballot + prefix count, as det_finish_kernel)
__global__ __launch_bounds__(64) void postprocess_kernel(const float* boxes, const float* scores, const int* classes, const int* count, int D,
                                                         const aldi_box_tfm* tfm, float* out_boxes, float* out_scores, int* out_classes, int* out_count) {
    const int n = blockIdx.x, lane = threadIdx.x;
    const int cnt = min(max(count[n], 0), D);
    const aldi_box_tfm t = tfm[n];
    const long base = (long)n * D;
    int nout = 0;
    for (int j0 = 0; j0 < cnt; j0 += 64) {
        const int j = j0 + lane;
        float4 b = make_float4(0, 0, 0, 0);
        float s = 0.f;
        int c = -1;
        bool keep = false;
        if (j < cnt) {
            const float4 r = load_box(boxes + (base + j) * 4);
            b = tfm_box(r.x, r.y, r.z, r.w, t);
            s = scores[base + j]; c = classes[base + j];
            keep = (b.z - b.x) > 0.f && (b.w - b.y) > 0.f;
        }
        const unsigned long long m = __ballot(keep);
        if (keep) {
            const int q = nout + __popcll(m & ((1ull << lane) - 1ull));     // q <= j < D
            store_box(out_boxes + (base + q) * 4, b); out_scores[base + q] = s; out_classes[base + q] = c;
        }
        nout += __popcll(m);
    }
    for (int j = nout + lane; j < D; j += 64) { store_box(out_boxes + (base + j) * 4, make_float4(0, 0, 0, 0)); out_scores[base + j] = 0.f; out_classes[base + j] = -1; }
    if (lane == 0) out_count[n] = nout;
}

struct MergeIn {
    const float* boxes; const float* scores; const int* classes; const int* count; const aldi_box_tfm* tfm;
    int A, D, K;
    float floor;
};

// row `t` = a * D + j of image b: a candidate?  -> its transformed box, score and class
__device__ __forceinline__ bool merge_row(const MergeIn& in, int b, int t, float4& box, float& score, int& cls) {
    const int a = t / in.D, j = t - a * in.D;
    if (a >= in.A) return false;
    const long v = (long)b * in.A + a;
    if (j >= min(max(in.count[v], 0), in.D)) return false;
    const long r = v * in.D + j;
    const float4 q = load_box(in.boxes + r * 4);
    score = in.scores[r]; cls = in.classes[r];
    if (!(isfinite(q.x) && isfinite(q.y) && isfinite(q.z) && isfinite(q.w) && isfinite(score)) || cls < 0 || cls >= in.K) return false;
    box = tfm_box(q.x, q.y, q.z, q.w, in.tfm[v]);
    return score > in.floor;
}

// one workgroup per original image: the candidates of all its views, sorted in LDS by (score descending, flat index ascending) -- the key
// layout of det_candidates_kernel / det_sort_kernel -- and materialised in that order for the NMS kernels of nms.h
__global__ __launch_bounds__(1024) void merge_sort_kernel(const MergeIn in, int p2, int cap, float4* __restrict__ boxes, float* __restrict__ scores,
                                                          int* __restrict__ cats, int* __restrict__ valid, int* __restrict__ cnt) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long sk[];   // p2 keys, then the candidate counter (no static LDS in
    int& s_cnt = *reinterpret_cast<int*>(sk + p2);                            // front of the keys: their 8-byte accesses stay aligned)
    const int b = blockIdx.x, total = in.A * in.D;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    for (int i0 = 0; i0 < p2; i0 += blockDim.x) {          // (p2 is a multiple of the 1024 threads: every wave is whole in every round)
        const int i = i0 + threadIdx.x;
        float4 box; float s = 0.f; int c;
        const bool ok = i < total && merge_row(in, b, i, box, s, c);
        sk[i] = ok ? (((unsigned long long)(~float_key_asc(s)) << 32) | (unsigned)i) : ~0ull;
        const unsigned long long m = __ballot(ok);
        if ((threadIdx.x & 63) == 0 && m) atomicAdd(&s_cnt, __popcll(m));
    }
    __syncthreads();
    const int n = min(s_cnt, cap);
    bitonic_sort_u64(sk, p2);
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int t = min((int)(sk[i] & 0xffffffffu), total - 1);
        float4 box = make_float4(0, 0, 0, 0); float s = 0.f; int c = -1;
        const bool ok = merge_row(in, b, t, box, s, c);
        const long slot = (long)b * cap + i;
        boxes[slot] = box; scores[slot] = s; cats[slot] = c; valid[slot] = ok ? 1 : 0;
    }
    if (threadIdx.x == 0) cnt[b] = n;
}

// first min(keep_count, topk) survivors -> the output rows; the rest zero boxes, zero scores, class -1
__global__ __launch_bounds__(64) void merge_finish_kernel(const float4* __restrict__ boxes, const float* __restrict__ scores, const int* __restrict__ cats,
                                                          const int* __restrict__ keep, const int* __restrict__ keep_count, int cap, int topk,
                                                          float* out_boxes, float* out_scores, int* out_classes, int* out_count) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int kc = min(min(max(keep_count[b], 0), topk), cap);
    for (int j = lane; j < topk; j += 64) {
        float4 bx = make_float4(0, 0, 0, 0);
        float s = 0.f;
        int c = -1;
        if (j < kc) {
            const long slot = (long)b * cap + min(max(keep[(long)b * cap + j], 0), cap - 1);
            bx = boxes[slot]; s = scores[slot]; c = cats[slot];
        }
        store_box(out_boxes + ((long)b * topk + j) * 4, bx); out_scores[(long)b * topk + j] = s; out_classes[(long)b * topk + j] = c;
    }
    if (lane == 0) out_count[b] = kc;
}

// the call's capacity: the views' rows rounded up to the 64-box words of the NMS mask
inline long merge_cap(long rows) { return rows < 64 ? 64 : (rows + 63) / 64 * 64; }

}  // namespace

extern "C" int aldi_detector_postprocess(const float* boxes, const float* scores, const int* classes, const int* count, int N, int D,
                                         const aldi_box_tfm* tfm, float* out_boxes, float* out_scores, int* out_classes, int* out_count,
                                         aldi_stream_t stream) {
    if (!boxes || !scores || !classes || !count || !tfm || !out_boxes || !out_scores || !out_classes || !out_count)
        return aldi_set_error_msg(ALDI_ERR_ARG, "detector_postprocess: null pointer");
    if (N < 0 || D < 0 || (long)N * D > 0x7fffffffL / 4) return aldi_set_error_msg(ALDI_ERR_ARG, "detector_postprocess: bad N or D");
    if (N == 0) return ALDI_OK;
    hipLaunchKernelGGL(postprocess_kernel, dim3(N), dim3(64), 0, static_cast<hipStream_t>(stream), boxes, scores, classes, count, D, tfm,
                       out_boxes, out_scores, out_classes, out_count);
    ALDI_CHECK_LAUNCH();
    return ALDI_OK;
}

extern "C" size_t aldi_tta_merge_workspace(int B, int A, int D) {
    if (B < 1 || A < 1 || D < 1 || (long)A * D > kMergeCap) return 0;
    const size_t cap = (size_t)merge_cap((long)A * D), b = (size_t)B;
    size_t s = 0;
    s += b * cap * (16 + 4 + 4 + 4) + 1024;     // boxes, scores, cats, valid
    s += b * 4 + 256;                           // cnt
    s += b * cap * (cap / 64) * 8 + 256;        // mask
    s += b * cap * 4 + b * 4 + 512;             // keep, keep_count
    return s + 1024;
}

extern "C" int aldi_tta_merge(const float* boxes, const float* scores, const int* classes, const int* count, const aldi_box_tfm* tfm,
                              int B, int A, int D, int K, float score_floor, float nms_thresh, int topk, void* workspace,
                              float* out_boxes, float* out_scores, int* out_classes, int* out_count, aldi_stream_t stream) {
    if (!boxes || !scores || !classes || !count || !tfm || !workspace || !out_boxes || !out_scores || !out_classes || !out_count)
        return aldi_set_error_msg(ALDI_ERR_ARG, "tta_merge: null pointer");
    if (B < 1 || A < 1 || D < 1 || K < 1 || topk < 1) return aldi_set_error_msg(ALDI_ERR_ARG, "tta_merge: B, A, D, K and topk must be positive");
    if ((long)A * D > kMergeCap) return aldi_set_error_msg(ALDI_ERR_ARG, "tta_merge: A * D exceeds the 8192-candidate capacity");
    if ((long)B * topk > 0x7fffffffL / 4) return aldi_set_error_msg(ALDI_ERR_ARG, "tta_merge: B * topk too large");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int total = A * D;
    const size_t cap = (size_t)merge_cap(total), b = (size_t)B;
    int p2 = 1024;
    while (p2 < total) p2 <<= 1;
    char* w = static_cast<char*>(workspace);
    auto take = [&](size_t bytes) { char* p = w; w += (bytes + 255) / 256 * 256; return p; };
    auto* sboxes = (float4*)take(b * cap * 16);
    auto* sscores = (float*)take(b * cap * 4);
    auto* cats = (int*)take(b * cap * 4);
    auto* valid = (int*)take(b * cap * 4);
    auto* cnt = (int*)take(b * 4);
    auto* mask = (unsigned long long*)take(b * cap * (cap / 64) * 8);
    auto* keep = (int*)take(b * cap * 4);
    auto* keep_count = (int*)take(b * 4);
    MergeIn in = {boxes, scores, classes, count, tfm, A, D, K, score_floor};
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(merge_sort_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kMergeCap * 8 + 16);
    hipLaunchKernelGGL(merge_sort_kernel, dim3(B), dim3(1024), (size_t)p2 * 8 + 16, st, in, p2, (int)cap, sboxes, sscores, cats, valid, cnt);
    ALDI_CHECK_LAUNCH();
    nms_mask_launch(st, B, sboxes, valid, cats, cnt, (int)cap, nms_thresh, mask, aldi_tuning().nms_mask_tri);
    ALDI_CHECK_LAUNCH();
    if (!nms_scan_launch(st, B, mask, valid, cnt, (int)cap, topk, keep, keep_count)) return aldi_set_error_msg(ALDI_ERR_ARG, "tta_merge: NMS capacity too large");
    ALDI_CHECK_LAUNCH();
    hipLaunchKernelGGL(merge_finish_kernel, dim3(B), dim3(64), 0, st, sboxes, sscores, cats, keep, keep_count, (int)cap, topk,
                       out_boxes, out_scores, out_classes, out_count);
    ALDI_CHECK_LAUNCH();
    return ALDI_OK;
}
