// COCO box-AP evaluation on the device (aldi_amd/evaluation.py DeviceCOCOEvaluator; the host statement of the same
// algorithm is evaluate_img / accumulate in that file, a restatement of pycocotools' COCOeval for iouType="bbox").
//
// Everything is fp64 and every operation is the host's operation on the host's operands, in the host's order (+, -, *, /,
// min, max, compare, int -> double; no FMA contraction, -ffp-contract=off), so the results are EQUAL to the host's, not
// close to them (tests/test_eval_device_gpu.py).  Three kernels:
//   1. coco_postprocess_kernel: detector_postprocess + the XYXY -> XYWH step of the evaluator's `process`;
//   2. coco_match_kernel: evaluate_img for one (image, category) per wave -- a lane per (area range, IoU threshold) problem;
//   3. coco_accumulate_kernel: accumulate for one (category, area range, IoU threshold) per workgroup -- block-wide scans;
//      its Detail instantiation also counts what AR at the cuts 1 / 10 and precision / recall above a score cut are made of.
// The orderings between them (stable sorts, segment offsets) are torch plumbing on device tensors.
#include "common.h"
#include "sortscan.h"

namespace {

constexpr int kAreas = ALDI_COCO_AREAS, kThrs = ALDI_COCO_THRS, kRecs = ALDI_COCO_RECS;
constexpr int kProblems = kAreas * kThrs;            // 40 lanes of the wave carry a problem each
constexpr int kDetLds = 128;                         // detections of one (image, category) after the cut (maxDets = 100)
constexpr int kGtLds = 256;                          // ground-truth boxes staged in LDS; a longer list is read from global memory

// `process`: float32 XYXY in network pixels -> float64, times (width / iw, height / ih), clip to the original image, drop
// empty boxes (Boxes.nonempty), store XYWH.  meta[c] = {sx, sy, width, height} of the `process` entry the detection came in.
__global__ __launch_bounds__(256) void coco_postprocess_kernel(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                               const long* __restrict__ classes, const int* __restrict__ entry,
                                                               const double* __restrict__ meta, long n, int K, double* __restrict__ obox,
                                                               double* __restrict__ oscore, unsigned char* __restrict__ valid) {
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* m = meta + 4L * entry[i];
    const double sx = m[0], sy = m[1], w = m[2], h = m[3];
    double x1 = (double)boxes[4 * i] * sx, y1 = (double)boxes[4 * i + 1] * sy, x2 = (double)boxes[4 * i + 2] * sx, y2 = (double)boxes[4 * i + 3] * sy;
    // np.clip(v, 0, hi) = minimum(maximum(v, 0), hi)
    x1 = x1 > 0.0 ? x1 : 0.0; x1 = x1 < w ? x1 : w;
    x2 = x2 > 0.0 ? x2 : 0.0; x2 = x2 < w ? x2 : w;
    y1 = y1 > 0.0 ? y1 : 0.0; y1 = y1 < h ? y1 : h;
    y2 = y2 > 0.0 ? y2 : 0.0; y2 = y2 < h ? y2 : h;
    const long c = classes[i];
    obox[4 * i] = x1; obox[4 * i + 1] = y1; obox[4 * i + 2] = x2 - x1; obox[4 * i + 3] = y2 - y1;
    oscore[i] = (double)scores[i];
    valid[i] = (x2 > x1) && (y2 > y1) && c >= 0 && c < K;
}

// evaluate_img.  One wave per (image, category) segment; lane l < 40 owns the problem (area range l / 10, threshold l % 10) and
// walks the detections in score order, the ground truth in two passes (not ignored, then ignored: the stable "non-ignored
// first" order without materialising it -- the ignored pass runs only for a lane that found nothing in the first, which is
// the host's `break`).  The IoU of a (detection, ground truth) pair is wave-uniform; what differs per lane is the decision.
// Matched flags of ground truth g live in a register bit for g < 64 and in the lane's own byte ws[(g0 + g) * 64 + lane] beyond
// (zeroed by the entry point; a lane reads only what it wrote itself, so no ordering between lanes is needed).
__global__ __launch_bounds__(64) void coco_match_kernel(const double* __restrict__ dbox, const int* __restrict__ det_off, const double* __restrict__ gbox,
                                                        const double* __restrict__ garea, const unsigned char* __restrict__ gflags,
                                                        const int* __restrict__ gt_off, const double* __restrict__ area_rng,
                                                        const double* __restrict__ iou_thrs, unsigned char* __restrict__ ws, int max_det,
                                                        unsigned long long* __restrict__ mbits, unsigned long long* __restrict__ igbits,
                                                        int* __restrict__ num_gt) {
    __shared__ double s_d[kDetLds * 4];
    __shared__ double s_g[kGtLds * 4];
    __shared__ double s_ga[kGtLds];
    __shared__ unsigned char s_gf[kGtLds];
    const int seg = blockIdx.x, lane = threadIdx.x, prob = lane % kProblems;
    const int a = prob / kThrs, t = prob % kThrs;
    const int d0 = det_off[seg], g0 = gt_off[seg], G = gt_off[seg + 1] - g0;
    int D = det_off[seg + 1] - d0;
    D = D < max_det ? D : max_det;
    const double lo = area_rng[2 * a], hi = area_rng[2 * a + 1];
    if (D == 0 && G == 0) {
        if (lane < kAreas) num_gt[seg * kAreas + lane] = 0;
        return;
    }
    for (int i = lane; i < D * 4; i += 64) s_d[i] = dbox[4L * d0 + i];
    const bool g_lds = G <= kGtLds;
    if (g_lds) {
        for (int i = lane; i < G * 4; i += 64) s_g[i] = gbox[4L * g0 + i];
        for (int i = lane; i < G; i += 64) { s_ga[i] = garea[g0 + i]; s_gf[i] = gflags[g0 + i]; }
    }
    __syncthreads();
    const double* gb = g_lds ? s_g : gbox + 4L * g0;
    const double* ga = g_lds ? s_ga : garea + g0;
    const unsigned char* gf = g_lds ? s_gf : gflags + g0;

    int npig = 0;
    for (int g = 0; g < G; ++g) {
        const double ar = ga[g];
        npig += !((gf[g] & 3) || ar < lo || ar > hi);
    }
    if (lane < kProblems && t == 0) num_gt[seg * kAreas + a] = npig;

    double thr = iou_thrs[t];
    thr = thr < 1 - 1e-10 ? thr : 1 - 1e-10;
    unsigned long long taken = 0;                        // ground truth g < 64 already matched in this lane's problem
    unsigned char* wl = ws + (long)g0 * 64 + lane;
    for (int d = 0; d < D; ++d) {
        const double dx = s_d[4 * d], dy = s_d[4 * d + 1], dw = s_d[4 * d + 2], dh = s_d[4 * d + 3];
        const double dx2 = dx + dw, dy2 = dy + dh, da = dw * dh;
        double best = thr;
        int m = -1;
        bool m_ig = false;
        for (int part = 0; part < 2; ++part) {
            const bool search = part == 0 || m < 0;      // the ignored boxes are searched only without a regular match
            if (!__any(search)) break;
            for (int g = 0; g < G; ++g) {
                const double gx = gb[4 * g], gy = gb[4 * g + 1], gw = gb[4 * g + 2], gh = gb[4 * g + 3], ar = ga[g];
                const int f = gf[g];
                const bool crowd = f & 1;
                const bool ig = (f & 3) || ar < lo || ar > hi;
                const bool tk = g < 64 ? (taken >> g) & 1 : (bool)wl[(long)g * 64];
                // iou_xywh: right / bottom edges recomputed from XYWH; union against a crowd box is the detection's area
                const double gx2 = gx + gw, gy2 = gy + gh;
                double iw = (dx2 < gx2 ? dx2 : gx2) - (dx > gx ? dx : gx);
                double ih = (dy2 < gy2 ? dy2 : gy2) - (dy > gy ? dy : gy);
                iw = iw > 0.0 ? iw : 0.0;
                ih = ih > 0.0 ? ih : 0.0;
                const double inter = iw * ih;
                const double uni = crowd ? da : da + gw * gh - inter;
                const double iou = inter / uni;
                if (search && ig == (part == 1) && !(tk && !crowd) && !(iou < best)) {     // equal IoU: the later box wins
                    best = iou;
                    m = g;
                    m_ig = ig;
                }
            }
        }
        if (m >= 0) {
            if (m < 64) taken |= 1ull << m;
            else wl[(long)m * 64] = 1;
        }
        const bool dig = m >= 0 ? m_ig : (da < lo || da > hi);
        const unsigned long long mb = __ballot(m >= 0), ib = __ballot(dig);
        if (lane == 0) {
            mbits[d0 + d] = mb & ((1ull << kProblems) - 1);
            igbits[d0 + d] = ib & ((1ull << kProblems) - 1);
        }
    }
}

__device__ __forceinline__ int block_sum_int(int v, int* smem /* >= 16 ints */) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) smem[threadIdx.x >> 6] = v;
    __syncthreads();
    int r = 0;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) r += smem[i];
    return r;
}

// accumulate.  One workgroup per (category, area range, threshold).  perm[cat_off[c] .. cat_off[c + 1]) lists the kept detection
// slots of category c in the host's order (images in order, then a stable descending score sort).  tp / fp are block-wide
// prefix counts carried over 256-element chunks.  The host's envelope + searchsorted pair
//     q[r] = max(pr[i] for i >= first i with rc[i] >= R[r])      (rc is non-decreasing)
// is the maximum of pr over {i : rc[i] >= R[r]}: every element goes to the bucket b(i) = #{r : R[r] <= rc[i]} (a binary
// search), buckets keep their maximum, and q[r] is the maximum over the buckets above r -- maxima of the same doubles, so exact.
//
// Detail (aldi_coco_accumulate_detail; the host's recall_at_cut / counts_above of the same per-image results): the same walk
// also counts, per thread and in integers, the true positives whose rank inside their (image, category) segment is below 1
// and below 10 (COCOeval's [:, 0:maxDet] before the concatenation) and the true / false positives whose score is above tau.
// The four counts are summed over the block after the loop (block_sum_int) and leave as doubles: recall_at = count / npig,
// the expression of recall[b]; tp_thr / fp_thr / num_gt_out the counts themselves.  No atomics, no floating-point sums.
struct CocoDetail {
    const long* rank;             // [N] position of the slot inside its segment (the order coco_match_kernel walked)
    const double* scores;         // [N] the slot's score (a float32 value held as a double)
    double tau;                   // a detection is above the cut iff score > tau
    double* recall_at;            // [K][4][10][2]: cuts 1 and 10
    double* tp_thr;               // [K][4][10]
    double* fp_thr;               // [K][4][10]
    double* num_gt;               // [K][4]
};

template <bool Detail>
__global__ __launch_bounds__(256) void coco_accumulate_kernel(const long* __restrict__ perm, const int* __restrict__ cat_off,
                                                              const unsigned long long* __restrict__ mbits, const unsigned long long* __restrict__ igbits,
                                                              const int* __restrict__ num_gt, int I, int K, const double* __restrict__ rec_thrs,
                                                              double* __restrict__ precision, double* __restrict__ recall, int* __restrict__ valid,
                                                              CocoDetail dt) {
    __shared__ int s_scan[32];
    __shared__ double s_rec[kRecs];
    __shared__ unsigned long long s_seg[kRecs + 1];      // bit patterns of non-negative doubles order as integers
    const int b = blockIdx.x, t = b % kThrs, a = (b / kThrs) % kAreas, c = b / kProblems, bit = a * kThrs + t;
    const int tid = threadIdx.x;
    int part = 0;
    for (int i = tid; i < I; i += 256) part += num_gt[((long)i * K + c) * kAreas + a];
    const int npig_i = block_sum_int(part, s_scan);
    for (int i = tid; i < kRecs; i += 256) s_rec[i] = rec_thrs[i];
    for (int i = tid; i <= kRecs; i += 256) s_seg[i] = 0;
    double* prow = precision + (long)b * kRecs;
    if (npig_i == 0) {                                   // the host's None: no evaluated image or no regular ground truth
        for (int i = tid; i < kRecs; i += 256) prow[i] = 0.0;
        if (tid == 0) {
            recall[b] = 0.0;
            if (t == 0) valid[c * kAreas + a] = 0;
            if (Detail) {
                dt.recall_at[2L * b] = 0.0; dt.recall_at[2L * b + 1] = 0.0;
                dt.tp_thr[b] = 0.0; dt.fp_thr[b] = 0.0;
                if (t == 0) dt.num_gt[c * kAreas + a] = 0.0;
            }
        }
        return;
    }
    const double npig = (double)npig_i, eps = 2.220446049250313e-16;     // np.spacing(1)
    const int beg = cat_off[c], n = cat_off[c + 1] - beg;
    int ctp = 0, cfp = 0;
    int tp1 = 0, tp10 = 0, tpt = 0, fpt = 0;             // Detail: this thread's own counts
    for (int base = 0; base < n; base += 256) {
        const int i = base + tid;
        const bool in = i < n;
        bool m = false, g = false;
        long slot = 0;
        if (in) {
            slot = perm[beg + i];
            m = (mbits[slot] >> bit) & 1;
            g = (igbits[slot] >> bit) & 1;
        }
        const bool ftp = in && m && !g, ffp = in && !m && !g;
        if (Detail && in) {
            const long rk = dt.rank[slot];
            const bool above = dt.scores[slot] > dt.tau;
            tp1 += ftp && rk < 1;
            tp10 += ftp && rk < 10;
            tpt += ftp && above;
            fpt += ffp && above;
        }
        int ttp, tfp;
        const int rtp = block_rank(ftp, s_scan, &ttp), rfp = block_rank(ffp, s_scan, &tfp);
        if (in) {
            const double tp = (double)(ctp + rtp + (int)ftp), fp = (double)(cfp + rfp + (int)ffp);
            const double rc = tp / npig, pr = tp / (fp + tp + eps);
            int lo = 0, hi = kRecs;                      // lo = #{r : R[r] <= rc}
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (s_rec[mid] <= rc) lo = mid + 1; else hi = mid;
            }
            atomicMax(&s_seg[lo], (unsigned long long)__double_as_longlong(pr));
        }
        ctp += ttp;
        cfp += tfp;
    }
    __syncthreads();
    for (int r = tid; r < kRecs; r += 256) {
        unsigned long long q = 0;
        for (int k = r + 1; k <= kRecs; ++k) q = s_seg[k] > q ? s_seg[k] : q;
        prow[r] = __longlong_as_double((long long)q);
    }
    if (tid == 0) {
        recall[b] = n ? (double)ctp / npig : 0.0;
        if (t == 0) valid[c * kAreas + a] = 1;
    }
    if (Detail) {
        tp1 = block_sum_int(tp1, s_scan);
        tp10 = block_sum_int(tp10, s_scan);
        tpt = block_sum_int(tpt, s_scan);
        fpt = block_sum_int(fpt, s_scan);
        if (tid == 0) {
            dt.recall_at[2L * b] = n ? (double)tp1 / npig : 0.0;
            dt.recall_at[2L * b + 1] = n ? (double)tp10 / npig : 0.0;
            dt.tp_thr[b] = (double)tpt;
            dt.fp_thr[b] = (double)fpt;
            if (t == 0) dt.num_gt[c * kAreas + a] = npig;
        }
    }
}

}  // namespace

extern "C" int aldi_coco_postprocess(const float* boxes, const float* scores, const long* classes, const int* entry, const double* meta, long n,
                                     int num_classes, double* out_boxes, double* out_scores, unsigned char* out_valid, aldi_stream_t stream) {
    if (n < 0 || num_classes <= 0) return aldi_set_error_msg(ALDI_ERR_ARG, "coco_postprocess: bad sizes");
    if (n == 0) return ALDI_OK;
    if (!boxes || !scores || !classes || !entry || !meta || !out_boxes || !out_scores || !out_valid)
        return aldi_set_error_msg(ALDI_ERR_ARG, "coco_postprocess: null pointer");
    hipLaunchKernelGGL(coco_postprocess_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), boxes, scores, classes,
                       entry, meta, n, num_classes, out_boxes, out_scores, out_valid);
    ALDI_CHECK_LAUNCH();
    return ALDI_OK;
}

extern "C" size_t aldi_coco_match_workspace(long num_gt) { return (size_t)(num_gt > 0 ? num_gt : 0) * 64 + 64; }

extern "C" int aldi_coco_match(const double* det_boxes, const int* det_off, const double* gt_boxes, const double* gt_area, const unsigned char* gt_flags,
                               const int* gt_off, int num_segments, long num_gt, const double* area_rng, const double* iou_thrs, int max_det,
                               void* workspace, unsigned long long* matched, unsigned long long* dt_ignore, int* num_gt_out, aldi_stream_t stream) {
    if (num_segments <= 0 || num_gt < 0 || max_det <= 0 || max_det > kDetLds) return aldi_set_error_msg(ALDI_ERR_ARG, "coco_match: bad sizes (max_det <= 128)");
    if (!det_boxes || !det_off || !gt_boxes || !gt_area || !gt_flags || !gt_off || !area_rng || !iou_thrs || !workspace || !matched || !dt_ignore || !num_gt_out)
        return aldi_set_error_msg(ALDI_ERR_ARG, "coco_match: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemsetAsync(workspace, 0, aldi_coco_match_workspace(num_gt), st);
    if (e != hipSuccess) return aldi_set_error(e, __FILE__, __LINE__);
    hipLaunchKernelGGL(coco_match_kernel, dim3((unsigned)num_segments), dim3(64), 0, st, det_boxes, det_off, gt_boxes, gt_area, gt_flags, gt_off, area_rng,
                       iou_thrs, static_cast<unsigned char*>(workspace), max_det, matched, dt_ignore, num_gt_out);
    ALDI_CHECK_LAUNCH();
    return ALDI_OK;
}

extern "C" int aldi_coco_accumulate(const long* perm, const int* cat_off, const unsigned long long* matched, const unsigned long long* dt_ignore,
                                    const int* num_gt, int num_images, int num_classes, const double* rec_thrs, double* precision, double* recall,
                                    int* valid, aldi_stream_t stream) {
    if (num_images <= 0 || num_classes <= 0) return aldi_set_error_msg(ALDI_ERR_ARG, "coco_accumulate: bad sizes");
    if (!perm || !cat_off || !matched || !dt_ignore || !num_gt || !rec_thrs || !precision || !recall || !valid)
        return aldi_set_error_msg(ALDI_ERR_ARG, "coco_accumulate: null pointer");
    hipLaunchKernelGGL(coco_accumulate_kernel<false>, dim3((unsigned)(num_classes * kProblems)), dim3(256), 0, static_cast<hipStream_t>(stream), perm,
                       cat_off, matched, dt_ignore, num_gt, num_images, num_classes, rec_thrs, precision, recall, valid, CocoDetail{});
    ALDI_CHECK_LAUNCH();
    return ALDI_OK;
}

extern "C" int aldi_coco_accumulate_detail(const long* perm, const int* cat_off, const unsigned long long* matched, const unsigned long long* dt_ignore,
                                           const int* num_gt, const long* rank, const double* scores, int num_images, int num_classes,
                                           const double* rec_thrs, double tau, double* precision, double* recall, int* valid, double* recall_at,
                                           double* tp_thr, double* fp_thr, double* num_gt_out, aldi_stream_t stream) {
    if (num_images <= 0 || num_classes <= 0) return aldi_set_error_msg(ALDI_ERR_ARG, "coco_accumulate_detail: bad sizes");
    if (tau != tau) return aldi_set_error_msg(ALDI_ERR_ARG, "coco_accumulate_detail: tau is NaN");
    if (!perm || !cat_off || !matched || !dt_ignore || !num_gt || !rank || !scores || !rec_thrs || !precision || !recall || !valid || !recall_at ||
        !tp_thr || !fp_thr || !num_gt_out)
        return aldi_set_error_msg(ALDI_ERR_ARG, "coco_accumulate_detail: null pointer");
    const CocoDetail dt{rank, scores, tau, recall_at, tp_thr, fp_thr, num_gt_out};
    hipLaunchKernelGGL(coco_accumulate_kernel<true>, dim3((unsigned)(num_classes * kProblems)), dim3(256), 0, static_cast<hipStream_t>(stream), perm,
                       cat_off, matched, dt_ignore, num_gt, num_images, num_classes, rec_thrs, precision, recall, valid, dt);
    ALDI_CHECK_LAUNCH();
    return ALDI_OK;
}
