// Which kernel a convolution gets: the host-only half of igemm.hip (no HIP types, no device code; compiles with a plain C++ compiler).
//
//   plan_conv / plan_conv_group   argument checks + select_tile: what aldi_conv_igemm, aldi_conv_igemm_group and aldi_conv_igemm_plan share
//   select_tile                   (shape, operands, knobs) -> Choice: a row of IGEMM_TILES plus the run-time modifiers
//   dispatch_name                 Choice -> the string aldi_last_dispatch() reports
//
// igemm.hip turns a Choice into a launch with a switch generated from the same IGEMM_TILES list.
#pragma once
#include "host.h"
#include <stdio.h>

namespace {

struct ConvDev {
    const void* x; const void* w; void* y; float* y_f32;
    const float* scale; const float* shift; const void* res; const void* mask;
    int N, H, W, Cin, Cout, KH, KW, stride, pad, Ho, Wo;
    int relu, res_mode, out_scale, OH, OW;
    int M, K, xcd, dbg;
    unsigned x_bytes, w_bytes;
    int ksplit, slabs_per_split;     // split-K (plain 1x1 / linear): blockIdx.z = slice, slabs_per_split K slabs each
    int lean;                        // unused (kept for the kernels' argument layout): the lean K loop is Choice::lean and the LEAN template argument
    // ReLU masks as BITS (bf16, Cout % 8 == 0, plain output layout): [M][Cout / 8] bytes, bit c % 8 of byte c / 8 = (y[m][c] > 0).
    // bits_out: written by the forward launch beside y; mask_bits: read by the backward launch instead of the 16x larger `mask` tensor.
    const unsigned char* mask_bits; unsigned char* bits_out;
};

// Several problems of ONE layer shape in one launch -- the student's and the teacher's pass through the same layer (different
// weights, different images), and the same kind of layer on the maps of several pyramid levels (the four FPN output convs, the
// RPN conv on p2..p6: same channels and taps, different H x W): the launches' fixed costs (ramp-up, partial last wave of tiles,
// dependent-launch gap: ~10 us per 3x3 layer at these sizes) are paid once, and the small problems' tiles fill the large one's tail.
constexpr int kMaxConvGroup = 12;
struct ConvGroup {
    int n;
    int wg_begin[kMaxConvGroup + 1];          // first workgroup of each problem (multiples of 8: the XCD-aware tile order assumes it)
    int nmt[kMaxConvGroup], nnt[kMaxConvGroup];
    ConvDev p[kMaxConvGroup];
};

// ---- the tile variants: one row per kernel instantiation igemm.hip launches.
//   X(id, element type, form, BM, BN, WM, WN, KC, PIPE, EPI)
// form: TAP (one K slab per tap and channel chunk), HALO (3x3 / stride 1 / pad 1: one pixel slab per three taps), ROLES (that, with the two wave
// halves in alternating roles), HALO64 (igemm_halo64.h), WS (igemm_ws.h: BM x BN per step, K = 8 * KC).  KC: 16-byte chunks per K-slab row
// (4 = 64-byte slabs, 8 = 128-byte).  PIPE: the software-pipelined K loop ("pipe") or the flat one.  EPI: 0 staged epilogue, 1 direct, 2 direct
// with the residual prefetch.  Run-time modifiers (Choice): the lean K loop of the direct tap tiles, HALO64's direct epilogue and interleaved loop.
#define IGEMM_TILES(X) \
    X(BF16_TAP_128x16,       bf16_t, TAP,    128, 16,  4, 1, 4, 1, 0) X(F32_TAP_128x16,   float, TAP,  128, 16,  4, 1, 4, 1, 0) \
    X(BF16_TAP_128x128,      bf16_t, TAP,    128, 128, 2, 2, 4, 1, 0) X(F32_TAP_128x128,  float, TAP,  128, 128, 2, 2, 4, 1, 0) \
    X(BF16_TAP_128x64,       bf16_t, TAP,    128, 64,  4, 1, 4, 1, 0) X(F32_TAP_128x64,   float, TAP,  128, 64,  4, 1, 4, 1, 0) \
    X(BF16_TAP_64x64,        bf16_t, TAP,    64,  64,  2, 2, 4, 1, 0) X(F32_TAP_64x64,    float, TAP,  64,  64,  2, 2, 4, 1, 0) \
    X(BF16_TAP_256x128,      bf16_t, TAP,    256, 128, 4, 2, 4, 0, 0) X(F32_TAP_256x128,  float, TAP,  256, 128, 4, 2, 4, 0, 0) \
    X(BF16_HALO_128x128,     bf16_t, HALO,   128, 128, 2, 2, 4, 0, 0) X(F32_HALO_128x128, float, HALO, 128, 128, 2, 2, 4, 0, 0) \
    X(BF16_HALO_128x64,      bf16_t, HALO,   128, 64,  4, 1, 4, 0, 0) X(F32_HALO_128x64,  float, HALO, 128, 64,  4, 1, 4, 0, 0) \
    X(BF16_HALO_256x128,     bf16_t, HALO,   256, 128, 4, 2, 4, 0, 0) X(F32_HALO_256x128, float, HALO, 256, 128, 4, 2, 4, 0, 0) \
    X(BF16_HALO_128x64_D,    bf16_t, HALO,   128, 64,  4, 1, 4, 0, 1) \
    X(BF16_HALO_96x64,       bf16_t, HALO,   96,  64,  3, 1, 4, 0, 0) X(BF16_HALO_96x64_D, bf16_t, HALO, 96, 64, 3, 1, 4, 0, 1) \
    X(BF16_HALO_64x64,       bf16_t, HALO,   64,  64,  2, 2, 4, 0, 0) X(BF16_HALO_64x64_D, bf16_t, HALO, 64, 64, 2, 2, 4, 0, 1) \
    X(BF16_HALO_240x128,     bf16_t, HALO,   240, 128, 3, 2, 4, 0, 0) \
    X(BF16_ROLES_256x128,    bf16_t, ROLES,  256, 128, 4, 2, 4, 0, 0) \
    X(BF16_HALO64_256x256,   bf16_t, HALO64, 256, 256, 4, 2, 8, 0, 0) \
    X(BF16_HALO64_128x128,   bf16_t, HALO64, 128, 128, 2, 2, 8, 0, 0) \
    X(BF16_HALO64_256x256_W4, bf16_t, HALO64, 256, 256, 2, 2, 8, 0, 0) \
    X(BF16_TAP_128x64_D,     bf16_t, TAP,    128, 64,  4, 1, 4, 1, 1) X(BF16_TAP_128x64_DR, bf16_t, TAP, 128, 64, 4, 1, 4, 1, 2) \
    X(BF16_TAP_128x128_K64,  bf16_t, TAP,    128, 128, 2, 2, 8, 0, 0) \
    X(BF16_TAP_128x64_K64,   bf16_t, TAP,    128, 64,  4, 1, 8, 0, 0) X(BF16_TAP_128x64_K64_D, bf16_t, TAP, 128, 64, 4, 1, 8, 0, 1) \
    X(BF16_TAP_64x64_K64,    bf16_t, TAP,    64,  64,  2, 2, 8, 0, 0) X(BF16_TAP_64x64_K64_D, bf16_t, TAP, 64, 64, 2, 2, 8, 0, 1) \
    X(BF16_TAP_256x128_K64,  bf16_t, TAP,    256, 128, 4, 2, 8, 0, 0) \
    X(BF16_WS_K64,           bf16_t, WS,     32,  256, 1, 4, 8, 0, 1) X(BF16_WS_K128,     bf16_t, WS,  32,  256, 1, 4, 16, 0, 1) \
    X(BF16_WS_K256,          bf16_t, WS,     32,  128, 1, 4, 32, 0, 1) X(BF16_WS_K512,    bf16_t, WS,  16,  128, 1, 4, 64, 0, 1)

enum TileForm { TAP, HALO, ROLES, HALO64, WS };
enum TileId {
#define IGEMM_TILE_ID(id, T, form, BM, BN, WM, WN, KC, PIPE, EPI) id,
    IGEMM_TILES(IGEMM_TILE_ID)
#undef IGEMM_TILE_ID
    kNumTiles
};
struct TileRow { const char* id; bool f32; TileForm form; int BM, BN, WM, WN, KC; bool pipe; int epi; };
constexpr TileRow kTiles[kNumTiles] = {
#define IGEMM_TILE_ROW(id, T, form, BM, BN, WM, WN, KC, PIPE, EPI) {#id, sizeof(T) == 4, form, BM, BN, WM, WN, KC, PIPE != 0, EPI},
    IGEMM_TILES(IGEMM_TILE_ROW)
#undef IGEMM_TILE_ROW
};

// a tile plus the run-time modifiers that are part of the decision
struct Choice {
    TileId tile;
    bool lean;            // direct-epilogue tap tiles: the lean K loop (igemm_lean)
    bool direct, ilv;     // HALO64: the direct epilogue (igemm_direct bit 8); the interleaved K loop of the 8-wave 256 x 256 tile (igemm_halo_ilv)
    int ksplit;           // > 1: a split-K launch (the slices; the caller adds the finalize pass)
    int ws_wgs;           // WS: workgroup count (igemm_ws_wgs)
    int group_n;          // > 0: one launch over the problems of a group
};

// ---- predicates
// igemm_ws.h takes: bf16, 1x1 / stride 1 / no padding, plain output layout, K = Cin in {64, 128, 256, 512}, whole channel groups, no full-tensor mask / fp32
// output / split-K
inline int ws_channels(int K) { return K == 64 || K == 128 ? 256 : K == 256 || K == 512 ? 128 : 0; }      // BN of the instantiation for this K
inline bool ws_ok(const ConvDev& d) {
    const int bn = ws_channels(d.K);
    return d.KH * d.KW == 1 && d.stride == 1 && d.pad == 0 && d.K == d.Cin && bn && d.Cout % bn == 0 && d.y && !d.y_f32 && !d.mask && d.out_scale == 1 &&
           d.ksplit <= 1 && (long)d.M * d.Cout * 2 < (1L << 31);
}
// the 128-byte-slab halo kernel (igemm_halo64.h), alone or over the problems of a group; the direct epilogue (igemm_direct bit 8) when every
// problem's output is plain bf16 with at most scale / shift / ReLU
inline bool halo64_direct_ok(const ConvDev& d) {
    return d.y && !d.y_f32 && d.out_scale == 1 && (d.Cout & 7) == 0 && !d.mask && !d.mask_bits && !d.bits_out && !d.res_mode;
}
inline bool plain_1x1(const ConvDev& d) { return d.KH * d.KW == 1 && d.stride == 1 && d.pad == 0; }

// Tile selection.  Every arm is reachable from a test through aldi_set_tuning("igemm_force", ...) and named by
// aldi_last_dispatch(); the thresholds are knobs of the same table (include/aldi_hip.h).
// d: the problem (a group: its largest problem with the COMBINED pixel count in M; group: its group_n problems).  Pure: reads its arguments only.
inline Choice select_tile(const ConvDev& d, const AldiTuning& tn, const bool f32, const int group_n, const ConvDev* group = nullptr) {
    Choice c = {BF16_TAP_128x128, false, false, false, d.ksplit > 1 ? d.ksplit : 0, tn.igemm_ws_wgs, group_n};
    const auto pick = [&](TileId bf16_id, TileId f32_id) {
        c.tile = f32 ? f32_id : bf16_id;
        const TileRow& r = kTiles[c.tile];
        // the lean K loop: plain 1x1 / linear layers with whole K slabs, on the direct-epilogue tap tiles
        c.lean = r.form == TAP && r.epi != 0 && tn.igemm_lean && plain_1x1(d) && d.K % 64 == 0 && !(tn.igemm_dbg & (8 | 16));
        if (r.form == HALO64) {
            c.direct = (tn.igemm_direct & 8) != 0;
            for (int i = 0; i < (group_n ? group_n : 1); ++i) c.direct = c.direct && halo64_direct_ok(group_n ? group[i] : d);
            // igemm_halo_ilv: the interleaved K loop (reads / DMA pieces between the MFMAs of a sub-phase; igemm_halo64.h) -- the 8-wave 256 x 256 tile
            c.ilv = c.tile == BF16_HALO64_256x256 && tn.igemm_halo_ilv != 0;
        }
        return c;
    };
#define BOTH(name) pick(BF16_##name, F32_##name)
#define BF16(name) pick(BF16_##name, BF16_##name)
    const bool bf16 = !f32;
    if (d.ksplit > 1) {
        // split-K (bf16 plain 1x1 / linear; the fp32 slices of every K range)
        // igemm_splitk_tile: 0 = 128x128 tiles with 128-byte K slabs (4 waves); 1 = 256x128 tiles, 64-byte slabs (8 waves: two per SIMD
        // also when the launch is one workgroup per CU: FC1 at 2048 rows 86 -> 72 us, at 2000 rows 94 -> 72 us, tools/fc1_splitk_sweep.py)
        const int tile_knob = tn.igemm_splitk_tile;       // 2 (default): 256x128 (128-byte slabs) when its launch still has ~one workgroup per CU; 4: the same rule with 64-byte slabs
        const bool big_ok = (long)cdiv(d.M, 256) * cdiv(d.Cout, 128) * d.ksplit >= 200;
        // 256x128 tiles with 128-byte K slabs (full cache lines per DMA lane group, half the barriers per MFMA of the 64-byte form: FC1 at 2048
        // rows 94 -> 79 us on cold weights, tools/fc1_cold.py)
        if (tile_knob == 3 || (tile_knob == 2 && big_ok)) return BF16(TAP_256x128_K64);
        if (tile_knob == 1 || (tile_knob == 4 && big_ok)) return BF16(TAP_256x128);
        return BF16(TAP_128x128_K64);
    }
    // the N=2 micro-batch leaves the deep layers (res4/res5, FC heads) with far fewer 128x128 tiles than the
    // 256 CUs: fall back to 64x64 tiles (4x the workgroups) when the big tiling cannot fill the chip
    const long big = (long)cdiv(d.M, 128) * cdiv(d.Cout, 128);
    // igemm_bigtile_min: long-K convs with thousands of tiles are bound by the L2 -> CU path (~31 B/clk/CU measured): the
    // 256x128 tile (8 waves) moves 25 % fewer bytes per flop.
    // igemm_bigtile_k / igemm_lintile_min: plain token GEMMs (ViT / ConvNeXt linears: K >= 768, M in the thousands): the
    // 256x128 tile already pays from ~770 tiles on (+10 % at K = 768, +30 % at K = 3072 measured); the short-K 1x1 convs of
    // the R50 trunk are HBM-bound and stay on 128x128.
    // igemm_halo: 3x3 / stride 1 / pad 1 (every 3x3 of the network): halo form, the pixel tile is loaded once per three taps.
    const int force = tn.igemm_force;     // 0 = heuristics; 1 = 128x128, 2 = 128x64, 3 = 64x64, 4 = 256x128, 5 = 128x16
    // igemm_direct (bit mask: 1 = the 128x64 1x1 / tap tile, 2 = the 64x64 long-K tile, 4 = the 128x64 halo tile): the direct epilogue of
    // the 64-channel tiles (igemm_epilogue_direct) for bf16 outputs in the plain layout; a residual needs the tile that prefetches it.
    // (No group and no split-K: the direct tiles have neither form.)
    const bool direct_ok = bf16 && !group_n && d.y && !d.y_f32 && d.out_scale == 1 && (d.Cout & 7) == 0 && !d.mask && d.ksplit <= 1 &&
                           !(d.mask_bits && (d.scale || d.shift)) && d.Cout >= 64 &&
                           !(d.mask_bits && (d.Cout & 31));        // (the mask bits arrive by a 4-byte LDS-DMA at bit offset (m * Cout + ch): dword-aligned for Cout % 32 == 0 only)
    const int direct = direct_ok ? tn.igemm_direct : 0;
    {
        // (fp32 -- the parity mode and the Deformable-DETR step's trunk: the halo form is the same code, 16 channels per group; igemm_halo_f32)
        const bool same3 = d.KH == 3 && d.KW == 3 && d.stride == 1 && d.pad == 1 && d.Ho == d.H && d.Wo == d.W && d.Cin % 32 == 0 && d.out_scale == 1;
        // fp32: OFF by default (igemm_halo_f32 = 0).  From ~400 half-width tiles on the halo form is faster alone (tools/halo_f32_sweep.py:
        // 33 600 px x 256 -> 256 324 -> 228 us, 33 600 x 128 -> 128 162 -> 115; below, the 64 x 64 tap form's four-fold workgroup count wins:
        // 8400 x 256 -> 256 148 vs 158, 2100 x 2048 -> 256 488 vs 647), but it sums K in another order (kh, channels, kw) than the tap form, so
        // a layer would round differently at N = 2 and at N = 6 -- the parity mode's fused-vs-sequential comparison flips discrete decisions --
        // and the Deformable-DETR step (N = 2 maps, few eligible layers) did not move (138 vs 140 ms)
        const bool f32_halo = f32 && tn.igemm_halo_f32 > 0 && (long)cdiv(d.M, 128) * cdiv(d.Cout, 64) >= tn.igemm_halo_f32;
        if (tn.igemm_halo && (bf16 || f32_halo) && same3) {
            if (force == 1) return BOTH(HALO_128x128);
            if (bf16 && force == 2 && (direct & 4) && !d.res_mode) return BF16(HALO_128x64_D);
            if (force == 2) return BOTH(HALO_128x64);
            if (force == 4) return BOTH(HALO_256x128);
            if (bf16) {
                // 64 x 64 halo tiles (4 waves of 32 x 32): four times the workgroups of the 128 x 128 count -- for the layers whose 128 x 64 tile count sits just
                // above a multiple of the 256 CUs (tools/quant_probe.py: 508 -> 516 workgroups = +23 % time)
                // 96 x 64 halo tiles on THREE waves (32 x 64 per wave, as in the 128 x 64 tile): 4/3 of its workgroups -- tools/quant_probe.py: a CU runs three
                // 128 x 64 workgroups in 1.23 x the time of two, and the mid-size layers of this network give it 2.06 (528 tiles) or 1.03 (264)
                if (force == 17 && (direct & 4) && !d.res_mode) return BF16(HALO_96x64_D);
                if (force == 17) return BF16(HALO_96x64);
                if (force == 16 && (direct & 4) && !d.res_mode) return BF16(HALO_64x64_D);
                if (force == 16) return BF16(HALO_64x64);
                if (force == 9) return BF16(HALO_240x128);
                if (force == 10 && !group_n) return BF16(ROLES_256x128);
                if (force == 11 && d.Cin % 64 == 0) return BF16(HALO64_256x256);
                if (force == 13 && d.Cin % 64 == 0) return BF16(HALO64_128x128);
                if (force == 15 && d.Cin % 64 == 0) return BF16(HALO64_256x256_W4);
            }
            if (force == 0 || force == 3) {      // (no 64x64 halo form; 5 = the 128x16 tap form)
                if (d.Cout <= 64) return BOTH(HALO_128x64);
                if (big >= tn.igemm_bigtile_min) {
                    // igemm_bigtile 64: 128-byte K slabs on a 256 x 256 tile (igemm_halo64.h) where the channels fill it
                    if (bf16 && tn.igemm_bigtile == 64 && d.Cin % 64 == 0 && d.Cout % 256 == 0) return BF16(HALO64_256x256);
                    if (bf16 && tn.igemm_bigtile == 65 && d.Cin % 64 == 0 && d.Cout % 256 == 0) return BF16(HALO64_256x256_W4);
                    if (tn.igemm_bigtile == 1) return BOTH(HALO_128x128);
                    if (bf16 && tn.igemm_bigtile == 10 && !group_n) return BF16(ROLES_256x128);
                    return BOTH(HALO_256x128);
                }
                // igemm_halo64_mid: mid-size layers with at least this many 128 x 128 tiles (two workgroups per CU: res3 / res4 conv2 at N = 4,
                // res3 at N = 2) take that tile with 128-byte K slabs (igemm_halo64.h); 0 = never
                if (bf16 && tn.igemm_halo64_mid > 0 && big >= tn.igemm_halo64_mid && d.Cin % 64 == 0 && d.Cout % 128 == 0) return BF16(HALO64_128x128);
                // below ~1000 128x128 tiles the tile count of this network sits just above a multiple of the 256 CUs (16800 pixels =
                // 131.25 row tiles: 264 / 528 tiles) and the last partial round costs as much as a full one; half-width tiles halve that
                // tail (measured 8-25 % faster on every res3..res5 / FPN p3..p6 3x3 at N = 2 and 4)
                // igemm_halo_small: long-K layers that do not even give every CU one or two 128 x 64 tiles (res5 conv2: 264 tiles at N = 4, 136 at N = 2)
                // take 64 x 64 tiles -- four waves of 32 x 32, four times the workgroups per pixel: 32.9 -> 30.4 / 27.7 -> 24.3 us, bit-identical (same K order;
                // tools/quant_probe.py, profiles/r06_quant_probe.txt).  At res4's K (16 800 px: 528 tiles) and res3's the larger tile wins (31.6 vs 38.3 us).
                // OFF by default (0; 320 selects res5 conv2): in the step, beside the other stream's workgroups, it measured 0.5 % slower (8.07 vs 8.02 ms).
                // igemm_halo96: layers with 200 .. 600 tiles of 128 x 64 (one or two per CU and a few left over: res4 conv2 at both batch sizes, res5 / res3 conv2
                // at one of them) on 96 x 64 three-wave tiles: 2-6 % faster alone, bit-identical (profiles/r06_quant_probe.txt)
                const long t64 = (long)cdiv(d.M, 128) * cdiv(d.Cout, 64);
                if (bf16 && tn.igemm_halo96 > 0 && t64 >= 200 && t64 <= 600) {
                    if ((direct & 4) && !d.res_mode) return BF16(HALO_96x64_D);
                    return BF16(HALO_96x64);
                }
                if (bf16 && tn.igemm_halo_small > 0 && t64 <= tn.igemm_halo_small && d.Cin >= 512) {
                    if ((direct & 4) && !d.res_mode) return BF16(HALO_64x64_D);
                    return BF16(HALO_64x64);
                }
                if (bf16 && (direct & 4) && !d.res_mode) return BF16(HALO_128x64_D);
                return BOTH(HALO_128x64);
            }
        }
    }
    // igemm_ws: the short-K 1x1 layers of the trunk (bottleneck expansions / reductions, their data gradients) on the weight-stationary persistent
    // kernel (igemm_ws.h; its epilogue is the direct one: igemm_direct bit 1 turns it off with that); igemm_force 14 forces it wherever it is eligible.
    // With an upsampled residual (FPN laterals) from 4 x igemm_ws_min pixels: p2's lateral 115 -> 107 us, p3's 39.7 -> 41.0 (tools/ws_ab.py)
    if (bf16 && !group_n && ws_ok(d) && (force == 14 || (force == 0 && tn.igemm_ws && (tn.igemm_direct & 1) && d.M >= (d.res_mode == 2 ? 4L : 1L) * tn.igemm_ws_min)))
        return d.K == 64 ? BF16(WS_K64) : d.K == 128 ? BF16(WS_K128) : d.K == 256 ? BF16(WS_K256) : BF16(WS_K512);
    if (force == 5 || (force == 0 && d.Cout <= 16)) return BOTH(TAP_128x16);
    if (force == 1) return BOTH(TAP_128x128);
    if (bf16 && force == 2 && (direct & 1)) return d.res_mode ? BF16(TAP_128x64_DR) : BF16(TAP_128x64_D);
    if (force == 2) return BOTH(TAP_128x64);
    if (force == 3) return BOTH(TAP_64x64);
    if (force == 4) return BOTH(TAP_256x128);
    if (bf16) {
        // 128-byte K slabs (64 channels: a full cache line per pixel row and k-step, half the barriers): plain 1x1 / linear
        // layers only (a ragged K tail is handled for those).  igemm_k64_min: long-K layers (res4/res5 reductions, their dgrads,
        // the box head's FCs) run 10-18 % faster on the 64x64 form than on any 32-channel tile (tools/igemm_sweep.py);
        // short-K layers (4 slabs) lose more to the shallower pipeline than they gain.
        const bool plain = plain_1x1(d);
        if (plain && force == 6) return BF16(TAP_128x128_K64);
        if (plain && force == 7) return BF16(TAP_128x64_K64);
        if (plain && force == 12 && (direct & 1) && !d.res_mode && d.K % 64 == 0) return BF16(TAP_128x64_K64_D);
        const bool lin256 = tn.igemm_tile != 9 && big >= tn.igemm_lintile_min && d.K >= tn.igemm_bigtile_k;     // (the token-GEMM rule below wins)
        if (plain && (force == 8 || (force == 0 && !lin256 && d.Cout > 64 && d.K % 64 == 0 && d.K >= tn.igemm_k64_min))) {
            if ((direct & 2) && !d.res_mode) return BF16(TAP_64x64_K64_D);
            return BF16(TAP_64x64_K64);
        }
    }
    // fp32 (the parity mode; the Deformable-DETR step's arithmetic): the f32-input MFMA runs at 1/16 of the bf16 rate, so a tile's K loop is
    // long and what pays is workgroups, not bytes per flop -- 64 x 64 tiles are as fast or faster than every larger tile on all of that
    // step's shapes (tools/f32_tile_sweep.py: 33 600 px x 128 -> 128 3x3 161 -> 110 us, 16 800 x 512 -> 128 77 -> 52, 44 646 x 256 -> 384
    // 100 -> 85, 44 646 x 1024 -> 256 205 -> 201); same K order per output element as the other tap-form tiles (bit-identical results)
    if (f32 && force == 0 && big < tn.igemm_f32_tile64_max) return BOTH(TAP_64x64);
    if (d.Cout <= 64) return BOTH(TAP_128x64);
    if (tn.igemm_tile != 9 && big >= tn.igemm_lintile_min && d.K >= tn.igemm_bigtile_k) {
        // 128-byte K slabs on this tile for plain bf16 layers with K % 64 == 0 (+8-17 % on the box head's FC1 dgrad and the ViT linears,
        // tools/lin_tile_ab.py; igemm_tile 7: the 64-byte slabs)
        if (bf16 && tn.igemm_tile != 7 && plain_1x1(d) && d.K % 64 == 0) return BF16(TAP_256x128_K64);
        return BOTH(TAP_256x128);
    }
    if (big < 200) return BOTH(TAP_64x64);
    // short-K layers (the bottlenecks' 1x1 expansions and res3's reductions: K = 128 .. 512, 4-16 slabs) are all prologue and
    // epilogue: half-width tiles (twice the workgroups, half the staging epilogue each) run them 8-13 % faster than 128x128
    // (tools/fc_dgrad_sweep.py: 16800 x 256 -> 1024: 25 -> 23 us, 67200 x 128 -> 512: 31 -> 27 us, 67200 x 512 -> 128: 26 -> 24 us)
    if (bf16 && d.K <= tn.igemm_narrow_k && (direct & 1)) return d.res_mode ? BF16(TAP_128x64_DR) : BF16(TAP_128x64_D);
    if (bf16 && d.K <= tn.igemm_narrow_k) return BOTH(TAP_128x64);
    return BOTH(TAP_128x128);
#undef BOTH
#undef BF16
}

// the name aldi_last_dispatch() reports, derived from the tile's row; -> its length
inline int dispatch_name(const Choice& c, char* name, int cap) {
    const TileRow& r = kTiles[c.tile];
    const char* elem = r.f32 ? "f32" : "bf16";
    const char* grp = c.group_n ? "_group" : "";           // "igemm_group<n><...": %.0d prints nothing for 0
    switch (r.form) {
    case WS: return snprintf(name, cap, "igemm_ws<%s,%d,%d,k%d>", elem, r.BM, r.BN, r.KC * 8);
    case HALO64:
        return snprintf(name, cap, "igemm%s%.0d<%s,%d,%d,%d,%d,halo64%s%s>", grp, c.group_n, elem, r.BM, r.BN, r.WM, r.WN, c.direct ? ",direct" : "",
                        (c.tile == BF16_HALO64_256x256 && !c.ilv) ? ",lockstep" : "");
    case ROLES: return snprintf(name, cap, "igemm<%s,%d,%d,%d,%d,roles,halo>", elem, r.BM, r.BN, r.WM, r.WN);
    default:
        return snprintf(name, cap, "igemm%s%.0d<%s,%d,%d,%d,%d,%s,%s%s%s>%s", grp, c.group_n, elem, r.BM, r.BN, r.WM, r.WN, r.pipe ? "pipe" : "flat", r.form == HALO ? "halo" : "tap",
                        r.KC == 8 ? ",k64" : "", r.epi == 2 ? ",direct+res" : r.epi == 1 ? ",direct" : "", c.ksplit > 1 ? " splitk" : "");
    }
}

// ---- argument checks: aldi_conv_args -> ConvDev
inline int fill_convdev(const aldi_conv_args* a, ConvDev& d) {
    if (!a || !a->x || !a->w || (!a->y && !a->y_f32)) return aldi_set_error_msg(ALDI_ERR_ARG, "conv_igemm: null pointer");
    const int bk = a->dtype == ALDI_BF16 ? 32 : 16;
    const int ep = a->dtype == ALDI_BF16 ? 8 : 4;
    if (a->dtype != ALDI_BF16 && a->dtype != ALDI_F32) return aldi_set_error_msg(ALDI_ERR_ARG, "conv_igemm: bad dtype");
    if (a->KH * a->KW == 1 ? (a->Cin % ep != 0) : (a->Cin % bk != 0))
        return aldi_set_error_msg(ALDI_ERR_ARG, "conv_igemm: Cin must be a multiple of 32 (bf16) / 16 (f32) for KxK convs; of a 16-B chunk for 1x1");
    if (a->Cout % 4 != 0) return aldi_set_error_msg(ALDI_ERR_ARG, "conv_igemm: Cout must be a multiple of 4");
    if (a->res_mode == 2 && ((a->Ho & 1) || (a->Wo & 1))) return aldi_set_error_msg(ALDI_ERR_ARG, "conv_igemm: upsample residual needs even Ho,Wo");
    if (a->res_mode < 0 || a->res_mode > 3 || (a->res_mode == 3 && a->out_scale > 1)) return aldi_set_error_msg(ALDI_ERR_ARG, "conv_igemm: res_mode is 0 .. 3 (3: dense output only)");
    if (a->res_mode && !a->res) return aldi_set_error_msg(ALDI_ERR_ARG, "conv_igemm: res_mode set without res");
    d.x = a->x; d.w = a->w; d.y = a->y; d.y_f32 = a->y_f32; d.scale = a->scale; d.shift = a->shift;
    d.res = a->res; d.mask = a->mask;
    d.N = a->N; d.H = a->H; d.W = a->W; d.Cin = a->Cin; d.Cout = a->Cout; d.KH = a->KH; d.KW = a->KW;
    d.stride = a->stride; d.pad = a->pad; d.Ho = a->Ho; d.Wo = a->Wo;
    d.relu = a->relu; d.res_mode = a->res_mode; d.out_scale = a->out_scale < 1 ? 1 : a->out_scale;
    d.OH = a->OH; d.OW = a->OW;
    long M = (long)a->N * a->Ho * a->Wo;
    if (M <= 0 || M > 0x7fffffffL) return aldi_set_error_msg(ALDI_ERR_ARG, "conv_igemm: bad M");
    d.M = (int)M;
    d.K = a->KH * a->KW * a->Cin;
    const size_t esz = a->dtype == ALDI_BF16 ? 2 : 4;
    const size_t xb = (size_t)a->N * a->H * a->W * a->Cin * esz, wb = (size_t)a->Cout * d.K * esz;
    const size_t yb = (size_t)a->N * (d.out_scale > 1 ? (size_t)a->OH * a->OW : (size_t)a->Ho * a->Wo) * a->Cout * esz;
    if (xb >= 0x80000000ull || wb >= 0x80000000ull || yb >= 0x80000000ull)
        return aldi_set_error_msg(ALDI_ERR_ARG, "conv_igemm: operand larger than 2 GiB (32-bit buffer offsets)");
    if (a->KH * a->KW > 16) return aldi_set_error_msg(ALDI_ERR_ARG, "conv_igemm: at most 16 taps");
    d.x_bytes = (unsigned)xb;
    d.w_bytes = (unsigned)wb;
    d.xcd = 0; d.dbg = 0;
    d.ksplit = 0; d.slabs_per_split = 0; d.lean = 0;
    d.mask_bits = static_cast<const unsigned char*>(a->mask_bits);
    d.bits_out = static_cast<unsigned char*>(a->bits_out);
    if ((a->mask_bits || a->bits_out) && (a->dtype != ALDI_BF16 || (a->Cout & 7) || d.out_scale != 1 || a->res_mode == 2 || !a->y || a->y_f32 || a->ksplit > 1))
        return aldi_set_error_msg(ALDI_ERR_ARG, "conv_igemm: bit masks take bf16 outputs with Cout % 8 == 0 in the plain layout (no fp32 output, scatter, upsampled residual or split-K)");
    if (a->mask_bits && a->mask) return aldi_set_error_msg(ALDI_ERR_ARG, "conv_igemm: mask and mask_bits are alternatives");
    return ALDI_OK;
}

// one convolution: d = the ConvDev to launch with c's kernel.  Split-K (a->ksplit > 1): d is the launch of the slices -- fp32 partial tiles
// to a->ws, no epilogue operand; the caller's finalize pass sums them and applies a's scale / shift / ReLU.
inline int plan_conv(const aldi_conv_args* a, const AldiTuning& tn, ConvDev& d, Choice& c) {
    if (int rc = fill_convdev(a, d)) return rc;
    if (a->ksplit > 1) {
        const int ks = a->ksplit;
        if (a->dtype != ALDI_BF16 || a->KH * a->KW != 1 || a->stride != 1 || a->pad != 0 || a->res_mode || a->mask || a->y_f32 || !a->y || !a->ws ||
            (a->out_scale > 1) || d.K % (64 * ks) != 0 || ks > 64)
            return aldi_set_error_msg(ALDI_ERR_ARG, "conv_igemm: split-K takes bf16 plain 1x1 / linear layers with K % (64 * ksplit) == 0, a workspace, no res / mask / fp32 output");
        d.y = nullptr; d.y_f32 = static_cast<float*>(a->ws); d.scale = nullptr; d.shift = nullptr; d.relu = 0;
        d.ksplit = ks;
    }
    c = select_tile(d, tn, a->dtype != ALDI_BF16, 0);
    d.xcd = tn.igemm_xcd; d.dbg = tn.igemm_dbg;
    if (c.ksplit > 1) d.slabs_per_split = d.K / (kTiles[c.tile].KC * 8) / c.ksplit;
    return ALDI_OK;
}

// one layer shape: everything that selects code paths inside the kernel template is equal; N, H x W (pyramid levels) and the
// tensors differ -- the tile heuristics look at the pixel count, Cout, K and the conv geometry ("same" padding or not) only
inline bool conv_group_same(const aldi_conv_args* args, int n, const AldiTuning& tn) {
    bool same = n <= kMaxConvGroup && tn.igemm_group;
    for (int i = 1; i < n && same; ++i) {
        const aldi_conv_args &a = args[0], &b = args[i];
        same = a.dtype == b.dtype && a.Cin == b.Cin && a.Cout == b.Cout && a.KH == b.KH && a.KW == b.KW &&
               a.stride == b.stride && a.pad == b.pad && (a.Ho == a.H) == (b.Ho == b.H) && (a.Wo == a.W) == (b.Wo == b.W) && a.out_scale == b.out_scale &&
               (a.y != nullptr) == (b.y != nullptr) && (a.y_f32 != nullptr) == (b.y_f32 != nullptr);
    }
    return same;
}

// n > 1 problems of one layer shape (conv_group_same) as ONE launch: G.p = the problems, largest first; d = what the tile is chosen for
inline int plan_conv_group(const aldi_conv_args* args, int n, const AldiTuning& tn, ConvGroup& G, ConvDev& d, Choice& c) {
    G.n = n;
    long Msum = 0;
    for (int i = 0; i < n; ++i) {
        if (int rc = fill_convdev(&args[i], G.p[i])) return rc;
        Msum += G.p[i].M;
    }
    for (int i = 1; i < n; ++i)         // largest problem first: the small ones' tiles fill its tail
        for (int j = i; j > 0 && G.p[j].M > G.p[j - 1].M; --j) { const ConvDev t_ = G.p[j]; G.p[j] = G.p[j - 1]; G.p[j - 1] = t_; }
    // the tile template is chosen for the COMBINED pixel count (the heuristics look at M, Cout, K and the conv geometry only)
    d = G.p[0];
    d.M = (int)(Msum > 0x7fffffffL ? 0x7fffffffL : Msum);
    c = select_tile(d, tn, args[0].dtype != ALDI_BF16, n, G.p);
    d.xcd = tn.igemm_xcd; d.dbg = tn.igemm_dbg;
    return ALDI_OK;
}

// ---- the pair form (igemm_pair.h): a 1x1 conv whose residual is a second 1x1 conv, formed in the same workgroup
struct PairPre {
    const void* x2; const void* w2; const float* scale2; const float* shift2;
    int H2, W2, Cin2, stride2;
    unsigned x2_bytes, w2_bytes;
};
// what igemm_pair_kernel takes: d = the main conv (fill_convdev), q = the inner one
inline bool pair_ok(const ConvDev& d, const bool f32, const PairPre& q) {
    return !f32 && plain_1x1(d) && d.y && !d.y_f32 && d.out_scale == 1 && !d.res_mode && !d.mask && !d.mask_bits && d.ksplit <= 1 && d.Cout % 64 == 0 &&
           d.K % 32 == 0 && q.x2 && q.w2 && q.Cin2 > 0 && q.Cin2 % 32 == 0 && q.stride2 >= 1 && q.H2 >= 1 && q.W2 >= 1 &&
           (q.H2 - 1) / q.stride2 + 1 == d.Ho && (q.W2 - 1) / q.stride2 + 1 == d.Wo;
}
// d: the main conv as the kernel takes it (res_mode = 1: its epilogue adds the inner conv's rounded result); two: the outer sum is rounded twice
inline int plan_conv_pair(const aldi_conv_args* a, const aldi_conv_pre_args* pre, const AldiTuning& tn, ConvDev& d, PairPre& q, bool& two) {
    if (!pre) return aldi_set_error_msg(ALDI_ERR_ARG, "conv_pair_igemm: null pointer");
    if (int rc = fill_convdev(a, d)) return rc;
    q = PairPre{pre->x2, pre->w2, pre->scale2, pre->shift2, pre->H2, pre->W2, pre->Cin2, pre->stride2, 0u, 0u};
    const size_t xb = (size_t)(a->N > 0 ? a->N : 0) * (size_t)(q.H2 > 0 ? q.H2 : 0) * (size_t)(q.W2 > 0 ? q.W2 : 0) * (size_t)(q.Cin2 > 0 ? q.Cin2 : 0) * 2;
    const size_t wb = (size_t)a->Cout * (size_t)(q.Cin2 > 0 ? q.Cin2 : 0) * 2;
    if (a->dtype != ALDI_BF16 || a->ksplit > 1 || !pair_ok(d, false, q) || xb >= 0x80000000ull || wb >= 0x80000000ull || (unsigned)pre->rounding > 2u)
        return aldi_set_error_msg(ALDI_ERR_ARG, "conv_pair_igemm: takes bf16, two 1x1 convs without padding on one output grid, the main one plain (stride 1, no res / "
                                                "mask / fp32 output / scatter / split-K), Cout % 64 == 0, Cin % 32 == 0, Cin2 % 32 == 0");
    q.x2_bytes = (unsigned)xb; q.w2_bytes = (unsigned)wb;
    d.res_mode = 1;                 // what the UNFUSED main launch is: the same conv with the inner one's map as `res`
    d.res = pre->x2;                // (never read: only "not null" matters to the selection)
    two = pre->rounding == 2;
    if (pre->rounding == 0) two = kTiles[select_tile(d, tn, false, 0).tile].epi == 0;
    d.res = nullptr;
    d.xcd = tn.igemm_xcd; d.dbg = tn.igemm_dbg;
    return ALDI_OK;
}
inline int pair_dispatch_name(const bool two, char* name, int cap) { return snprintf(name, cap, "igemm_pair<bf16,128,64,4,1,pipe,tap,round%d>", two ? 2 : 1); }

}  // namespace
