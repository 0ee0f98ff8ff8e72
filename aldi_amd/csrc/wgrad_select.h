// What a weight-gradient call launches: the host-only half of wgrad.hip (no HIP types, no device code; compiles with a plain C++ compiler).
//
//   plan_wgrad      (args, n, entry point, knobs) -> WgPlan: the ordered list of launches of one call, the finalize items of the ordered
//                   epilogue and the workspace they are carved from.  Pure: no HIP call, no pointer dereferenced.
//   workspace_bytes what aldi_conv_wgrad_group_workspace answers
//   dispatch_name   WgPlan -> the string aldi_last_dispatch() reports
//
// wgrad.hip executes a plan: every launch (a switch over WgForm), then the finalize pass, then the dispatch note.
#pragma once
#include "host.h"
#include <limits.h>
#include <stdio.h>
#include <vector>

namespace {

// validated device-side description of one weight-gradient problem (the kernels' argument)
struct WgDev {
    const void* x; const void* g; float* dw; const float* scale; float* db;
    int N, H, W, Cin, Cout, KH, KW, stride, pad, Ho, Wo;
    int M, K, pix_per_split, ident, xcd, dbg;
    unsigned x_bytes, g_bytes, dw_bytes;
    // ordered epilogue (no float atomics): a pixel split writes its partial tile to `ws` (fragment order, 16 B per lane) and its
    // partial bias sums to `wsb`; wgrad_finalize_kernel adds the splits IN ORDER to dw / db.  splits == 1: the only owner of a tile
    // adds to dw with plain loads and stores.  ordered == 0: the float-atomic epilogue (callers without a workspace).
    float* ws; float* wsb;
    int splits, ordered;
};

// Grouped form: the weight gradients of SEVERAL layers in one launch.  A bottleneck stage's layers are small GEMMs (16-36 output
// tiles each) over the same 16800 pixels; launched one by one each needs an 11-24-way pixel split to occupy the chip, and every
// split ends in 16 K float atomics -- 20-50 % of the kernel time (tools/wgrad_sweep.py) -- plus a launch and a tail per layer.
// The backward pass does not need them one by one (nothing reads a weight gradient before the optimizer), so the engine
// collects a stage's layers and launches them together: hundreds of tiles, (almost) no pixel split, a handful of atomics.
constexpr int kMaxGroup = 24;
struct WgGroup {
    int n;
    int wg_begin[kMaxGroup + 1];      // first workgroup of each problem; wg_begin[n] = grid size
    int gx[kMaxGroup], gy[kMaxGroup], gz[kMaxGroup]; // output tiles and pixel splits of each problem (its workgroups: tile-fastest, then split)
    WgDev p[kMaxGroup];
};

// Second pass of the ordered epilogue: dw += scale * (split 0 + split 1 + ...), db += (...), the splits in index order -- the
// same bits on every run, and plain loads / stores.  One 256-thread workgroup per (tile, fragment, 4 waves of the producer).
struct WgFinItem {
    const float* ws; const float* wsb; float* dw; float* db; const float* scale;
    int Cout, K, gx, gy, S, big;
};
struct WgFin {
    int n;
    int wg_begin[kMaxGroup + 1];
    WgFinItem it[kMaxGroup];
};
// workgroups of one finalize item: (tile, fragment, four producer waves) + the bias workgroup
inline int fin_workgroups(const WgFinItem& it) { return it.gx * it.gy * (it.big ? 32 * 2 : 16) + 1; }

// ---- the launch forms: one row per kernel wgrad.hip launches.  X(id, printed name, threads per workgroup, output tile)
// Modifier (WgLaunch::ilv, knob wgrad_ilv): the interleaved loop of the big64 / big64 group / lean64 group templates.
#define WGRAD_FORMS(X) \
    X(WG_GENERIC,       "wgrad_bf16_generic",      256, 128) X(WG_LEAN,         "wgrad_bf16_lean",        256, 128) \
    X(WG_BIG,           "wgrad_bf16_big",          512, 256) X(WG_BIG64,        "wgrad_bf16_big64",       512, 256) \
    X(WG_DMA,           "wgrad_bf16_dma",          256, 128) X(WG_F32,          "wgrad_f32",              256, 64) \
    X(WG_F32_T128,      "wgrad_f32_t128",          256, 128) \
    X(WG_LEAN_GROUP,    "wgrad_bf16_lean_group",   256, 128) X(WG_LEAN_GROUP_DB, "wgrad_bf16_lean_group",  256, 128) \
    X(WG_LEAN64_GROUP,  "wgrad_bf16_lean64_group", 256, 128) X(WG_BIG_GROUP,    "wgrad_bf16_big_group",   512, 256) \
    X(WG_BIG64_GROUP,   "wgrad_bf16_big64_group",  512, 256)
enum WgForm {
#define WGRAD_FORM_ID(id, name, threads, tile) id,
    WGRAD_FORMS(WGRAD_FORM_ID)
#undef WGRAD_FORM_ID
    kNumWgForms
};
struct WgFormRow { const char* name; int threads, tile; };
constexpr WgFormRow kWgForms[kNumWgForms] = {
#define WGRAD_FORM_ROW(id, name, threads, tile) {name, threads, tile},
    WGRAD_FORMS(WGRAD_FORM_ROW)
#undef WGRAD_FORM_ROW
};
inline bool is_group_form(WgForm f) { return f >= WG_LEAN_GROUP; }

// one kernel launch of a call
struct WgLaunch {
    WgForm form;
    bool ilv;                 // the ilv template flag
    bool bias_pass;           // aldi_bias_grad(d.g, d.db, d.M, d.Cout, dtype) follows: only the lean / 256x256 kernels add the bias gradient themselves
    int dtype;
    int gx, gy, gz, lds;      // grid; dynamic LDS bytes (block: kWgForms[form].threads)
    WgDev d;                  // single forms: the kernel's argument
    int group;                // group forms: WgPlan::groups[group] is
    // what the name prints: pixel splits (single) / pixels per workgroup (group); " ordered" from d.ordered (single) / the CALL's flag, even when
    // every member keeps the atomic epilogue (group); "_db" from knob wgrad_db on every 128 x 128 group, the lean64 one included
    int splits; long pix; bool ordered_tag, db_tag;
};

struct WgPlan {
    std::vector<WgLaunch> launches;       // in launch order
    std::vector<WgFinItem> fin;           // second pass of the ordered epilogue: after ALL launches
    WgGroup groups[2];                    // (thread-local storage in the callers: cleared, not freed, between calls)
    int ngroups;
    float* ws_base; size_t ws_cap, ws_used;          // workspace of the ordered epilogue in floats, carved in 256-B units
    bool ordered;
    void reset(bool ordered_, float* base, size_t cap) {
        launches.clear(); fin.clear();
        ngroups = 0; ws_base = base; ws_cap = cap; ws_used = 0; ordered = ordered_;
    }
    float* take(size_t n_floats) {
        float* r = ws_base ? ws_base + ws_used : nullptr;
        ws_used += (n_floats + 63) / 64 * 64;
        return r;
    }
    bool fits() const { return ws_used <= ws_cap; }
};

// ---- argument checks: aldi_wgrad_args -> WgDev
inline int fill_wgdev(const aldi_wgrad_args* a, WgDev& d) {
    if (!a || !a->x || !a->g || !a->dw) return aldi_set_error_msg(ALDI_ERR_ARG, "conv_wgrad: null pointer");
    const int ep = a->dtype == ALDI_BF16 ? 8 : 4;
    if (a->Cin % ep || a->Cout % ep) return aldi_set_error_msg(ALDI_ERR_ARG, "conv_wgrad: Cin/Cout must be multiples of a 16-B chunk");
    d.x = a->x; d.g = a->g; d.dw = a->dw; d.scale = a->scale; d.db = a->db;
    d.N = a->N; d.H = a->H; d.W = a->W; d.Cin = a->Cin; d.Cout = a->Cout; d.KH = a->KH; d.KW = a->KW;
    d.stride = a->stride; d.pad = a->pad; d.Ho = a->Ho; d.Wo = a->Wo;
    long M = (long)a->N * a->Ho * a->Wo;
    if (M <= 0 || M > 0x7fffffffL) return aldi_set_error_msg(ALDI_ERR_ARG, "conv_wgrad: bad M");
    d.M = (int)M;
    d.K = a->KH * a->KW * a->Cin;
    const size_t esz = a->dtype == ALDI_BF16 ? 2 : 4;
    const size_t xb = (size_t)a->N * a->H * a->W * a->Cin * esz, gb = (size_t)M * a->Cout * esz;
    if (a->dtype == ALDI_BF16 && (xb >= 0x80000000ull || gb >= 0x80000000ull))
        return aldi_set_error_msg(ALDI_ERR_ARG, "conv_wgrad: operand larger than 2 GiB (32-bit buffer offsets)");
    d.x_bytes = (unsigned)xb;
    d.g_bytes = (unsigned)gb;
    const size_t wb = (size_t)a->Cout * d.K * 4;
    if (wb >= 0x80000000ull) return aldi_set_error_msg(ALDI_ERR_ARG, "conv_wgrad: gradient larger than 2 GiB (32-bit buffer offsets)");
    d.dw_bytes = (unsigned)wb;
    d.ident = (a->KH == 1 && a->KW == 1 && a->stride == 1 && a->pad == 0 && a->Ho == a->H && a->Wo == a->W) ? 1 : 0;
    d.pix_per_split = d.M; d.xcd = 0; d.dbg = 0;
    d.ws = d.wsb = nullptr; d.splits = 1; d.ordered = 0;
    return ALDI_OK;
}
// the lean / 256x256 / LDS-DMA kernels take bf16 1x1 stride-1 layers and "same"-padded K x K ones with whole 64-channel groups
inline bool lean_eligible(const aldi_wgrad_args* a, const WgDev& d) {
    const bool same = a->stride == 1 && a->Ho == a->H && a->Wo == a->W && 2 * a->pad == a->KH - 1 && a->KH == a->KW && a->Cin % 64 == 0;
    return a->dtype == ALDI_BF16 && (d.ident || same);
}
// 256x256 tile (one 8-wave workgroup per CU) when every workgroup still gets a long pixel range
inline bool wants_big_tile(const WgDev& d, const AldiTuning& tn) {
    if (tn.wgrad_big_min <= 0 || d.Cout % 256 || d.K % 256) return false;
    const int tb = (d.Cout / 256) * (d.K / 256);
    const int sb = tn.wgrad_big_slots / tb;            // floor: one 8-wave workgroup per CU, never 257 of them
    return cdiv(d.M, 64) / (sb > 0 ? sb : 1) >= tn.wgrad_big_min;
}

// The pixel ranges of problem d: d.pix_per_split pixels each (whole slabs of bp), recounted so that none is empty -> d.splits.
// T == 0: from a wanted COUNT -- at most slabs / 4 (at least 4 slabs of work behind every epilogue), at least 1, at most cap.
// T > 0: from a LENGTH (a group's common pixels per workgroup, a multiple of bp).
inline int split_pixels(WgDev& d, int bp, int want, int cap, long T = 0) {
    const int slabs = cdiv(d.M, bp);
    if (T <= 0) {
        if (want > slabs / 4) want = slabs / 4;
        if (want < 1) want = 1;
        if (want > cap) want = cap;
        T = (long)cdiv(slabs, want) * bp;
    } else if (T >= d.M) T = (long)slabs * bp;
    d.pix_per_split = (int)T;
    return d.splits = cdiv(d.M, d.pix_per_split);
}

// ordered epilogue of problem d (tile x tile output tiles, d.splits pixel ranges): workspace + second pass when split
inline void plan_ordered(WgDev& d, int big, WgPlan& P) {
    d.ordered = 1;
    d.ws = d.wsb = nullptr;
    if (d.splits <= 1) return;
    const int tile = big ? 256 : 128;
    const size_t gx = cdiv(d.Cout, tile), gy = cdiv(d.K, tile);
    d.ws = P.take(gx * gy * (size_t)d.splits * tile * tile);
    if (d.db) d.wsb = P.take(gx * (size_t)d.splits * tile);
    P.fin.push_back(WgFinItem{d.ws, d.wsb, d.dw, d.db, d.scale, d.Cout, d.K, (int)gx, (int)gy, d.splits, big});
}

// one problem alone (aldi_conv_wgrad; what a group forwards)
inline int plan_single(const aldi_wgrad_args* a, const AldiTuning& tn, bool ordered, WgPlan& P) {
    WgLaunch L = {};
    WgDev& d = L.d;
    if (int rc = fill_wgdev(a, d)) return rc;
    const bool bf16 = a->dtype == ALDI_BF16;
    const bool lean = tn.wgrad_lean && lean_eligible(a, d);
    const bool big = lean && wants_big_tile(d, tn);
    const bool f32_t128 = a->dtype == ALDI_F32 && tn.wgrad_f32_tile128 && d.Cout >= 128 && d.K >= 128;
    // LDS-DMA + transpose-read form (wgrad_dma: 0 off, 1 = 128x128 tile in place of the lean kernel, 2 = also in place of the 256x256 one)
    const bool dma = lean && tn.wgrad_dma > 0 && (d.ident ? a->Cin % 8 == 0 : a->Cin % 16 == 0) && a->KH * a->KW <= 25 && !(big && tn.wgrad_dma < 2);
    L.form = dma ? WG_DMA : big ? ((tn.wgrad_dma64 & 1) ? WG_BIG64 : WG_BIG) : lean ? WG_LEAN : bf16 ? WG_GENERIC : f32_t128 ? WG_F32_T128 : WG_F32;
    if (!bf16 && a->dtype != ALDI_F32) return aldi_set_error_msg(ALDI_ERR_ARG, "conv_wgrad: bad dtype");
    const int tile = kWgForms[L.form].tile;
    const int bp = bf16 ? 64 : (f32_t128 ? 32 : 16);
    const int slabs = cdiv(d.M, bp);
    const int tiles = cdiv(d.Cout, tile) * cdiv(d.K, tile);
    // the kernel is bound per CU (L2 -> CU path, LDS), not by latency: few, long splits (1-2 workgroups per CU) beat
    // many short ones, whose epilogues also contend on the same dW lines
    // (the 256x256 tile: floor of its own slots; the LDS-DMA kernel in its place: the 128x128 rule, and no cap)
    int want = L.form == WG_BIG || L.form == WG_BIG64 ? tn.wgrad_big_slots / tiles : cdiv(tn.wgrad_slots, tiles);
    if (f32_t128) {
        // MFMA-bound, two workgroups per CU (VGPRs): the launch runs in rounds of 512 workgroups, a round lasting (slabs per split + an
        // epilogue of ~6 slabs: 16 K float atomics per workgroup).  cdiv(512, tiles) splits put 576 workgroups = two rounds on
        // res5's 3x3 (169 us against 150 for the 64x64 kernel)
        long best = -1;
        for (int sp = 1; sp <= 512 && sp <= (slabs + 3) / 4; ++sp) {
            const long rounds = ((long)tiles * sp + 511) / 512;
            const long cost = rounds * (cdiv(slabs, sp) + 6);
            if (best < 0 || cost < best) { best = cost; want = sp; }
        }
    }
    L.splits = split_pixels(d, bp, want, dma && big ? INT_MAX : 512);
    d.xcd = tn.wgrad_xcd;
    d.dbg = tn.wgrad_dbg;
    if (L.form == WG_LEAN || L.form == WG_BIG || L.form == WG_BIG64) {
        if (ordered) plan_ordered(d, big, P);
        if (!P.fits()) return aldi_set_error_msg(ALDI_ERR_ARG, "conv_wgrad: workspace too small (aldi_conv_wgrad_group_workspace)");
    }
    L.ilv = L.form == WG_BIG64 && tn.wgrad_ilv;
    L.bias_pass = a->db && L.form != WG_LEAN && L.form != WG_BIG && L.form != WG_BIG64;
    L.dtype = a->dtype;
    L.gx = cdiv(d.Cout, tile); L.gy = cdiv(d.K, tile); L.gz = L.splits;
    L.ordered_tag = d.ordered != 0;
    P.launches.push_back(L);
    return ALDI_OK;
}

// one grouped launch of probs[0..ng) with a common pixel length per workgroup; big: 256x256 tiles, one workgroup per CU
inline int plan_group_launch(const WgDev* probs, int ng, bool big, const AldiTuning& tn, WgPlan& P) {
    const int tile = big ? 256 : 128;
    long tiles_of[kMaxGroup];
    int order[kMaxGroup];
    long maxM = 0;
    for (int i = 0; i < ng; ++i) {
        tiles_of[i] = (long)cdiv(probs[i].Cout, tile) * cdiv(probs[i].K, tile);
        if (probs[i].M > maxM) maxM = probs[i].M;
        order[i] = i;
    }
    auto wgs_for = [&](long T) {
        long w = 0;
        for (int i = 0; i < ng; ++i) w += tiles_of[i] * cdiv(probs[i].M, T);
        return w;
    };
    // Pixels per workgroup: ONE value T for the whole group (workgroups of equal length), chosen by a round model.  128x128: three
    // workgroups are resident per CU (168 VGPRs) and need each other to hide their LDS / DMA latency, so the chip works through
    // the launch in rounds of 768, a round lasting (T / 32 slab steps + one epilogue of ~wgrad_group_epi slab steps).  Measured on
    // the step's groups: 392 unsplit res4 tiles 603 us, three splits (1176 workgroups) 544 us; one 256-workgroup round of res3
    // 553 us against 432 us for 512 half-length workgroups.  256x256: one workgroup per CU, rounds of wgrad_big_slots.
    long T = (maxM + 63) / 64 * 64;
    const long target = big ? 0 : tn.wgrad_group_slots;
    if (target > 0) {
        while (T > 256 && wgs_for(T) < target) T = (T / 2 + 63) / 64 * 64;   // >= 4 slabs behind every epilogue
    } else {
        const long slots = big ? (tn.wgrad_big_slots > 0 ? tn.wgrad_big_slots : 256) : 768;
        const long epi = big ? tn.wgrad_big_epi : tn.wgrad_group_epi;
        const long minT = big ? 512 : 256;
        long best = -1;
        for (int sp = 1; sp <= 4096; ++sp) {
            const long Ts = ((maxM + sp - 1) / sp + 63) / 64 * 64;
            if (Ts < minT && sp > 1) break;
            const long rounds = (wgs_for(Ts) + slots - 1) / slots;
            const long cost = rounds * (Ts / 32 + epi);
            if (best < 0 || cost < best) { best = cost; T = Ts; }
        }
    }
    // longest-running problems first (K x K convs before 1x1: more k-steps per pixel do not matter, pixels per workgroup do)
    for (int i = 1; i < ng; ++i)
        for (int j = i; j > 0 && probs[order[j]].M > probs[order[j - 1]].M; --j) { int t_ = order[j]; order[j] = order[j - 1]; order[j - 1] = t_; }
    WgGroup& G = P.groups[P.ngroups];
    G.n = ng;
    int wg = 0;
    // wgrad_dma64 bit 2: the 128 x 128 group on the LDS-DMA + transpose-read loop when every layer's rows are whole 16-byte chunks
    bool lean64 = !big && (tn.wgrad_dma64 & 2);
    for (int k = 0; k < ng; ++k) {
        WgDev d = probs[order[k]];
        split_pixels(d, 64, 0, 0, T);
        if (P.ordered && d.ordered >= 0) plan_ordered(d, big, P);     // (d.ordered < 0: shares its gradient buffer)
        else d.ordered = 0;
        lean64 = lean64 && d.Cin % 8 == 0 && d.Cout % 8 == 0;
        G.p[k] = d;
        G.gx[k] = cdiv(d.Cout, tile);
        G.gy[k] = cdiv(d.K, tile);
        G.gz[k] = d.splits;
        G.wg_begin[k] = wg;
        wg += G.gx[k] * G.gy[k] * G.gz[k];
    }
    if (!P.fits()) return aldi_set_error_msg(ALDI_ERR_ARG, "conv_wgrad_group: workspace too small (aldi_conv_wgrad_group_workspace)");
    for (int k = ng; k <= kMaxGroup; ++k) G.wg_begin[k] = wg;
    WgLaunch L = {};
    L.form = big ? ((tn.wgrad_dma64 & 1) ? WG_BIG64_GROUP : WG_BIG_GROUP) : lean64 ? WG_LEAN64_GROUP : tn.wgrad_db ? WG_LEAN_GROUP_DB : WG_LEAN_GROUP;
    L.ilv = (L.form == WG_BIG64_GROUP || L.form == WG_LEAN64_GROUP) && tn.wgrad_ilv;
    L.gx = wg; L.gy = L.gz = 1;
    L.lds = L.form == WG_LEAN_GROUP ? tn.wgrad_lds_pad_kb << 10 : 0;
    L.group = P.ngroups++;
    L.pix = T; L.ordered_tag = P.ordered; L.db_tag = !big && tn.wgrad_db;
    P.launches.push_back(L);
    return ALDI_OK;
}

// The launches of aldi_conv_wgrad (group_entry false: args[0] alone) / aldi_conv_wgrad_group(args, n) into P, as the launch makes them: the ordered
// epilogue when the first problem brings a workspace (and knob wgrad_ordered), carved from that workspace.  query: as
// aldi_conv_wgrad_group_workspace plans -- ordered whatever the knob and the arguments say (callers size a grow-only buffer from it, and
// captured graphs hold its address), no limit, no addresses.
inline int plan_wgrad(const aldi_wgrad_args* args, int n, bool group_entry, bool query, const AldiTuning& tn, WgPlan& P) {
    if (group_entry && (!args || n < 1)) return aldi_set_error_msg(ALDI_ERR_ARG, "conv_wgrad_group: no problems");
    if (!args) return aldi_set_error_msg(ALDI_ERR_ARG, "conv_wgrad: null pointer");
    if (query) P.reset(true, nullptr, (size_t)-1);
    else P.reset(args[0].ws != nullptr && tn.wgrad_ordered, static_cast<float*>(args[0].ws), (size_t)args[0].ws_bytes / 4);
    if (!group_entry) return plan_single(args, tn, P.ordered, P);
    // problems the lean / 256x256 kernels cannot take (fp32, strided, unpadded ...) go through the single-problem dispatcher
    WgDev lean_p[kMaxGroup], big_p[kMaxGroup];
    int nl = 0, nb = 0;
    for (int i = 0; i < n; ++i) {
        WgDev d;
        if (int rc = fill_wgdev(&args[i], d)) return rc;
        // layers that SHARE a gradient buffer inside one call (one conv applied to several pyramid levels) would race in the plain
        // read-modify-write / second pass: those keep the float-atomic epilogue
        bool shared = false;
        for (int j = 0; j < n && !shared; ++j)
            shared = j != i && (args[j].dw == args[i].dw || (args[i].db && args[j].db == args[i].db));
        const bool elig = lean_eligible(&args[i], d) && tn.wgrad_lean;
        const bool big_group = elig && tn.wgrad_big_group && d.Cout % 256 == 0 && d.K % 256 == 0 && d.M >= 512 && nb < kMaxGroup;
        if (!elig || (!big_group && (nl == kMaxGroup || wants_big_tile(d, tn)))) {      // (alone, the big tile has its own launch)
            if (int rc = plan_single(&args[i], tn, P.ordered && !shared, P)) return rc;
            continue;
        }
        d.dbg = tn.wgrad_dbg;
        d.xcd = tn.wgrad_xcd;
        d.ordered = shared ? -1 : 0;
        if (big_group) big_p[nb++] = d; else lean_p[nl++] = d;
    }
    if (nb) {
        // a 256x256 launch wants a CU-count of workgroups with >= 1000 pixels each; a couple of tiles would be cut into hundreds of
        // short pixel ranges (each ending in a 256-KB partial tile) just to occupy the chip: those layers stay with the 128x128 group
        double tile_pixels = 0.0;
        for (int i = 0; i < nb; ++i) tile_pixels += (double)(big_p[i].Cout / 256) * (big_p[i].K / 256) * big_p[i].M;
        if (tile_pixels < 4096.0 * tn.wgrad_big_group_min && nl + nb <= kMaxGroup) {
            for (int i = 0; i < nb; ++i) lean_p[nl++] = big_p[i];
            nb = 0;
        }
    }
    if (nb) if (int rc = plan_group_launch(big_p, nb, true, tn, P)) return rc;
    if (nl) if (int rc = plan_group_launch(lean_p, nl, false, tn, P)) return rc;
    return ALDI_OK;
}

// bytes of workspace the ordered epilogue of aldi_conv_wgrad_group(args, n) needs; < 0: bad arguments
inline long workspace_bytes(const aldi_wgrad_args* args, int n, const AldiTuning& tn, WgPlan& P) {
    if (plan_wgrad(args, n, true, true, tn, P)) return -1;
    size_t need = P.ws_used;
    if (n == 1) {
        // one problem may be handed to aldi_conv_wgrad instead, whose dispatcher splits the pixels by its own rule (knob wgrad_slots): the larger of the two
        if (plan_wgrad(args, 1, false, true, tn, P)) return -1;
        if (P.ws_used > need) need = P.ws_used;
    }
    return (long)(need * 4);
}

// the name aldi_last_dispatch() reports: the group launches' ("<128 x 128 group> | <256 x 256 group>") when the call has any, else its last launch's
inline int dispatch_name(const WgPlan& P, char* name, int cap) {
    char part[2][96] = {"", ""};           // [0]: the 128 x 128 group, [1]: the 256 x 256 one
    const WgLaunch* last = nullptr;
    for (const WgLaunch& L : P.launches) {
        last = &L;
        if (!is_group_form(L.form)) continue;
        snprintf(part[kWgForms[L.form].tile == 256], sizeof(part[0]), "%s%s n=%d wgs=%d pix=%ld%s", kWgForms[L.form].name, L.db_tag ? "_db" : "", P.groups[L.group].n, L.gx,
                 L.pix, L.ordered_tag ? " ordered" : "");
    }
    if (P.ngroups) return snprintf(name, cap, "%s%s%s", part[0], (part[0][0] && part[1][0]) ? " | " : "", part[1]);
    if (!last) return snprintf(name, cap, "%s", "");
    return snprintf(name, cap, "%s splits=%d%s", kWgForms[last->form].name, last->splits, last->ordered_tag ? " ordered" : "");
}

}  // namespace
