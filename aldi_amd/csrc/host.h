// What host-only code shares (no HIP types: compiles with a plain C++ compiler): the tuning knobs, the error text, the dispatch note.
#pragma once
#include "../../include/aldi_hip.h"

int aldi_set_error_msg(int code, const char* msg);

typedef uint16_t bf16_t;  // raw bf16 storage

// run-time tuning knobs (aldi_set_tuning / ALDI_<NAME> environment defaults; core.hip).  ONE list: X(name, default) gives the AldiTuning
// fields here and the name table of aldi_set_tuning / aldi_get_tuning in core.hip; include/aldi_hip.h documents every knob
// (tests/test_conv_dispatch_cpu.py holds that comment and this list to each other).
#define ALDI_KNOBS(X) \
    X(igemm_xcd, 1) X(igemm_tile, 0) X(igemm_dbg, 0) X(igemm_bigtile_min, 1024) X(igemm_bigtile, 64) X(igemm_bigtile_k, 768) X(igemm_lintile_min, 768) \
    X(igemm_halo, 1) X(igemm_force, 0) X(igemm_k64_min, 1024) X(igemm_group, 1) X(igemm_narrow_k, 512) X(igemm_splitk_tile, 2) X(igemm_halo_f32, 0) \
    X(igemm_f32_tile64_max, 4096) X(igemm_direct, 15) X(igemm_lean, 1) X(igemm_halo64_mid, 0) X(igemm_ws, 1) X(igemm_ws_wgs, 512) X(igemm_ws_min, 40000) \
    X(wgrad_lean, 1) X(wgrad_big_min, 28) X(wgrad_big_slots, 256) X(wgrad_slots, 384) X(wgrad_xcd, 1) \
    X(igemm_halo_ilv, 1) X(igemm_halo_small, 0) X(igemm_halo96, 0) \
    X(wgrad_dma, 0) X(wgrad_dbg, 0) X(wgrad_group_slots, 0) X(wgrad_group_epi, 24) X(wgrad_db, 0) X(wgrad_ordered, 1) X(wgrad_big_group, 1) X(wgrad_big_epi, 12) \
    X(wgrad_big_group_min, 64) X(wgrad_lds_pad_kb, 0) X(wgrad_f32_tile128, 1) X(wgrad_dma64, 3) X(wgrad_ilv, 0) \
    X(msda_gather, 7) X(msda_gather_list, 1500) X(msda_bin, 1) X(msda_bin_list, 512) X(roialign_sep, 1) X(roialign_bwd_rows, 2) \
    X(colsum_blocks, 256) X(colsum_minrows, 16) X(colsum_nt, 1024) X(colsum_block_kb, 384) \
    X(stem_mfma, 1) X(stem_pool_wgs, 0) X(sab_blocks, 512) X(ln_bwd_blocks, 512) X(ln_bwd_blocks_narrow, 1024) X(rpn_topk_fused, 1) X(ema_blocks, 2048) X(nms_mask_tri, 1) X(match_wave, 1) \
    X(resize_fused, 1)

struct AldiTuning {
#define ALDI_KNOB_FIELD(name, dflt) int name;
    ALDI_KNOBS(ALDI_KNOB_FIELD)
#undef ALDI_KNOB_FIELD
};
AldiTuning& aldi_tuning();
void aldi_note_dispatch(const char* kernel);   // what aldi_last_dispatch() reports (thread local)

static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }
