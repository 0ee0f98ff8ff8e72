// Error plumbing of libaldi_hip.so (no exceptions cross the C ABI).
#include "common.h"
#include <stdio.h>
#include <string.h>

static thread_local char g_err[512] = "";

int aldi_set_error(hipError_t e, const char* file, int line) {
    snprintf(g_err, sizeof(g_err), "HIP error %d (%s) at %s:%d", (int)e, hipGetErrorString(e), file, line);
    return ALDI_ERR_HIP;
}
int aldi_set_error_msg(int code, const char* msg) {
    snprintf(g_err, sizeof(g_err), "%s", msg);
    return code;
}
extern "C" const char* aldi_last_error(void) { return g_err; }
extern "C" int aldi_version(void) { return 1; }

// an empty one-workgroup launch: what timing harnesses calibrate the cost of a launch / an event pair with
namespace { __global__ void noop_kernel() {} }
extern "C" int aldi_noop(aldi_stream_t stream) {
    hipLaunchKernelGGL(noop_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream));
    ALDI_CHECK_LAUNCH();
    return ALDI_OK;
}

// ---- tuning knobs (include/aldi_hip.h: aldi_set_tuning) -------------------------------------------------------------
// One table; the defaults can be overridden once from the environment (ALDI_<UPPER-CASE NAME>) and at any time through
// the C ABI, so a single test process can select every dispatch arm.
#include <stdlib.h>
namespace {
struct Knob { const char* name; int AldiTuning::*field; int dflt; };
const Knob kKnobs[] = {
#define ALDI_KNOB_ROW(name, dflt) {#name, &AldiTuning::name, dflt},
    ALDI_KNOBS(ALDI_KNOB_ROW)
#undef ALDI_KNOB_ROW
};
AldiTuning make_tuning() {
    AldiTuning t;
    for (const Knob& k : kKnobs) {
        char env[64] = "ALDI_";
        size_t n = strlen(env);
        for (const char* c = k.name; *c && n + 1 < sizeof(env); ++c) env[n++] = (*c >= 'a' && *c <= 'z') ? (char)(*c - 32) : *c;
        env[n] = 0;
        const char* v = getenv(env);
        t.*(k.field) = v ? atoi(v) : k.dflt;
    }
    return t;
}
thread_local char g_dispatch[224] = "";
}  // namespace

AldiTuning& aldi_tuning() {
    static AldiTuning t = make_tuning();
    return t;
}
void aldi_note_dispatch(const char* kernel) { snprintf(g_dispatch, sizeof(g_dispatch), "%s", kernel); }

extern "C" int aldi_set_tuning(const char* name, int value) {
    if (!name) return aldi_set_error_msg(ALDI_ERR_ARG, "set_tuning: null name");
    for (const Knob& k : kKnobs)
        if (!strcmp(k.name, name)) { aldi_tuning().*(k.field) = value; return ALDI_OK; }
    return aldi_set_error_msg(ALDI_ERR_ARG, "set_tuning: unknown knob");
}
extern "C" int aldi_get_tuning(const char* name, int* value) {
    if (!name || !value) return aldi_set_error_msg(ALDI_ERR_ARG, "get_tuning: null argument");
    for (const Knob& k : kKnobs)
        if (!strcmp(k.name, name)) { *value = aldi_tuning().*(k.field); return ALDI_OK; }
    return aldi_set_error_msg(ALDI_ERR_ARG, "get_tuning: unknown knob");
}
extern "C" int aldi_reset_tuning(void) {
    aldi_tuning() = make_tuning();
    return ALDI_OK;
}
extern "C" const char* aldi_last_dispatch(void) { return g_dispatch; }
