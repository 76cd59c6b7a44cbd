// The C prologue every companion library shares (beam, logits, score, spec, spec_sample; wq and w4 through qgemv.hpp): the
// thread's last error text, the launch check, and the two entry points each companion's header declares next to its own,
// vly_<name>_abi_version / vly_<name>_last_error.  Each companion is ONE translation unit, so the anonymous namespace gives
// every library its own error buffer; the main library's vly_set_error (capi.hip) is shared between units and stays there.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>

namespace {

thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// after a launch: 0, or the runtime's refusal recorded under the entry point's name
int check_launch(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: launch failed: %s", what, hipGetErrorString(e));
        return -(1000 + (int)e);
    }
    return 0;
}

}  // namespace

// VLY_COMPANION_CAPI(beam, VLY_BEAM_ABI_VERSION) defines vly_beam_abi_version and vly_beam_last_error
#define VLY_COMPANION_CAPI(name, version)                                  \
    extern "C" int vly_##name##_abi_version(void) { return version; }     \
    extern "C" const char* vly_##name##_last_error(void) { return g_err; }
