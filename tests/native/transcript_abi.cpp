// The trh_tr_* entries of include/trh.h for tests/native/transcript_test.cpp, defined from csrc/transcript.h as csrc/capi.hip defines them for
// the library, with the two things they need from it: set_error and trh_last_error.  Host only; compiled under address + undefined sanitizers.
#include <stdarg.h>

#define TRH_TRANSCRIPT_ABI
#include "../../tiny-ram-halo2_amd/csrc/transcript.h"

static thread_local char g_err[512] = "";
void trh::set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char* trh_last_error(void) { return g_err; }
