// lib.hip — what belongs to the whole library and to no kernel family: the thread-local error text behind
// wft_set_error / wft_last_error, and wft_version.  Host code only.
#include "common.h"
#include <stdarg.h>

static thread_local char g_err[512] = "";
void wft_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
extern "C" const char* wft_last_error(void) { return g_err; }
extern "C" const char* wft_version(void) { return "wft 0.1 gfx950" WFT_BUILD_KIND; }
