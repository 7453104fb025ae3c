// ABI version + thread-local error string.  The entry points themselves live beside their kernels (the newest, additive within ABI 14:
// pag_tv_* in regularizer.hip, pag_sample_* in sample.hip, pag_vis_* - the validation pictures of pc_nerf/trainer.py:710-829 - in visualize.hip).
#include <stdarg.h>
#include <stdio.h>
#include "../../include/pagnerf_hip.h"

static thread_local char g_err[512] = "";

void pag_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" int pag_abi_version(void) { return PAG_ABI_VERSION; }
extern "C" const char *pag_last_error_string(void) { return g_err; }
