// knob.hip - host side only: the switch every FNN_* test variable of the library is read through, and the kernel log
// (which kernel variant a launcher picked: fnn_kernel_log, tests and tools read it).
#include "fnn_device.h"
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

// nullptr unless FNN_KNOBS is set to something other than 0: a production process's environment changes no kernel
const char *fnn_knob(const char *name) {
    static const bool on = [] { const char *v = getenv("FNN_KNOBS"); return v && strcmp(v, "0") != 0; }();
    return on ? getenv(name) : nullptr;
}

static thread_local std::vector<std::string> *g_klog = nullptr;
void fnn_klog_target(void *v) { g_klog = (std::vector<std::string> *)v; }
void fnn_note_kernel(const char *fmt, ...) {
    if (!g_klog) return;
    char buf[160];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_klog->push_back(buf);
}
