// tests/hostsim_gatv2/launchers.cpp -- TEST INFRASTRUCTURE: the GATv2 entry points of the library (flex_amd/csrc/attention_gatv2_entry.h,
// included by this file) in a host-simulator build, on stand-in launchers that log the kernel instantiation the real ones
// (attention_gatv2_kernels.hip) would launch and compute nothing.  tests/test_gatv2_entry_host.py compiles this file as one more
// source of tests/hostsim's library (hostsim.build(extra_flags=(this file,), out=...)), so tests/hostsim/ itself stays as it is.  The
// shim's launch log is local to its file; this one keeps a log and accessors of its own, which is always on.
#include <cstdio>
#include <string>

#include "attention_gatv2_entry.h"

namespace {
std::string g_log;  // one instantiation per line, in launch order

int logged(const char *kernel, const flex::AttentionPick &pick) {
    char name[96];
    std::snprintf(name, sizeof name, "gatv2::%s<%d, %d>\n", kernel, pick.W, pick.NS);
    g_log += name;
    return FLEX_OK;
}
}  // namespace

namespace flex::gatv2 {
int launch_rows(const flex_plan *, const AttentionPick &pick, int, int, const float *, const float *, const float *, float, float *, float *, hipStream_t) {
    return logged("rows", pick);
}
// what the row launch was asked for stands behind its name: "+gxt", "+gatt"
int launch_rows_backward(const flex_plan *, const AttentionPick &pick, int, int, const float *, const float *, const float *, const float *,
                         const float *, float, float *GXt, float *, float *AttWork, hipStream_t) {
    logged("rows_backward", pick);
    g_log.pop_back();
    g_log += GXt ? " +gxt" : "";
    g_log += AttWork ? " +gatt" : "";
    g_log += '\n';
    return FLEX_OK;
}
int launch_columns_backward(const flex_plan *, const AttentionPick &pick, int, int, const float *, const float *, const float *, const float *,
                            const float *, const float *, float, float *, hipStream_t) {
    return logged("columns_backward", pick);
}
int launch_att_reduce(const flex_plan *, const float *, float *, hipStream_t) {
    g_log += "gatv2::gatt_reduce\n";
    return FLEX_OK;
}
}  // namespace flex::gatv2

extern "C" {
void hostsim_gatv2_log_clear(void) { g_log.clear(); }
const char *hostsim_gatv2_log_read(void) { return g_log.c_str(); }
}
