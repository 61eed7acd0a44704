// tests/hostsim_gatv2_dropout/launchers.cpp -- TEST INFRASTRUCTURE: the GATv2 entry points of the library with and without dropout
// (flex_amd/csrc/attention_gatv2_entry.h and attention_gatv2_dropout_entry.h, both included by this file) in a host-simulator build,
// on stand-in launchers that log the kernel instantiation the real ones (attention_gatv2_kernels.hip,
// attention_gatv2_dropout_kernels.hip) would launch and compute nothing.  tests/test_gatv2_dropout_entry_host.py compiles this file
// as one more source of tests/hostsim's library, as tests/test_gatv2_entry_host.py does with tests/hostsim_gatv2/launchers.cpp; that
// file and tests/hostsim/ stay as they are.  The log's lines are that file's, with "gatv2_dropout::" for the dropout launchers.
#include <cstdio>
#include <string>

#include "attention_gatv2_dropout_entry.h"
#include "attention_gatv2_entry.h"

namespace {
std::string g_log;  // one instantiation per line, in launch order

int logged(const char *space, const char *kernel, const flex::AttentionPick &pick, bool gxt = false, bool gatt = false) {
    char name[96];
    std::snprintf(name, sizeof name, "%s::%s<%d, %d>%s%s\n", space, kernel, pick.W, pick.NS, gxt ? " +gxt" : "", gatt ? " +gatt" : "");
    g_log += name;
    return FLEX_OK;
}
}  // namespace

namespace flex::gatv2 {
int launch_rows(const flex_plan *, const AttentionPick &pick, int, int, const float *, const float *, const float *, float, float *, float *, hipStream_t) {
    return logged("gatv2", "rows", pick);
}
// what the row launch was asked for stands behind its name: "+gxt", "+gatt"
int launch_rows_backward(const flex_plan *, const AttentionPick &pick, int, int, const float *, const float *, const float *, const float *,
                         const float *, float, float *GXt, float *, float *AttWork, hipStream_t) {
    return logged("gatv2", "rows_backward", pick, GXt != nullptr, AttWork != nullptr);
}
int launch_columns_backward(const flex_plan *, const AttentionPick &pick, int, int, const float *, const float *, const float *, const float *,
                            const float *, const float *, float, float *, hipStream_t) {
    return logged("gatv2", "columns_backward", pick);
}
int launch_att_reduce(const flex_plan *, const float *, float *, hipStream_t) {
    g_log += "gatv2::gatt_reduce\n";
    return FLEX_OK;
}
}  // namespace flex::gatv2

namespace flex::gatv2_dropout {
int launch_rows(const flex_plan *, const AttentionPick &pick, int, int, const float *, const float *, const float *, float, const DropMask &, float *,
                float *, hipStream_t) {
    return logged("gatv2_dropout", "rows", pick);
}
int launch_rows_backward(const flex_plan *, const AttentionPick &pick, int, int, const float *, const float *, const float *, const float *,
                         const float *, float, const DropMask &, float *GXt, float *, float *AttWork, hipStream_t) {
    return logged("gatv2_dropout", "rows_backward", pick, GXt != nullptr, AttWork != nullptr);
}
int launch_columns_backward(const flex_plan *, const AttentionPick &pick, int, int, const float *, const float *, const float *, const float *,
                            const float *, const float *, float, const DropMask &, float *, hipStream_t) {
    return logged("gatv2_dropout", "columns_backward", pick);
}
}  // namespace flex::gatv2_dropout

extern "C" {
void hostsim_gatv2_dropout_log_clear(void) { g_log.clear(); }
const char *hostsim_gatv2_dropout_log_read(void) { return g_log.c_str(); }
}
