// tests/hostsim_gat_edge/launchers.cpp -- TEST INFRASTRUCTURE: the entry points of the fused GAT attention with a per-edge score term
// (flex_amd/csrc/attention_gat_edge_entry.h, included by this file) in a host-simulator build, on stand-in row launchers that log the
// kernel instantiation the real ones (attention_gat_edge_kernels.hip) would launch and compute nothing.
// tests/test_gat_edge_entry_host.py compiles this file as one more source of tests/hostsim's library, as
// tests/test_gatv2_dropout_entry_host.py does with its launchers.cpp; tests/hostsim/ stays as it is.  The column launch of the backward
// is the GAT family's, so it is tests/hostsim/shim.cpp's stand-in that answers it, in the shim's own log (hostsim_launch_log).
#include <cstdio>
#include <string>

#include "attention_gat_edge_entry.h"

namespace {
std::string g_log;  // one instantiation per line, in launch order

int logged(const char *kernel, const flex::AttentionPick &pick, bool drop, const char *tail, const void *work = nullptr) {
    char name[144], where[40] = "";
    if (work) std::snprintf(where, sizeof where, " work=%p", work);
    std::snprintf(name, sizeof name, "gat_edge::%s<%d, %d, %s>%s%s\n", kernel, pick.W, pick.NS, drop ? "true" : "false", tail, where);
    g_log += name;
    return FLEX_OK;
}
}  // namespace

namespace flex::gat_edge {
int launch_rows(const flex_plan *, const AttentionPick &pick, int, int, const float *, const float *, const float *, const float *, float,
                const DropMask *dm, float *, float *P, hipStream_t) {
    return logged("gat_edge_rows", pick, dm != nullptr, P ? "" : " -p");
}
// what the row launch was asked for stands behind its name: "+gel", and the address of the work array it was handed
int launch_rows_backward(const flex_plan *, const AttentionPick &pick, int, int, const float *, const float *, const float *, const float *,
                         const float *, const float *, float, const DropMask *dm, float *GEl, float *Work, hipStream_t) {
    return logged("gat_edge_rows_backward", pick, dm != nullptr, GEl ? " +gel" : "", Work);
}
}  // namespace flex::gat_edge

extern "C" {
void hostsim_gat_edge_log_clear(void) { g_log.clear(); }
const char *hostsim_gat_edge_log_read(void) { return g_log.c_str(); }
}
