"""ctypes binding of include/flex_spmm.h (the C ABI of libflex_spmm.so).

Device buffers are raw pointers (``tensor.data_ptr()``), streams are raw hipStream_t
values (``torch.cuda.current_stream().cuda_stream``): torch is plumbing here, the
kernels live in the shared library.  There is no fallback: if the library is missing
or a call fails, FlexError is raised.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "csrc")
_SO = os.path.join(_HERE, "lib", "libflex_spmm.so")

FLEX_ORDER_NATURAL = 0
FLEX_ORDER_RCM = 1
FLEX_ORDER_CLUSTER = 2
FLEX_ORDER_GORDER = 3
FLEX_PLAN_STATS = 0x100
FLEX_PLAN_AUTOTUNE = 0x200
FLEX_PLAN_ROW_RANGE = 0x1000
FLEX_PLAN_XCD_INTERLEAVE = 0x2000
FLEX_PLAN_TRANSPOSE = 0x8000
FLEX_PLAN_MUTABLE_VALUES = 0x10000
FLEX_PLAN_ATTENTION = 0x40000
FLEX_PLAN_ATTENTION_BACKWARD = 0x80000
FLEX_PLAN_BF16 = 0x100000


class FlexError(RuntimeError):
    pass


class _Csr(C.Structure):  # flex_csr
    _fields_ = [("m", C.c_int32), ("n", C.c_int32), ("nnz", C.c_int64),
                ("rowPtr", C.c_void_p), ("col", C.c_void_p), ("vals", C.c_void_p)]


class _HostCsr(C.Structure):  # flex_host_csr
    _fields_ = [("m", C.c_int32), ("n", C.c_int32), ("nnz", C.c_int64),
                ("rowPtr", C.POINTER(C.c_uint32)), ("col", C.POINTER(C.c_uint32)),
                ("vals", C.POINTER(C.c_float)),
                ("uni_nb", C.c_int64), ("n_edges_one_way", C.c_int64),
                ("n_edges_asymmetric", C.c_int64),
                ("n_nodes_z_out", C.c_int32), ("n_nodes_z_in", C.c_int32),
                ("n_nodes_z_deg", C.c_int32), ("is_directed", C.c_int32), ("c", C.c_int32)]


class _PlanInfo(C.Structure):  # flex_plan_info
    _fields_ = [("m", C.c_int32), ("n", C.c_int32), ("k", C.c_int32), ("device", C.c_int32),
                ("nnz", C.c_int64), ("n_tasks", C.c_int64), ("n_chunks", C.c_int64),
                ("n_split_rows", C.c_int64), ("n_partials", C.c_int64),
                ("device_bytes", C.c_int64), ("lanes_per_nz", C.c_int32), ("order", C.c_int32),
                ("plan_ms", C.c_double), ("n_slots", C.c_int64), ("two_d", C.c_int32), ("panel_rows", C.c_int32),
                ("n_tiles", C.c_int64), ("tile_nnz", C.c_int64), ("n_records", C.c_int64),
                ("n_blocks", C.c_int64), ("block_rows", C.c_int64), ("block_nnz", C.c_int64), ("block_hot_nnz", C.c_int64),
                ("block_hot_cols", C.c_int64), ("block_panels", C.c_int64), ("block_records", C.c_int64),
                ("n_bundles", C.c_int64), ("bundle_rows", C.c_int64),
                ("n_moved_pieces", C.c_int64), ("moved_records", C.c_int64)]


class _PlanStats(C.Structure):  # flex_plan_stats
    _fields_ = [("records", C.c_int64), ("cols_wave", C.c_int64), ("cols_wg", C.c_int64),
                ("cols_xcd", C.c_int64), ("reuse_wave", C.c_double), ("reuse_wg", C.c_double),
                ("reuse_xcd", C.c_double), ("gather_bytes", C.c_double), ("l2_bytes", C.c_double),
                ("chunk_rec_max", C.c_int64), ("chunk_rec_mean", C.c_double),
                ("chunk_imb_pct", C.c_double), ("xcd_imb_pct", C.c_double),
                ("split_nnz_pct", C.c_double), ("pad_pct", C.c_double), ("n_workgroups", C.c_int64),
                ("tile_nnz_pct_10", C.c_double), ("tile_nnz_pct_25", C.c_double), ("tile_nnz_pct_50", C.c_double),
                ("tile_mean_fill", C.c_double), ("mfma_tiles", C.c_int64), ("mfma_nnz_pct", C.c_double),
                ("lds_hot_pct_2", C.c_double), ("lds_hot_pct_4", C.c_double), ("lds_u_2", C.c_double), ("lds_u_4", C.c_double)]


class _ClusterTuning(C.Structure):  # flex_cluster_tuning
    _fields_ = [(f, C.c_int32) for f in ("batch", "no_refine", "stretch", "sweeps", "stride")]


class _PlanTuning(C.Structure):  # flex_plan_tuning: every field 0 = the planner's rule
    _fields_ = [(f, C.c_int32) for f in (
        "lanes_per_nz", "chunk_records", "long_row", "piece_records", "row_cost", "xcd_slices", "xcd_balance",
        "chunk_cost", "task_cost", "split_rows", "rec_nt", "unroll", "two_d", "panel_kb", "seg_min", "mfma",
        "mfma_fill_pct", "lds_extra", "host_threads")] + [("cluster", _ClusterTuning)] + [(f, C.c_int32) for f in (
        "blocks", "block_rounds", "block_panel_rows", "block_thr", "block_cap", "block_ablate_retired", "tile_group", "xcd_stretch", "far_first", "bundle", "bundle_len", "rec_pack",
        "hub_row", "hub_window", "hub_min_run")] + [("reserved", C.c_int32 * 1)]


TUNING_FIELDS = tuple(f for f, _ in _PlanTuning._fields_ if f not in ("cluster", "block_ablate_retired", "reserved"))
CLUSTER_TUNING_FIELDS = tuple(f for f, _ in _ClusterTuning._fields_)


# Knobs applied to every Plan() of this PROCESS that does not name them itself: a convenience of this binding for tests and
# tools whose plans are created inside helpers (the library has no such state: it only sees the descriptor it is handed).
DEFAULT_TUNING: dict = {}


def _tuning(d) -> "_PlanTuning | None":
    """dict -> flex_plan_tuning; keys are its field names, cluster knobs as cluster_<field> (cluster_no_refine=1 ...)."""
    if not d:
        return None
    t = _PlanTuning()
    for key, val in d.items():
        if key in TUNING_FIELDS:
            setattr(t, key, int(val))
        elif key.startswith("cluster_") and key[8:] in CLUSTER_TUNING_FIELDS:
            setattr(t.cluster, key[8:], int(val))
        else:
            raise FlexError(f"unknown tuning knob {key!r} (flex_plan_tuning has: {', '.join(TUNING_FIELDS)}, cluster_*)")
    return t


class _PlanDesc(C.Structure):  # flex_plan_desc
    _fields_ = [("struct_size", C.c_size_t), ("A", C.POINTER(_Csr)), ("k", C.c_int), ("ldb", C.c_int), ("ldc", C.c_int),
                ("device", C.c_int), ("flags", C.c_uint), ("row_begin", C.c_int64), ("row_end", C.c_int64),
                ("col_map", C.c_void_p), ("row_map", C.c_void_p), ("tuning", C.POINTER(_PlanTuning))]


class _KernelInfo(C.Structure):  # flex_kernel_info
    _fields_ = [("vgprs", C.c_int32), ("sgprs", C.c_int32), ("lds_bytes", C.c_int32), ("scratch_bytes", C.c_int32),
                ("threads_per_block", C.c_int32), ("waves_per_cu", C.c_int32)]


class _Imbalance(C.Structure):  # flex_imbalance
    _fields_ = [("waves", C.c_int64), ("cus_seen", C.c_int32), ("xcds_seen", C.c_int32), ("span_us", C.c_double),
                ("cu_busy_imb_pct", C.c_double), ("cu_end_spread_pct", C.c_double), ("xcd_busy_imb_pct", C.c_double),
                ("xcd_end_spread_pct", C.c_double), ("wave_us_mean", C.c_double), ("wave_us_max", C.c_double)]


class _SoftmaxInfo(C.Structure):  # flex_softmax_info
    _fields_ = [(f, C.c_int64) for f in ("rows", "entries", "items", "groups", "rows_empty", "rows_packed", "rows_wave", "rows_block",
                                          "group_entries", "device_bytes")]


class _AttentionInfo(C.Structure):  # flex_attention_info
    _fields_ = [(f, C.c_int64) for f in ("rows", "entries", "items", "groups", "rows_empty", "rows_slot", "rows_wave", "rows_block",
                                          "group_budget", "device_bytes")]


class _AttentionBackwardInfo(C.Structure):  # flex_attention_backward_info
    _fields_ = [(f, C.c_int64) for f in ("columns", "entries", "items", "groups", "columns_empty", "columns_slot", "columns_wave", "columns_block",
                                          "group_budget", "device_bytes")]


class _RecordInfo(C.Structure):  # flex_record_info
    _fields_ = [("packed", C.c_int32), ("reserved", C.c_int32)] + [(f, C.c_int64) for f in ("records", "wide_records", "exceptions", "stream_bytes")]


class _SynthParams(C.Structure):  # flex_synth_params
    _fields_ = [("n", C.c_int64), ("nnz", C.c_int64), ("alpha", C.c_double),
                ("community", C.c_int64), ("p_in", C.c_double), ("p_near", C.c_double),
                ("near_window", C.c_int32), ("shuffle", C.c_int32), ("gcn_norm", C.c_int32),
                ("directed", C.c_int32), ("seed", C.c_uint64)]


# every symbol include/flex_spmm.h declares (tests/test_abi.py checks the header against this)
SYMBOLS = [
    "flex_plan_create", "flex_plan_create_ex", "flex_plan_create_ld", "flex_plan_create_mapped", "flex_plan_create_rows", "flex_spmm",
    "flex_plan_destroy", "flex_plan_measure_imbalance", "flex_plan_get_info", "flex_plan_get_stats", "flex_plan_get_tuning", "flex_set_host_threads", "flex_order_cluster_ex", "flex_plan_self_check", "flex_plan_kernel_info", "flex_hbm_probe", "flex_gather_rows", "flex_csv_load", "flex_mtx_load",
    "flex_csv_save", "flex_csr_save_bin", "flex_csr_load_bin", "flex_csr_fingerprint", "flex_perm_save", "flex_perm_load",
    "flex_host_csr_free", "flex_fill_dense_rand", "flex_order_rcm", "flex_order_cluster", "flex_order_gorder", "flex_perm_csr",
    "flex_order_deg", "flex_order_dfs", "flex_order_rabbit", "flex_shard_rows", "flex_synth_graph", "flex_synth_preset", "flex_strerror", "flex_last_hip_error",
    "flex_last_hip_error_string", "flex_abi_version", "flex_plan_set_values", "flex_sddmm",
    "flex_edge_softmax", "flex_edge_softmax_backward", "flex_plan_softmax_info", "flex_attention", "flex_plan_attention_info",
    "flex_attention_backward", "flex_plan_attention_backward_info", "flex_attention_heads", "flex_attention_heads_backward",
    "flex_gat_attention", "flex_gat_attention_backward", "flex_plan_record_info", "flex_plan_read_records",
    "flex_attention_bf16", "flex_attention_bf16_backward", "flex_spmm_bf16", "flex_plan_is_bf16",
    "flex_attention_bias", "flex_attention_bias_backward", "flex_attention_bf16_bias", "flex_attention_bf16_bias_backward",
    "flex_attention_dropout", "flex_attention_dropout_backward", "flex_attention_bf16_dropout", "flex_attention_bf16_dropout_backward",
    "flex_dropout_mask", "flex_gat_attention_dropout", "flex_gat_attention_dropout_backward",
    "flex_gat_attention_bf16", "flex_gat_attention_bf16_backward", "flex_gat_attention_bf16_dropout", "flex_gat_attention_bf16_dropout_backward",
    "flex_gatv2_attention", "flex_gatv2_attention_backward", "flex_gatv2_attention_work_size",
    "flex_dropout_gatv2_attention", "flex_dropout_gatv2_attention_backward",
    "flex_edge_gat_attention", "flex_edge_gat_attention_backward",
]

_lib = None


def lib_path() -> str:
    return _SO


def build(force: bool = False) -> str:
    """Compile libflex_spmm.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    if force and os.path.exists(_SO):
        os.remove(_SO)
    subprocess.check_call(["make", "-s", "-C", _CSRC, "all"])
    return _SO


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_SO):
            raise FlexError(f"{_SO} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                            "(there is no CPU fallback)")
        # torch bundles its own libamdhip64.so; if ours were loaded first, libflex_spmm.so would bind
        # to /opt/rocm's copy and the process would hold TWO HIP runtimes (the second one sees no
        # device, and pointers/streams of one are foreign to the other).  Import torch first so the
        # library resolves to the runtime that owns the tensors it is handed.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(_SO)
        vp, i64, i32, u32 = C.c_void_p, C.c_int64, C.c_int, C.c_uint
        L.flex_plan_create.argtypes = [C.POINTER(vp), C.POINTER(_Csr), i32, i32, u32]
        L.flex_plan_create_ex.argtypes = [C.POINTER(vp), C.POINTER(_PlanDesc)]
        L.flex_plan_create_ld.argtypes = [C.POINTER(vp), C.POINTER(_Csr), i32, i32, i32, i32, u32]
        L.flex_plan_create_mapped.argtypes = [C.POINTER(vp), C.POINTER(_Csr), vp, i32, i32, u32]
        L.flex_plan_create_rows.argtypes = [C.POINTER(vp), C.POINTER(_Csr), i64, i64, vp, i32, i32, u32]
        L.flex_spmm.argtypes = [vp, vp, vp, vp]
        L.flex_plan_destroy.argtypes = [vp]
        L.flex_plan_get_info.argtypes = [vp, C.POINTER(_PlanInfo)]
        L.flex_plan_get_stats.argtypes = [vp, C.POINTER(_PlanStats)]
        L.flex_plan_get_tuning.argtypes = [vp, C.POINTER(_PlanTuning)]
        L.flex_set_host_threads.argtypes = [i32]
        L.flex_order_cluster_ex.argtypes = [C.POINTER(_Csr), C.POINTER(_ClusterTuning), vp]
        L.flex_plan_self_check.argtypes = [vp]
        L.flex_plan_measure_imbalance.argtypes = [vp, vp, vp, vp, C.POINTER(_Imbalance)]
        L.flex_plan_kernel_info.argtypes = [vp, C.POINTER(_KernelInfo)]
        L.flex_gather_rows.argtypes = [vp, vp, vp, i64, i32, vp]
        L.flex_hbm_probe.argtypes = [i32, i64, i32, i32, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.flex_csv_load.argtypes = [C.c_char_p, C.POINTER(_HostCsr)]
        L.flex_mtx_load.argtypes = [C.c_char_p, i32, C.POINTER(_HostCsr)]
        L.flex_csv_save.argtypes = [C.c_char_p, C.POINTER(_Csr)]
        L.flex_csr_fingerprint.argtypes = [C.POINTER(_Csr)]
        L.flex_csr_fingerprint.restype = C.c_uint64
        L.flex_perm_save.argtypes = [C.c_char_p, vp, i64, C.c_uint64]
        L.flex_perm_load.argtypes = [C.c_char_p, vp, i64, C.c_uint64]
        L.flex_csr_save_bin.argtypes = [C.c_char_p, C.POINTER(_Csr)]
        L.flex_csr_load_bin.argtypes = [C.c_char_p, C.POINTER(_HostCsr)]
        L.flex_host_csr_free.argtypes = [C.POINTER(_HostCsr)]
        L.flex_host_csr_free.restype = None
        L.flex_fill_dense_rand.argtypes = [vp, i64, i32]
        L.flex_order_rcm.argtypes = [C.POINTER(_Csr), vp]
        L.flex_order_cluster.argtypes = [C.POINTER(_Csr), vp]
        L.flex_order_gorder.argtypes = [C.POINTER(_Csr), u32, vp]
        L.flex_order_dfs.argtypes = [C.POINTER(_Csr), vp]
        L.flex_order_rabbit.argtypes = [C.POINTER(_Csr), i32, vp]
        L.flex_order_deg.argtypes = [C.POINTER(_Csr), i32, vp]
        L.flex_synth_preset.argtypes = [C.c_char_p, i32, C.POINTER(_SynthParams)]
        L.flex_perm_csr.argtypes = [C.POINTER(_Csr), vp, vp, vp, vp, vp]
        L.flex_shard_rows.argtypes = [C.POINTER(_Csr), i32, i32, vp]
        L.flex_synth_graph.argtypes = [C.POINTER(_SynthParams), C.POINTER(_HostCsr)]
        L.flex_strerror.argtypes = [i32]
        L.flex_strerror.restype = C.c_char_p
        L.flex_last_hip_error.restype = i32
        L.flex_last_hip_error_string.restype = C.c_char_p
        L.flex_abi_version.restype = i32
        L.flex_plan_softmax_info.argtypes = [vp, C.POINTER(_SoftmaxInfo)]
        L.flex_plan_attention_info.argtypes = [vp, C.POINTER(_AttentionInfo)]
        L.flex_plan_attention_backward_info.argtypes = [vp, C.POINTER(_AttentionBackwardInfo)]
        L.flex_plan_record_info.argtypes = [vp, C.POINTER(_RecordInfo)]
        L.flex_plan_read_records.argtypes = [vp, vp, i64]
        L.flex_plan_is_bf16.argtypes = [vp]
        L.flex_dropout_mask.argtypes = [C.c_uint64, C.c_float, C.c_uint64, C.c_uint64, vp]
        _lib = L
    return _lib


def _values_fn(name: str):
    """flex_plan_set_values / flex_sddmm / flex_edge_softmax / flex_edge_softmax_backward, the 22 fused-attention calls (flex_attention*,
    flex_gat_attention*), the three GATv2 calls (flex_gatv2_attention*), their two dropout forms (flex_dropout_gatv2_attention*) and flex_spmm_bf16, looked up at first use and not when the library loads: a host-only build without the kernel
    files does not have to define them.  tests/hostsim defines them all: the attention calls are the library's own entry points
    (csrc/attention_entry.h) on stand-in launchers that only log which kernel the real ones would launch, the others are stand-ins that
    log the same way."""
    L = lib()
    f = getattr(L, name)
    if f.argtypes is None:
        vp, fl, i32, u64 = C.c_void_p, C.c_float, C.c_int, C.c_uint64
        f.argtypes = {"flex_plan_set_values": [vp, vp, vp], "flex_sddmm": [vp, vp, vp, vp, vp], "flex_edge_softmax": [vp, vp, fl, vp, vp],
                      "flex_edge_softmax_backward": [vp, vp, vp, fl, vp, vp], "flex_attention": [vp, vp, vp, vp, fl, vp, vp, vp],
                      "flex_attention_backward": [vp, vp, vp, vp, vp, vp, fl, vp, vp, vp, vp, vp],
                      "flex_attention_heads": [vp, i32, vp, vp, vp, fl, vp, vp, vp],
                      "flex_attention_heads_backward": [vp, i32, vp, vp, vp, vp, vp, fl, vp, vp, vp, vp, vp],
                      "flex_attention_bf16": [vp, i32, vp, vp, vp, fl, vp, vp, vp],
                      "flex_attention_bf16_backward": [vp, i32, vp, vp, vp, vp, vp, fl, vp, vp, vp, vp, vp],
                      "flex_attention_bias": [vp, i32, vp, vp, vp, vp, fl, vp, vp, vp],
                      "flex_attention_bias_backward": [vp, i32, vp, vp, vp, vp, vp, fl, vp, vp, vp, vp, vp, vp],
                      "flex_attention_bf16_bias": [vp, i32, vp, vp, vp, vp, fl, vp, vp, vp],
                      "flex_attention_bf16_bias_backward": [vp, i32, vp, vp, vp, vp, vp, fl, vp, vp, vp, vp, vp, vp],
                      "flex_attention_dropout": [vp, i32, vp, vp, vp, vp, fl, fl, u64, vp, vp, vp],
                      "flex_attention_dropout_backward": [vp, i32, vp, vp, vp, vp, vp, fl, fl, u64, vp, vp, vp, vp, vp, vp],
                      "flex_attention_bf16_dropout": [vp, i32, vp, vp, vp, vp, fl, fl, u64, vp, vp, vp],
                      "flex_attention_bf16_dropout_backward": [vp, i32, vp, vp, vp, vp, vp, fl, fl, u64, vp, vp, vp, vp, vp, vp],
                      "flex_spmm_bf16": [vp, vp, vp, vp],
                      "flex_gat_attention": [vp, i32, vp, vp, vp, fl, vp, vp, vp],
                      "flex_gat_attention_backward": [vp, i32, vp, vp, vp, vp, vp, fl, vp, vp, vp, vp, vp],
                      "flex_gat_attention_dropout": [vp, i32, vp, vp, vp, fl, fl, u64, vp, vp, vp],
                      "flex_gat_attention_dropout_backward": [vp, i32, vp, vp, vp, vp, vp, fl, fl, u64, vp, vp, vp, vp, vp],
                      "flex_gat_attention_bf16": [vp, i32, vp, vp, vp, fl, vp, vp, vp],
                      "flex_gat_attention_bf16_backward": [vp, i32, vp, vp, vp, vp, vp, fl, vp, vp, vp, vp, vp],
                      "flex_gat_attention_bf16_dropout": [vp, i32, vp, vp, vp, fl, fl, u64, vp, vp, vp],
                      "flex_gat_attention_bf16_dropout_backward": [vp, i32, vp, vp, vp, vp, vp, fl, fl, u64, vp, vp, vp, vp, vp],
                      "flex_gatv2_attention": [vp, i32, vp, vp, vp, fl, vp, vp, vp],
                      "flex_gatv2_attention_backward": [vp, i32, vp, vp, vp, vp, vp, fl, vp, vp, vp, vp, vp, vp],
                      "flex_gatv2_attention_work_size": [vp, C.POINTER(u64)],
                      "flex_dropout_gatv2_attention": [vp, i32, vp, vp, vp, fl, fl, u64, vp, vp, vp],
                      "flex_dropout_gatv2_attention_backward": [vp, i32, vp, vp, vp, vp, vp, fl, fl, u64, vp, vp, vp, vp, vp, vp],
                      "flex_edge_gat_attention": [vp, i32, vp, vp, vp, vp, fl, fl, u64, vp, vp, vp],
                      "flex_edge_gat_attention_backward": [vp, i32, vp, vp, vp, vp, vp, vp, fl, fl, u64, vp, vp, vp, vp, vp, vp]}[name]
    return f


def _check(rc: int, what: str):
    if rc != 0:
        L = lib()
        msg = L.flex_strerror(rc).decode()
        if rc == -3:
            msg += f" [hip {L.flex_last_hip_error()}: {L.flex_last_hip_error_string().decode()}]"
        raise FlexError(f"{what}: {msg} ({rc})")


class HostCsr:
    """Host CSR (numpy, uint32 indices / float32 values) + the DataLoader statistics."""

    def __init__(self, rowPtr, col, vals, n=None, **stats):
        self.rowPtr = np.ascontiguousarray(rowPtr, dtype=np.uint32)
        self.col = np.ascontiguousarray(col, dtype=np.uint32)
        self.vals = np.ascontiguousarray(vals, dtype=np.float32)
        self.m = len(self.rowPtr) - 1
        self.n = self.m if n is None else int(n)
        self.nnz = len(self.col)
        self.__dict__.update(stats)

    def view(self) -> _Csr:
        return _Csr(self.m, self.n, self.nnz, self.rowPtr.ctypes.data, self.col.ctypes.data,
                    self.vals.ctypes.data)


def _take(s: _HostCsr) -> HostCsr:
    n = s.n
    try:
        rp = np.ctypeslib.as_array(s.rowPtr, shape=(s.m + 1,)).copy()
        col = np.ctypeslib.as_array(s.col, shape=(max(s.nnz, 1),))[: s.nnz].copy()
        vals = np.ctypeslib.as_array(s.vals, shape=(max(s.nnz, 1),))[: s.nnz].copy()
        stats = {k: getattr(s, k) for k in ("uni_nb", "n_edges_one_way", "n_edges_asymmetric",
                                           "n_nodes_z_out", "n_nodes_z_in", "n_nodes_z_deg",
                                           "is_directed", "c")}
    finally:
        lib().flex_host_csr_free(C.byref(s))
    return HostCsr(rp, col, vals, n=n, **stats)


def csv_load(path: str) -> HostCsr:
    s = _HostCsr()
    _check(lib().flex_csv_load(os.fsencode(path), C.byref(s)), f"flex_csv_load({path})")
    return _take(s)


def mtx_load(path: str, sort_columns: bool = True) -> HostCsr:
    s = _HostCsr()
    _check(lib().flex_mtx_load(os.fsencode(path), int(sort_columns), C.byref(s)), f"flex_mtx_load({path})")
    return _take(s)


def csv_save(path: str, a: HostCsr):
    v = a.view()
    _check(lib().flex_csv_save(os.fsencode(path), C.byref(v)), f"flex_csv_save({path})")


def csr_save_bin(path: str, a: HostCsr):
    v = a.view()
    _check(lib().flex_csr_save_bin(os.fsencode(path), C.byref(v)), f"flex_csr_save_bin({path})")


def csr_load_bin(path: str) -> HostCsr:
    s = _HostCsr()
    _check(lib().flex_csr_load_bin(os.fsencode(path), C.byref(s)), f"flex_csr_load_bin({path})")
    return _take(s)


def hbm_probe(device: int = 0, mib: int = 2048, reps: int = 10, temporal: bool = False) -> dict:
    """Measured GB/s of a read-only stream and of a copy (read + write bytes) on `device`."""
    r, c = C.c_double(), C.c_double()
    _check(lib().flex_hbm_probe(device, mib << 20, reps, int(temporal), C.byref(r), C.byref(c)), "flex_hbm_probe")
    return {"read_GBps": r.value, "copy_GBps": c.value}


def csr_fingerprint(a: HostCsr) -> int:
    v = a.view()
    return int(lib().flex_csr_fingerprint(C.byref(v)))


def perm_save(path: str, rank, fingerprint: int):
    r = np.ascontiguousarray(rank, dtype=np.uint32)
    _check(lib().flex_perm_save(os.fsencode(path), r.ctypes.data, len(r), fingerprint), f"flex_perm_save({path})")


def perm_load(path: str, n: int, fingerprint: int) -> np.ndarray:
    rank = np.empty(max(n, 1), dtype=np.uint32)
    _check(lib().flex_perm_load(os.fsencode(path), rank.ctypes.data, n, fingerprint), f"flex_perm_load({path})")
    return rank[:n]


def fill_dense_rand(n: int, k: int) -> np.ndarray:
    B = np.empty((n, k), dtype=np.float32)
    _check(lib().flex_fill_dense_rand(B.ctypes.data, n, k), "flex_fill_dense_rand")
    return B


def order_rcm(a: HostCsr) -> np.ndarray:
    rank = np.empty(max(a.m, 1), dtype=np.uint32)
    v = a.view()
    _check(lib().flex_order_rcm(C.byref(v), rank.ctypes.data), "flex_order_rcm")
    return rank[: a.m]


def order_cluster(a: HostCsr, **knobs) -> np.ndarray:
    """The engine's community order (agglomeration + vertex moves, cluster.cpp): rank[old] = new.
    knobs: fields of flex_cluster_tuning (batch, no_refine, stretch, sweeps, stride)."""
    rank = np.empty(max(a.m, 1), dtype=np.uint32)
    v = a.view()
    t = _ClusterTuning()
    for key, val in knobs.items():
        if key not in CLUSTER_TUNING_FIELDS:
            raise FlexError(f"unknown cluster knob {key!r}")
        setattr(t, key, int(val))
    _check(lib().flex_order_cluster_ex(C.byref(v), C.byref(t), rank.ctypes.data), "flex_order_cluster_ex")
    return rank[: a.m]


def set_host_threads(n: int) -> int:
    """Process-wide cap on the planner's / orderings' / generator's worker threads (0 = core count); returns the old value."""
    return int(lib().flex_set_host_threads(int(n)))


def perm_csr(a: HostCsr, rank: np.ndarray):
    """DataLoaderRcm body: returns (vo_mp, permuted HostCsr)."""
    rank = np.ascontiguousarray(rank, dtype=np.uint32)
    vo = np.empty(max(a.m, 1), dtype=np.int32)
    rp2 = np.empty(a.m + 1, dtype=np.uint32)
    c2 = np.empty(max(a.nnz, 1), dtype=np.uint32)
    v2 = np.empty(max(a.nnz, 1), dtype=np.float32)
    v = a.view()
    _check(lib().flex_perm_csr(C.byref(v), rank.ctypes.data, vo.ctypes.data, rp2.ctypes.data,
                               c2.ctypes.data, v2.ctypes.data), "flex_perm_csr")
    return vo[: a.m], HostCsr(rp2, c2[: a.nnz], v2[: a.nnz], n=a.n)


def shard_rows(a: HostCsr, k: int, nparts: int) -> np.ndarray:
    bounds = np.empty(nparts + 1, dtype=np.int64)
    v = a.view()
    _check(lib().flex_shard_rows(C.byref(v), k, nparts, bounds.ctypes.data), "flex_shard_rows")
    return bounds


SYNTH_PRESETS = ("amazon", "flickr", "ppi", "pubmed", "reddit", "soc-sign-epinions", "wiki-vote", "yelp")


def synth_preset(name: str, scale: int = 1) -> _SynthParams:
    """Generator parameters of the stand-in for a README / SuiteSparse graph (flex_synth_preset)."""
    p = _SynthParams()
    _check(lib().flex_synth_preset(name.lower().encode(), int(scale), C.byref(p)), f"flex_synth_preset({name})")
    return p


def synth_graph(name: str | None = None, *, scale: int = 1, n=None, nnz=None, alpha=2.1, community=0, p_in=0.0,
                p_near=0.0, near_window=8, shuffle=True, gcn_norm=True, directed=False, seed=0xF1E0) -> HostCsr:
    if name is not None:
        p = synth_preset(name, scale)
        p.shuffle = int(bool(shuffle))
    else:
        p = _SynthParams(int(n), int(nnz), float(alpha), int(community), float(p_in), float(p_near),
                         int(near_window), int(bool(shuffle)), int(bool(gcn_norm)), int(bool(directed)), int(seed))
    s = _HostCsr()
    _check(lib().flex_synth_graph(C.byref(p), C.byref(s)), f"flex_synth_graph({name or n})")
    return _take(s)


def order_gorder(a: HostCsr, window: int = 3) -> np.ndarray:
    rank = np.empty(max(a.m, 1), dtype=np.uint32)
    v = a.view()
    _check(lib().flex_order_gorder(C.byref(v), int(window), rank.ctypes.data), "flex_order_gorder")
    return rank[: a.m]


def order_dfs(a: HostCsr) -> np.ndarray:
    rank = np.empty(max(a.m, 1), dtype=np.uint32)
    v = a.view()
    _check(lib().flex_order_dfs(C.byref(v), rank.ctypes.data), "flex_order_dfs")
    return rank[: a.m]


def order_rabbit(a: HostCsr, is_directed: bool | None = None) -> np.ndarray:
    """flex_order_rabbit: the reference's Rabbit order (DataLoader.cu:455-655); is_directed defaults to the loader's statistic."""
    if is_directed is None:
        is_directed = bool(getattr(a, "is_directed", 0))
    rank = np.empty(max(a.m, 1), dtype=np.uint32)
    v = a.view()
    _check(lib().flex_order_rabbit(C.byref(v), int(bool(is_directed)), rank.ctypes.data), "flex_order_rabbit")
    return rank[: a.m]


def order_deg(a: HostCsr, descending: bool = True) -> np.ndarray:
    rank = np.empty(max(a.m, 1), dtype=np.uint32)
    v = a.view()
    _check(lib().flex_order_deg(C.byref(v), int(descending), rank.ctypes.data), "flex_order_deg")
    return rank[: a.m]


class Plan:
    """flex_plan handle (≙ Mat after csr2_DiagTiling + alpha_transfer)."""

    def __init__(self, a: HostCsr, k: int, device: int = 0, order: int = FLEX_ORDER_NATURAL,
                 vo_mp=None, rows=None, col_map=None, ldb: int | None = None, ldc: int | None = None, tuning: dict | None = None,
                 transpose: bool = False, mutable_values: bool = False, attention: bool = False, attention_backward: bool = False,
                 bf16: bool = False):
        """tuning: plan-time knobs as a dict of flex_plan_tuning fields (0 / absent = the planner's rule), e.g.
        {"lanes_per_nz": 16, "split_rows": 1, "cluster_no_refine": 1}.
        transpose: plan A^T (FLEX_PLAN_TRANSPOSE): C [a.n, k] = A^T B [a.m, k]; every other argument refers to A^T.
        mutable_values: FLEX_PLAN_MUTABLE_VALUES -- set_values() and sddmm() work on the plan; both index A's entries in a's CSR
        order, whatever the plan (transposed, mapped, a shard).
        attention: FLEX_PLAN_ATTENTION -- attention() works on the plan (not with transpose, vo_mp or col_map).
        attention_backward: FLEX_PLAN_ATTENTION_BACKWARD -- attention_backward() works on the plan too (needs attention; not with rows).
        bf16: FLEX_PLAN_BF16 -- B and C are bfloat16, sums fp32; the plan runs spmm_bf16() / plan(B) on bfloat16 tensors and nothing else
        (k, ldb, ldc multiples of 8; not with mutable_values, attention or autotune)."""
        self._h = C.c_void_p()
        self.src_nnz = a.nnz
        if transpose:
            order |= FLEX_PLAN_TRANSPOSE
        if mutable_values:
            order |= FLEX_PLAN_MUTABLE_VALUES
        if attention:
            order |= FLEX_PLAN_ATTENTION
        if attention_backward:
            order |= FLEX_PLAN_ATTENTION_BACKWARD
        if bf16:
            order |= FLEX_PLAN_BF16
        self._keep = (a, vo_mp, col_map)
        v = a.view()
        L = lib()
        tn = _tuning({**DEFAULT_TUNING, **(tuning or {})})
        if tn is not None or ((ldb is not None or ldc is not None) and (rows is not None or vo_mp is not None)):
            # a combination the named entry points do not cover: the general one
            cm = None if col_map is None else np.ascontiguousarray(col_map, dtype=np.int32)
            vm = None if vo_mp is None else np.ascontiguousarray(vo_mp, dtype=np.int32)
            self._keep = (a, cm, vm)
            d = _PlanDesc(C.sizeof(_PlanDesc), C.pointer(v), k, ldb or 0, ldc or 0, device,
                          order | (0 if rows is None else FLEX_PLAN_ROW_RANGE),
                          0 if rows is None else int(rows[0]), 0 if rows is None else int(rows[1]),
                          (cm if cm is not None else vm).ctypes.data if (cm is not None or vm is not None) else None,
                          None if vm is None else vm.ctypes.data, None if tn is None else C.pointer(tn))
            rc = L.flex_plan_create_ex(C.byref(self._h), C.byref(d))
        elif rows is not None:
            cm = None if col_map is None else np.ascontiguousarray(col_map, dtype=np.int32)
            self._keep = (a, cm)
            rc = L.flex_plan_create_rows(C.byref(self._h), C.byref(v), int(rows[0]), int(rows[1]),
                                         None if cm is None else cm.ctypes.data, k, device, order)
        elif vo_mp is not None:
            vm = np.ascontiguousarray(vo_mp, dtype=np.int32)
            rc = L.flex_plan_create_mapped(C.byref(self._h), C.byref(v), vm.ctypes.data, k, device, order)
        elif ldb is not None or ldc is not None:
            rc = L.flex_plan_create_ld(C.byref(self._h), C.byref(v), k, ldb or k, ldc or k, device, order)
        else:
            rc = L.flex_plan_create(C.byref(self._h), C.byref(v), k, device, order)
        _check(rc, "flex_plan_create")
        self.k = k
        self._keep = None  # the plan copies what it needs

    def info(self) -> dict:
        i = _PlanInfo()
        _check(lib().flex_plan_get_info(self._h, C.byref(i)), "flex_plan_get_info")
        d = {f: getattr(i, f) for f, _ in _PlanInfo._fields_}
        d["rec_packed"] = self.record_info()["packed"]
        d["bf16"] = int(lib().flex_plan_is_bf16(self._h))  # 1: k above counts bfloat16 elements and the plan runs spmm_bf16()
        return d

    def record_info(self) -> dict:
        """flex_plan_record_info: how the record stream is stored (packed, records, wide_records, exceptions, stream_bytes)."""
        ri = _RecordInfo()
        _check(lib().flex_plan_record_info(self._h, C.byref(ri)), "flex_plan_record_info")
        return {f: getattr(ri, f) for f, _ in _RecordInfo._fields_ if f != "reserved"}

    def records(self) -> np.ndarray:
        """flex_plan_read_records: the record stream read back from the device image, decoded where it is packed: uint32 [n_records, 2] =
        {B-row byte offset or column id, value bits}."""
        n = self.record_info()["records"]
        out = np.empty((max(n, 1), 2), dtype=np.uint32)
        _check(lib().flex_plan_read_records(self._h, out.ctypes.data, n), "flex_plan_read_records")
        return out[:n]

    def stats(self) -> dict:
        """flex_plan_stats (≙ alpha_stats_collect + B-Re1/B-Re2); the plan must be made with FLEX_PLAN_STATS."""
        st = _PlanStats()
        _check(lib().flex_plan_get_stats(self._h, C.byref(st)), "flex_plan_get_stats")
        return {f: getattr(st, f) for f, _ in _PlanStats._fields_}

    def tuning(self) -> dict:
        """flex_plan_get_tuning: the knobs this plan was built with, rules resolved."""
        t = _PlanTuning()
        _check(lib().flex_plan_get_tuning(self._h, C.byref(t)), "flex_plan_get_tuning")
        d = {f: getattr(t, f) for f in TUNING_FIELDS}
        d.update({"cluster_" + f: getattr(t.cluster, f) for f in CLUSTER_TUNING_FIELDS})
        return d

    def kernel_info(self) -> dict:
        ki = _KernelInfo()
        _check(lib().flex_plan_kernel_info(self._h, C.byref(ki)), "flex_plan_kernel_info")
        return {f: getattr(ki, f) for f, _ in _KernelInfo._fields_}

    def measure_imbalance(self, dB_ptr: int, dC_ptr: int, stream: int = 0) -> dict:
        """flex_plan_measure_imbalance (≙ the per-SM "Imb" column, flex.cu:5087-5126): one stamped launch, per-CU / per-XCD busy imbalance."""
        im = _Imbalance()
        _check(lib().flex_plan_measure_imbalance(self._h, dB_ptr, dC_ptr, stream, C.byref(im)), "flex_plan_measure_imbalance")
        return {f: getattr(im, f) for f, _ in _Imbalance._fields_}

    def self_check(self):
        """flex_plan_self_check: the device image of the plan is a partition of the work (raises FlexError if not)."""
        _check(lib().flex_plan_self_check(self._h), "flex_plan_self_check")

    def spmm(self, dB_ptr: int, dC_ptr: int, stream: int = 0):
        _check(lib().flex_spmm(self._h, dB_ptr, dC_ptr, stream), "flex_spmm")

    def spmm_bf16(self, dB_ptr: int, dC_ptr: int, stream: int = 0):
        """flex_spmm_bf16 (bf16=True plans only): dB, dC device pointers to bfloat16 rows, both 16-byte aligned."""
        _check(_values_fn("flex_spmm_bf16")(self._h, dB_ptr, dC_ptr, stream), "flex_spmm_bf16")

    def __call__(self, B, out=None):
        """torch convenience: B is a cuda [n,k] tensor, float32 -- bfloat16 on a bf16 plan (TypeError on the other); returns C [m,k] of
        the same dtype."""
        import torch
        i = self.info()
        want = torch.bfloat16 if i["bf16"] else torch.float32
        if B.dtype != want:
            raise TypeError(f"this plan takes {want} operands, got {B.dtype}")
        assert B.is_cuda and B.is_contiguous() and tuple(B.shape) == (i["n"], i["k"])
        if out is None:
            out = torch.empty((i["m"], i["k"]), dtype=want, device=B.device)
        elif out.dtype != want:
            raise TypeError(f"this plan writes {want}, out is {out.dtype}")
        run = self.spmm_bf16 if i["bf16"] else self.spmm
        run(B.data_ptr(), out.data_ptr(), torch.cuda.current_stream(B.device).cuda_stream)
        return out

    def set_values(self, vals, stream: int | None = None):
        """flex_plan_set_values: vals is a float32 cuda tensor of a.nnz values in the CSR order of the `a` the plan was made from.
        Stream-ordered (torch's current stream by default): launches of the plan queued before it read the old values."""
        import torch
        assert vals.is_cuda and vals.dtype == torch.float32 and vals.is_contiguous() and vals.numel() == self.src_nnz, "float32 cuda [nnz]"
        s = torch.cuda.current_stream(vals.device).cuda_stream if stream is None else stream
        _check(_values_fn("flex_plan_set_values")(self._h, vals.data_ptr(), s), "flex_plan_set_values")

    def sddmm_ptr(self, dG_ptr: int, dB_ptr: int, dOut_ptr: int, stream: int = 0):
        _check(_values_fn("flex_sddmm")(self._h, dG_ptr, dB_ptr, dOut_ptr, stream), "flex_sddmm")

    def sddmm(self, G, B, out=None):
        """flex_sddmm: out[e] = <G[dst(e)], B[src(e)]> for the entries e the plan holds (the gradient of C = A(v) B with respect to v),
        a float32 cuda tensor [a.nnz] in a's CSR order.  G: [m, k] like C, B: [n, k] like B.  Entries the plan does not hold (other
        shards) keep what `out` held; a new `out` starts at zero."""
        import torch
        i = self.info()
        assert G.is_cuda and G.dtype == torch.float32 and G.is_contiguous() and tuple(G.shape) == (i["m"], i["k"])
        assert B.is_cuda and B.dtype == torch.float32 and B.is_contiguous() and tuple(B.shape) == (i["n"], i["k"])
        if out is None:
            out = torch.zeros(self.src_nnz, dtype=torch.float32, device=G.device)
        assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == self.src_nnz
        self.sddmm_ptr(G.data_ptr(), B.data_ptr(), out.data_ptr(), torch.cuda.current_stream(G.device).cuda_stream)
        return out

    def softmax_info(self) -> dict:
        """flex_plan_softmax_info: the schedule of edge_softmax on this plan (rows, entries, items, groups, rows by class)."""
        i = _SoftmaxInfo()
        _check(lib().flex_plan_softmax_info(self._h, C.byref(i)), "flex_plan_softmax_info")
        return {f: getattr(i, f) for f, _ in _SoftmaxInfo._fields_}

    def edge_softmax_ptr(self, dScores_ptr: int, scale: float, dOut_ptr: int, stream: int = 0):
        _check(_values_fn("flex_edge_softmax")(self._h, dScores_ptr, scale, dOut_ptr, stream), "flex_edge_softmax")

    def edge_softmax_backward_ptr(self, dP_ptr: int, dGradP_ptr: int, scale: float, dGradS_ptr: int, stream: int = 0):
        _check(_values_fn("flex_edge_softmax_backward")(self._h, dP_ptr, dGradP_ptr, scale, dGradS_ptr, stream), "flex_edge_softmax_backward")

    def _edge_vectors(self, *ts):
        import torch
        for t in ts:
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == self.src_nnz, "float32 cuda [nnz]"

    def edge_softmax(self, s, scale: float = 1.0, out=None):
        """flex_edge_softmax: the softmax of scale * s over each row of `a`; s and the result are float32 cuda tensors [a.nnz] in a's CSR
        order (out=s: in place).  -inf scores are masked edges (p = +0).  Entries the plan does not hold (other shards) keep what `out`
        held; a new `out` starts at zero."""
        import torch
        if out is None:
            out = torch.zeros_like(s)
        self._edge_vectors(s, out)
        self.edge_softmax_ptr(s.data_ptr(), scale, out.data_ptr(), torch.cuda.current_stream(s.device).cuda_stream)
        return out

    def edge_softmax_backward(self, p, gp, scale: float = 1.0, out=None):
        """flex_edge_softmax_backward: scale * p * (gp - sum over the row of p * gp), p the forward's output (out=gp: in place)."""
        import torch
        if out is None:
            out = torch.zeros_like(gp)
        self._edge_vectors(p, gp, out)
        self.edge_softmax_backward_ptr(p.data_ptr(), gp.data_ptr(), scale, out.data_ptr(), torch.cuda.current_stream(p.device).cuda_stream)
        return out

    def attention_info(self) -> dict:
        """flex_plan_attention_info: the schedule of attention() on this plan (rows, entries, items, groups, rows by class)."""
        i = _AttentionInfo()
        _check(lib().flex_plan_attention_info(self._h, C.byref(i)), "flex_plan_attention_info")
        return {f: getattr(i, f) for f, _ in _AttentionInfo._fields_}

    def attention_ptr(self, dQ_ptr: int, dK_ptr: int, dV_ptr: int, scale: float, dOut_ptr: int, dP_ptr: int | None = None, stream: int = 0,
                      heads: int | None = None):
        """heads=None: flex_attention.  heads=H (1 included): flex_attention_heads with that H; dP is then nnz x H floats, entry-major."""
        if heads is None:
            _check(_values_fn("flex_attention")(self._h, dQ_ptr, dK_ptr, dV_ptr, scale, dOut_ptr, dP_ptr, stream), "flex_attention")
        else:
            _check(_values_fn("flex_attention_heads")(self._h, heads, dQ_ptr, dK_ptr, dV_ptr, scale, dOut_ptr, dP_ptr, stream), "flex_attention_heads")

    def _head_edge_arrays(self, heads, *ts):
        """The edge arrays of the per-head calls (heads, bf16, bias and GAT): float32 cuda [nnz, heads], heads = 1 included."""
        import torch
        for t in ts:
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (self.src_nnz, heads), "float32 cuda [nnz, heads]"

    def _edge_arrays(self, heads, *ts):
        if heads == 1:
            self._edge_vectors(*ts)
        else:
            self._head_edge_arrays(heads, *ts)

    def attention(self, Q, K, V, scale: float, out=None, p=None, heads: int = 1):
        """flex_attention: out [m, k] = sum over each row's entries of alpha V[col], alpha = the softmax over the row of
        scale * <Q[row], K[col]>, in one launch.  Q: [m, k] like C; K, V: [n, k] like B; float32 cuda tensors.  p (optional): a float32
        cuda tensor [a.nnz] that receives alpha in a's CSR order for the plan's rows (entries of other shards keep what it held).
        heads > 1 (flex_attention_heads): head h is columns [h k / heads, (h + 1) k / heads) and has its own softmax, still in one launch;
        p is then [a.nnz, heads]."""
        import torch
        i = self.info()
        for t, rows in ((Q, i["m"]), (K, i["n"]), (V, i["n"])):
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (rows, i["k"])
        if out is None:  # every row is written, except by a plan without entries, which launches nothing
            out = (torch.empty if i["nnz"] else torch.zeros)((i["m"], i["k"]), dtype=torch.float32, device=Q.device)
        assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (i["m"], i["k"])
        if p is not None:
            self._edge_arrays(heads, p)
        self.attention_ptr(Q.data_ptr(), K.data_ptr(), V.data_ptr(), scale, out.data_ptr(), None if p is None else p.data_ptr(),
                           torch.cuda.current_stream(Q.device).cuda_stream, heads=None if heads == 1 else heads)
        return out

    def attention_backward_info(self) -> dict:
        """flex_plan_attention_backward_info: the schedule of attention_backward()'s column launch (columns, entries, items, groups, columns by class)."""
        i = _AttentionBackwardInfo()
        _check(lib().flex_plan_attention_backward_info(self._h, C.byref(i)), "flex_plan_attention_backward_info")
        return {f: getattr(i, f) for f, _ in _AttentionBackwardInfo._fields_}

    def attention_backward_ptr(self, dQ_ptr: int, dK_ptr: int, dV_ptr: int, dP_ptr: int, dGradOut_ptr: int, scale: float, dGradQ_ptr: int | None,
                               dGradK_ptr: int | None, dGradV_ptr: int | None, dWork_ptr: int, stream: int = 0, heads: int | None = None):
        """heads=None: flex_attention_backward.  heads=H (1 included): flex_attention_heads_backward with that H; dP and dWork are then
        nnz x H floats, entry-major."""
        if heads is None:
            _check(_values_fn("flex_attention_backward")(self._h, dQ_ptr, dK_ptr, dV_ptr, dP_ptr, dGradOut_ptr, scale, dGradQ_ptr, dGradK_ptr, dGradV_ptr,
                                                         dWork_ptr, stream), "flex_attention_backward")
        else:
            _check(_values_fn("flex_attention_heads_backward")(self._h, heads, dQ_ptr, dK_ptr, dV_ptr, dP_ptr, dGradOut_ptr, scale, dGradQ_ptr, dGradK_ptr,
                                                               dGradV_ptr, dWork_ptr, stream), "flex_attention_heads_backward")

    def attention_backward(self, Q, K, V, p, grad_out, scale: float, grad_q=None, grad_k=None, grad_v=None, work=None, want=(True, True, True),
                           heads: int = 1):
        """flex_attention_backward: (gQ [m, k], gK [n, k], gV [n, k]) of attention()'s out from its p and grad_out [m, k], in two launches; an
        output that `want` does not ask for is None and is not computed.  work (optional): a float32 cuda tensor [a.nnz], not p, that
        receives the gradient in the scores whenever gQ or gK is wanted.  heads > 1 (flex_attention_heads_backward): the backward of
        attention(..., heads=heads); p and work are [a.nnz, heads]."""
        import torch
        i = self.info()
        for t, rows in ((Q, i["m"]), (K, i["n"]), (V, i["n"]), (grad_out, i["m"])):
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (rows, i["k"])
        if work is None:
            work = torch.empty(self.src_nnz if heads == 1 else (self.src_nnz, heads), dtype=torch.float32, device=Q.device)
        self._edge_arrays(heads, p, work)
        outs = []
        for wanted, t, rows in zip(want, (grad_q, grad_k, grad_v), (i["m"], i["n"], i["n"])):
            if wanted and t is None:  # every row is written, except by a plan without entries, which launches nothing
                t = (torch.empty if i["nnz"] else torch.zeros)((rows, i["k"]), dtype=torch.float32, device=Q.device)
            if wanted:
                assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (rows, i["k"])
            outs.append(t if wanted else None)
        self.attention_backward_ptr(Q.data_ptr(), K.data_ptr(), V.data_ptr(), p.data_ptr(), grad_out.data_ptr(), scale,
                                    *(None if t is None else t.data_ptr() for t in outs), work.data_ptr(),
                                    torch.cuda.current_stream(Q.device).cuda_stream, heads=None if heads == 1 else heads)
        return tuple(outs)

    def attention_bf16_ptr(self, dQ_ptr: int, dK_ptr: int, dV_ptr: int, scale: float, dOut_ptr: int, dP_ptr: int | None = None, stream: int = 0,
                           heads: int = 1):
        """flex_attention_bf16: Q, K, V and Out are bf16 rows, dP (optional) is nnz x H floats, entry-major."""
        _check(_values_fn("flex_attention_bf16")(self._h, heads, dQ_ptr, dK_ptr, dV_ptr, scale, dOut_ptr, dP_ptr, stream), "flex_attention_bf16")

    def attention_bf16(self, Q, K, V, scale: float, heads: int = 1, out=None, p=None):
        """flex_attention_bf16: attention(..., heads=heads) on torch.bfloat16 cuda tensors Q [m, k], K, V [n, k]; scores, softmax and sums
        in float32, out [m, k] bfloat16 rounded once at its store.  p (optional): a float32 cuda tensor [a.nnz, heads] that receives alpha,
        not rounded.  heads = 1 runs here too: k / heads is a power of two in 4 .. 256 for every heads."""
        import torch
        i = self.info()
        for t, rows in ((Q, i["m"]), (K, i["n"]), (V, i["n"])):
            assert t.is_cuda and t.dtype == torch.bfloat16 and t.is_contiguous() and tuple(t.shape) == (rows, i["k"]), "bfloat16 cuda [rows, k]"
        if out is None:  # every row is written, except by a plan without entries, which launches nothing
            out = (torch.empty if i["nnz"] else torch.zeros)((i["m"], i["k"]), dtype=torch.bfloat16, device=Q.device)
        assert out.is_cuda and out.dtype == torch.bfloat16 and out.is_contiguous() and tuple(out.shape) == (i["m"], i["k"])
        if p is not None:
            self._head_edge_arrays(heads, p)
        self.attention_bf16_ptr(Q.data_ptr(), K.data_ptr(), V.data_ptr(), scale, out.data_ptr(), None if p is None else p.data_ptr(),
                                torch.cuda.current_stream(Q.device).cuda_stream, heads=heads)
        return out

    def attention_bf16_backward_ptr(self, dQ_ptr: int, dK_ptr: int, dV_ptr: int, dP_ptr: int, dGradOut_ptr: int, scale: float, dGradQ_ptr: int | None,
                                    dGradK_ptr: int | None, dGradV_ptr: int | None, dWork_ptr: int, stream: int = 0, heads: int = 1):
        """flex_attention_bf16_backward: the row operands and the gradients are bf16 rows, dP and dWork nnz x H floats, entry-major."""
        _check(_values_fn("flex_attention_bf16_backward")(self._h, heads, dQ_ptr, dK_ptr, dV_ptr, dP_ptr, dGradOut_ptr, scale, dGradQ_ptr, dGradK_ptr,
                                                          dGradV_ptr, dWork_ptr, stream), "flex_attention_bf16_backward")

    def attention_bf16_backward(self, Q, K, V, p, grad_out, scale: float, heads: int = 1, grad_q=None, grad_k=None, grad_v=None, work=None,
                                want=(True, True, True)):
        """flex_attention_bf16_backward: (gQ [m, k], gK [n, k], gV [n, k]) in bfloat16 of attention_bf16()'s out from its p [a.nnz, heads]
        (float32) and grad_out [m, k] (bfloat16), in two launches; an output that `want` does not ask for is None and is not computed.
        work (optional): a float32 cuda tensor [a.nnz, heads], not p, that receives the gradient in the scores whenever gQ or gK is wanted."""
        import torch
        i = self.info()
        for t, rows in ((Q, i["m"]), (K, i["n"]), (V, i["n"]), (grad_out, i["m"])):
            assert t.is_cuda and t.dtype == torch.bfloat16 and t.is_contiguous() and tuple(t.shape) == (rows, i["k"]), "bfloat16 cuda [rows, k]"
        if work is None:
            work = torch.empty((self.src_nnz, heads), dtype=torch.float32, device=Q.device)
        self._head_edge_arrays(heads, p, work)
        outs = []
        for wanted, t, rows in zip(want, (grad_q, grad_k, grad_v), (i["m"], i["n"], i["n"])):
            if wanted and t is None:  # every row is written, except by a plan without entries, which launches nothing
                t = (torch.empty if i["nnz"] else torch.zeros)((rows, i["k"]), dtype=torch.bfloat16, device=Q.device)
            if wanted:
                assert t.is_cuda and t.dtype == torch.bfloat16 and t.is_contiguous() and tuple(t.shape) == (rows, i["k"])
            outs.append(t if wanted else None)
        self.attention_bf16_backward_ptr(Q.data_ptr(), K.data_ptr(), V.data_ptr(), p.data_ptr(), grad_out.data_ptr(), scale,
                                         *(None if t is None else t.data_ptr() for t in outs), work.data_ptr(),
                                         torch.cuda.current_stream(Q.device).cuda_stream, heads=heads)
        return tuple(outs)

    def attention_bias_ptr(self, dQ_ptr: int, dK_ptr: int, dV_ptr: int, dBias_ptr: int, scale: float, dOut_ptr: int, dP_ptr: int | None = None,
                           stream: int = 0, heads: int = 1):
        """flex_attention_bias: fp32 rows; dBias and dP (optional) are nnz x H floats, entry-major."""
        _check(_values_fn("flex_attention_bias")(self._h, heads, dQ_ptr, dK_ptr, dV_ptr, dBias_ptr, scale, dOut_ptr, dP_ptr, stream), "flex_attention_bias")

    def attention_bf16_bias_ptr(self, dQ_ptr: int, dK_ptr: int, dV_ptr: int, dBias_ptr: int, scale: float, dOut_ptr: int, dP_ptr: int | None = None,
                                stream: int = 0, heads: int = 1):
        """flex_attention_bf16_bias: Q, K, V and Out are bf16 rows; dBias and dP (optional) are nnz x H floats, entry-major."""
        _check(_values_fn("flex_attention_bf16_bias")(self._h, heads, dQ_ptr, dK_ptr, dV_ptr, dBias_ptr, scale, dOut_ptr, dP_ptr, stream),
               "flex_attention_bf16_bias")

    def attention_bias_backward_ptr(self, dQ_ptr: int, dK_ptr: int, dV_ptr: int, dP_ptr: int, dGradOut_ptr: int, scale: float, dGradQ_ptr: int | None,
                                    dGradK_ptr: int | None, dGradV_ptr: int | None, dGradBias_ptr: int | None, dWork_ptr: int, stream: int = 0,
                                    heads: int = 1):
        """flex_attention_bias_backward: fp32 rows; dP, dGradBias and dWork are nnz x H floats, entry-major."""
        _check(_values_fn("flex_attention_bias_backward")(self._h, heads, dQ_ptr, dK_ptr, dV_ptr, dP_ptr, dGradOut_ptr, scale, dGradQ_ptr, dGradK_ptr,
                                                          dGradV_ptr, dGradBias_ptr, dWork_ptr, stream), "flex_attention_bias_backward")

    def attention_bf16_bias_backward_ptr(self, dQ_ptr: int, dK_ptr: int, dV_ptr: int, dP_ptr: int, dGradOut_ptr: int, scale: float,
                                         dGradQ_ptr: int | None, dGradK_ptr: int | None, dGradV_ptr: int | None, dGradBias_ptr: int | None,
                                         dWork_ptr: int, stream: int = 0, heads: int = 1):
        """flex_attention_bf16_bias_backward: the row operands and gQ, gK, gV are bf16 rows; dP, dGradBias and dWork nnz x H floats."""
        _check(_values_fn("flex_attention_bf16_bias_backward")(self._h, heads, dQ_ptr, dK_ptr, dV_ptr, dP_ptr, dGradOut_ptr, scale, dGradQ_ptr,
                                                               dGradK_ptr, dGradV_ptr, dGradBias_ptr, dWork_ptr, stream),
               "flex_attention_bf16_bias_backward")

    def _attention_bias(self, dtype, run, Q, K, V, bias, scale, heads, out, p):
        import torch
        i = self.info()
        for t, rows in ((Q, i["m"]), (K, i["n"]), (V, i["n"])):
            assert t.is_cuda and t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == (rows, i["k"]), f"{dtype} cuda [rows, k]"
        if heads == 1 and bias.dim() == 1:
            bias = bias.unsqueeze(1)
        self._head_edge_arrays(heads, bias)
        if out is None:  # every row is written, except by a plan without entries, which launches nothing
            out = (torch.empty if i["nnz"] else torch.zeros)((i["m"], i["k"]), dtype=dtype, device=Q.device)
        assert out.is_cuda and out.dtype == dtype and out.is_contiguous() and tuple(out.shape) == (i["m"], i["k"])
        if p is not None:
            self._head_edge_arrays(heads, p)
        run(Q.data_ptr(), K.data_ptr(), V.data_ptr(), bias.data_ptr(), scale, out.data_ptr(), None if p is None else p.data_ptr(),
            torch.cuda.current_stream(Q.device).cuda_stream, heads=heads)
        return out

    def _attention_bias_backward(self, dtype, run, Q, K, V, p, grad_out, scale, heads, grads, work, want):
        import torch
        i = self.info()
        for t, rows in ((Q, i["m"]), (K, i["n"]), (V, i["n"]), (grad_out, i["m"])):
            assert t.is_cuda and t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == (rows, i["k"]), f"{dtype} cuda [rows, k]"
        if work is None:
            work = torch.empty((self.src_nnz, heads), dtype=torch.float32, device=Q.device)
        self._head_edge_arrays(heads, p, work)
        shapes = ((i["m"], i["k"]), (i["n"], i["k"]), (i["n"], i["k"]), (self.src_nnz, heads))
        outs = []
        for wanted, t, shape, dt in zip(want, grads, shapes, (dtype, dtype, dtype, torch.float32)):
            if wanted and t is None:  # every element is written, except by a plan without entries, which launches nothing
                t = (torch.empty if i["nnz"] else torch.zeros)(shape, dtype=dt, device=Q.device)
            if wanted:
                assert t.is_cuda and t.dtype == dt and t.is_contiguous() and tuple(t.shape) == shape
            outs.append(t if wanted else None)
        run(Q.data_ptr(), K.data_ptr(), V.data_ptr(), p.data_ptr(), grad_out.data_ptr(), scale, *(None if t is None else t.data_ptr() for t in outs),
            work.data_ptr(), torch.cuda.current_stream(Q.device).cuda_stream, heads=heads)
        return tuple(outs)

    def attention_bias(self, Q, K, V, bias, scale: float, heads: int = 1, out=None, p=None):
        """flex_attention_bias: attention(..., heads=heads) with bias [a.nnz, heads] (float32 cuda, a's CSR order; [a.nnz] is taken as
        [a.nnz, 1] when heads == 1) added to the scaled score of every entry and head before the softmax; -inf masks an entry for a head.
        Q [m, k], K, V [n, k] float32; p (optional): a float32 cuda tensor [a.nnz, heads] that receives alpha.  heads = 1 runs here too:
        k / heads is a power of two in 4 .. 256 for every heads."""
        import torch
        return self._attention_bias(torch.float32, self.attention_bias_ptr, Q, K, V, bias, scale, heads, out, p)

    def attention_bf16_bias(self, Q, K, V, bias, scale: float, heads: int = 1, out=None, p=None):
        """flex_attention_bf16_bias: attention_bias() on torch.bfloat16 Q, K, V; out is bfloat16, rounded once at its store; bias and p
        stay float32 and are not rounded."""
        import torch
        return self._attention_bias(torch.bfloat16, self.attention_bf16_bias_ptr, Q, K, V, bias, scale, heads, out, p)

    def attention_bias_backward(self, Q, K, V, p, grad_out, scale: float, heads: int = 1, grad_q=None, grad_k=None, grad_v=None, grad_bias=None,
                                work=None, want=(True, True, True, True)):
        """flex_attention_bias_backward: (gQ [m, k], gK [n, k], gV [n, k], gBias [a.nnz, heads]) of attention_bias()'s out from its p
        [a.nnz, heads] and grad_out [m, k], in two launches; it does not take the bias.  An output that `want` does not ask for is None
        and is not computed.  work (optional): a float32 cuda tensor [a.nnz, heads], neither p nor grad_bias, that receives the gradient
        in the scores whenever gQ, gK or gBias is wanted."""
        import torch
        return self._attention_bias_backward(torch.float32, self.attention_bias_backward_ptr, Q, K, V, p, grad_out, scale, heads,
                                             (grad_q, grad_k, grad_v, grad_bias), work, want)

    def attention_bf16_bias_backward(self, Q, K, V, p, grad_out, scale: float, heads: int = 1, grad_q=None, grad_k=None, grad_v=None,
                                     grad_bias=None, work=None, want=(True, True, True, True)):
        """flex_attention_bf16_bias_backward: attention_bias_backward() on torch.bfloat16 Q, K, V and grad_out; gQ, gK and gV are bfloat16,
        p, gBias and work float32."""
        import torch
        return self._attention_bias_backward(torch.bfloat16, self.attention_bf16_bias_backward_ptr, Q, K, V, p, grad_out, scale, heads,
                                             (grad_q, grad_k, grad_v, grad_bias), work, want)

    def attention_dropout_ptr(self, dQ_ptr: int, dK_ptr: int, dV_ptr: int, dBias_ptr: int | None, scale: float, p: float, seed: int, dOut_ptr: int,
                              dP_ptr: int | None = None, stream: int = 0, heads: int = 1):
        """flex_attention_dropout: fp32 rows; dBias (None: no bias) and dP (optional) are nnz x H floats, entry-major; dP receives the
        UNDROPPED probabilities.  p: the dropout probability, 0 <= p < 1; seed: 64 bits."""
        _check(_values_fn("flex_attention_dropout")(self._h, heads, dQ_ptr, dK_ptr, dV_ptr, dBias_ptr, scale, p, seed, dOut_ptr, dP_ptr, stream),
               "flex_attention_dropout")

    def attention_bf16_dropout_ptr(self, dQ_ptr: int, dK_ptr: int, dV_ptr: int, dBias_ptr: int | None, scale: float, p: float, seed: int,
                                   dOut_ptr: int, dP_ptr: int | None = None, stream: int = 0, heads: int = 1):
        """flex_attention_bf16_dropout: attention_dropout_ptr on bf16 rows (Q, K, V, Out)."""
        _check(_values_fn("flex_attention_bf16_dropout")(self._h, heads, dQ_ptr, dK_ptr, dV_ptr, dBias_ptr, scale, p, seed, dOut_ptr, dP_ptr, stream),
               "flex_attention_bf16_dropout")

    def attention_dropout_backward_ptr(self, dQ_ptr: int, dK_ptr: int, dV_ptr: int, dP_ptr: int, dGradOut_ptr: int, scale: float, p: float, seed: int,
                                       dGradQ_ptr: int | None, dGradK_ptr: int | None, dGradV_ptr: int | None, dGradBias_ptr: int | None,
                                       dWork_ptr: int, stream: int = 0, heads: int = 1):
        """flex_attention_dropout_backward: fp32 rows; dP, dGradBias (None: not wanted) and dWork are nnz x H floats, entry-major."""
        _check(_values_fn("flex_attention_dropout_backward")(self._h, heads, dQ_ptr, dK_ptr, dV_ptr, dP_ptr, dGradOut_ptr, scale, p, seed, dGradQ_ptr,
                                                             dGradK_ptr, dGradV_ptr, dGradBias_ptr, dWork_ptr, stream), "flex_attention_dropout_backward")

    def attention_bf16_dropout_backward_ptr(self, dQ_ptr: int, dK_ptr: int, dV_ptr: int, dP_ptr: int, dGradOut_ptr: int, scale: float, p: float,
                                            seed: int, dGradQ_ptr: int | None, dGradK_ptr: int | None, dGradV_ptr: int | None,
                                            dGradBias_ptr: int | None, dWork_ptr: int, stream: int = 0, heads: int = 1):
        """flex_attention_bf16_dropout_backward: attention_dropout_backward_ptr on bf16 rows (Q, K, V, g, gQ, gK, gV)."""
        _check(_values_fn("flex_attention_bf16_dropout_backward")(self._h, heads, dQ_ptr, dK_ptr, dV_ptr, dP_ptr, dGradOut_ptr, scale, p, seed,
                                                                  dGradQ_ptr, dGradK_ptr, dGradV_ptr, dGradBias_ptr, dWork_ptr, stream),
               "flex_attention_bf16_dropout_backward")

    def _attention_dropout(self, dtype, run, Q, K, V, scale, p, seed, heads, bias, out, probs):
        import torch
        i = self.info()
        for t, rows in ((Q, i["m"]), (K, i["n"]), (V, i["n"])):
            assert t.is_cuda and t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == (rows, i["k"]), f"{dtype} cuda [rows, k]"
        if bias is not None:
            if heads == 1 and bias.dim() == 1:
                bias = bias.unsqueeze(1)
            self._head_edge_arrays(heads, bias)
        if out is None:  # every row is written, except by a plan without entries, which launches nothing
            out = (torch.empty if i["nnz"] else torch.zeros)((i["m"], i["k"]), dtype=dtype, device=Q.device)
        assert out.is_cuda and out.dtype == dtype and out.is_contiguous() and tuple(out.shape) == (i["m"], i["k"])
        if probs is not None:
            self._head_edge_arrays(heads, probs)
        run(Q.data_ptr(), K.data_ptr(), V.data_ptr(), None if bias is None else bias.data_ptr(), scale, p, seed, out.data_ptr(),
            None if probs is None else probs.data_ptr(), torch.cuda.current_stream(Q.device).cuda_stream, heads=heads)
        return out

    def attention_dropout(self, Q, K, V, scale: float, p: float, seed: int, heads: int = 1, bias=None, out=None, probs=None):
        """flex_attention_dropout: attention(..., heads=heads) (attention_bias() with bias [a.nnz, heads]) whose probabilities are dropped
        with probability p after the softmax and the kept ones scaled by 1 / (1 - p), in the same one launch.  The mask is
        dropout_mask(seed, p, e * heads + h, 1) for entry e and head h.  probs (optional): a float32 cuda tensor [a.nnz, heads] that
        receives the UNDROPPED alpha, which attention_dropout_backward() starts from.  heads = 1 runs here too: k / heads is a power of
        two in 4 .. 256 for every heads.  p = 0 is the undropped call, bit for bit."""
        import torch
        return self._attention_dropout(torch.float32, self.attention_dropout_ptr, Q, K, V, scale, p, seed, heads, bias, out, probs)

    def attention_bf16_dropout(self, Q, K, V, scale: float, p: float, seed: int, heads: int = 1, bias=None, out=None, probs=None):
        """flex_attention_bf16_dropout: attention_dropout() on torch.bfloat16 Q, K, V; out is bfloat16, rounded once at its store; bias and
        probs stay float32."""
        import torch
        return self._attention_dropout(torch.bfloat16, self.attention_bf16_dropout_ptr, Q, K, V, scale, p, seed, heads, bias, out, probs)

    def _attention_dropout_backward(self, dtype, run, Q, K, V, probs, grad_out, scale, p, seed, heads, grads, work, want):
        import torch
        if len(want) == 3:
            want = (*want, False)
        return self._attention_bias_backward(dtype, lambda q, k, v, pr, g, sc, *rest, heads: run(q, k, v, pr, g, sc, p, seed, *rest, heads=heads),
                                             Q, K, V, probs, grad_out, scale, heads, grads, work, want)

    def attention_dropout_backward(self, Q, K, V, probs, grad_out, scale: float, p: float, seed: int, heads: int = 1, grad_q=None, grad_k=None,
                                   grad_v=None, grad_bias=None, work=None, want=(True, True, True, False)):
        """flex_attention_dropout_backward: (gQ [m, k], gK [n, k], gV [n, k], gBias [a.nnz, heads]) of attention_dropout()'s out from its
        probs [a.nnz, heads] and grad_out [m, k] under the same p and seed, in two launches.  An output that `want` does not ask for is
        None and is not computed (gBias: only where the forward had a bias).  work (optional): a float32 cuda tensor [a.nnz, heads],
        neither probs nor grad_bias, that receives the gradient in the scores whenever gQ, gK or gBias is wanted."""
        import torch
        return self._attention_dropout_backward(torch.float32, self.attention_dropout_backward_ptr, Q, K, V, probs, grad_out, scale, p, seed, heads,
                                                (grad_q, grad_k, grad_v, grad_bias), work, want)

    def attention_bf16_dropout_backward(self, Q, K, V, probs, grad_out, scale: float, p: float, seed: int, heads: int = 1, grad_q=None,
                                        grad_k=None, grad_v=None, grad_bias=None, work=None, want=(True, True, True, False)):
        """flex_attention_bf16_dropout_backward: attention_dropout_backward() on torch.bfloat16 Q, K, V and grad_out; gQ, gK and gV are
        bfloat16, probs, gBias and work float32."""
        import torch
        return self._attention_dropout_backward(torch.bfloat16, self.attention_bf16_dropout_backward_ptr, Q, K, V, probs, grad_out, scale, p, seed,
                                                heads, (grad_q, grad_k, grad_v, grad_bias), work, want)

    def gat_attention_ptr(self, heads: int, dEl_ptr: int, dEr_ptr: int, dV_ptr: int, slope: float, dOut_ptr: int, dP_ptr: int | None = None,
                          stream: int = 0):
        """flex_gat_attention; dEl is rows x H floats, dEr n x H, dP (optional) nnz x H, entry-major."""
        _check(_values_fn("flex_gat_attention")(self._h, heads, dEl_ptr, dEr_ptr, dV_ptr, slope, dOut_ptr, dP_ptr, stream), "flex_gat_attention")

    def _node_scalars(self, el, er):
        """heads, from el [m, H] and er [n, H]: one float32 per node and head."""
        import torch
        i = self.info()
        assert el.dim() == 2 and el.shape[1] >= 1, "el is [m, heads]"
        heads = int(el.shape[1])
        for t, rows in ((el, i["m"]), (er, i["n"])):
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (rows, heads), "float32 cuda [rows, heads]"
        return heads

    def gat_attention(self, el, er, V, slope: float = 0.2, out=None, p=None):
        """flex_gat_attention: out [m, k] = sum over each row's entries of alpha V[col] per head, alpha = the softmax over the row of
        leaky_relu(el[row, h] + er[col, h], slope), in one launch.  el: [m, H], er: [n, H] (H = el.shape[1] heads of k / H columns),
        V: [n, k] like B; float32 cuda tensors.  p (optional): a float32 cuda tensor [a.nnz, H] that receives alpha in a's CSR order
        for the plan's rows (entries of other shards keep what it held)."""
        import torch
        i = self.info()
        heads = self._node_scalars(el, er)
        assert V.is_cuda and V.dtype == torch.float32 and V.is_contiguous() and tuple(V.shape) == (i["n"], i["k"])
        if out is None:  # every row is written, except by a plan without entries, which launches nothing
            out = (torch.empty if i["nnz"] else torch.zeros)((i["m"], i["k"]), dtype=torch.float32, device=V.device)
        assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (i["m"], i["k"])
        if p is not None:
            self._head_edge_arrays(heads, p)
        self.gat_attention_ptr(heads, el.data_ptr(), er.data_ptr(), V.data_ptr(), slope, out.data_ptr(), None if p is None else p.data_ptr(),
                               torch.cuda.current_stream(V.device).cuda_stream)
        return out

    def gat_attention_backward_ptr(self, heads: int, dEl_ptr: int, dEr_ptr: int, dV_ptr: int, dP_ptr: int, dGradOut_ptr: int, slope: float,
                                   dGradEl_ptr: int | None, dGradEr_ptr: int | None, dGradV_ptr: int | None, dWork_ptr: int, stream: int = 0):
        """flex_gat_attention_backward; dP and dWork are nnz x H floats, entry-major."""
        _check(_values_fn("flex_gat_attention_backward")(self._h, heads, dEl_ptr, dEr_ptr, dV_ptr, dP_ptr, dGradOut_ptr, slope, dGradEl_ptr, dGradEr_ptr,
                                                         dGradV_ptr, dWork_ptr, stream), "flex_gat_attention_backward")

    def gat_attention_backward(self, el, er, V, p, grad_out, slope: float = 0.2, grad_el=None, grad_er=None, grad_v=None, work=None,
                               want=(True, True, True)):
        """flex_gat_attention_backward: (gEl [m, H], gEr [n, H], gV [n, k]) of gat_attention()'s out from its p [a.nnz, H] and grad_out
        [m, k], in two launches; an output that `want` does not ask for is None and is not computed.  work (optional): a float32 cuda
        tensor [a.nnz, H], not p, that receives the gradient in el + er per entry whenever gEl or gEr is wanted."""
        import torch
        i = self.info()
        heads = self._node_scalars(el, er)
        for t, rows in ((V, i["n"]), (grad_out, i["m"])):
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (rows, i["k"])
        if work is None:
            work = torch.empty((self.src_nnz, heads), dtype=torch.float32, device=V.device)
        self._head_edge_arrays(heads, p, work)
        outs = []
        for wanted, t, shape in zip(want, (grad_el, grad_er, grad_v), ((i["m"], heads), (i["n"], heads), (i["n"], i["k"]))):
            if wanted and t is None:  # every row is written, except by a plan without entries, which launches nothing
                t = (torch.empty if i["nnz"] else torch.zeros)(shape, dtype=torch.float32, device=V.device)
            if wanted:
                assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape
            outs.append(t if wanted else None)
        self.gat_attention_backward_ptr(heads, el.data_ptr(), er.data_ptr(), V.data_ptr(), p.data_ptr(), grad_out.data_ptr(), slope,
                                        *(None if t is None else t.data_ptr() for t in outs), work.data_ptr(),
                                        torch.cuda.current_stream(V.device).cuda_stream)
        return tuple(outs)

    def gatv2_attention_ptr(self, heads: int, dXt_ptr: int, dXs_ptr: int, dAtt_ptr: int, slope: float, dOut_ptr: int, dP_ptr: int | None = None,
                            stream: int = 0):
        """flex_gatv2_attention; dXt is rows x k floats (stride ldc), dXs n x k (stride ldb), dAtt k, dP (optional) nnz x H, entry-major."""
        _check(_values_fn("flex_gatv2_attention")(self._h, heads, dXt_ptr, dXs_ptr, dAtt_ptr, slope, dOut_ptr, dP_ptr, stream), "flex_gatv2_attention")

    def gatv2_attention_backward_ptr(self, heads: int, dXt_ptr: int, dXs_ptr: int, dAtt_ptr: int, dP_ptr: int, dGradOut_ptr: int, slope: float,
                                     dGradXt_ptr: int | None, dGradXs_ptr: int | None, dGradAtt_ptr: int | None, dWork_ptr: int,
                                     dAttWork_ptr: int | None = None, stream: int = 0):
        """flex_gatv2_attention_backward; dP and dWork are nnz x H floats, entry-major; dAttWork holds gatv2_attention_work_size() floats
        and is needed where dGradAtt is wanted."""
        _check(_values_fn("flex_gatv2_attention_backward")(self._h, heads, dXt_ptr, dXs_ptr, dAtt_ptr, dP_ptr, dGradOut_ptr, slope, dGradXt_ptr,
                                                           dGradXs_ptr, dGradAtt_ptr, dWork_ptr, dAttWork_ptr, stream), "flex_gatv2_attention_backward")

    def gatv2_attention_work_size(self) -> int:
        """flex_gatv2_attention_work_size: the floats of the dAttWork of gatv2_attention_backward_ptr (k per workgroup of its row launch)."""
        n = C.c_uint64(0)
        _check(_values_fn("flex_gatv2_attention_work_size")(self._h, C.byref(n)), "flex_gatv2_attention_work_size")
        return int(n.value)

    def _gatv2_operands(self, xt, xs, att):
        """heads, from att [H, d]; xt [m, k] like C, xs [n, k] like B: float32 cuda tensors, k = H d."""
        import torch
        i = self.info()
        assert att.dim() == 2 and att.shape[0] >= 1 and att.shape[0] * att.shape[1] == i["k"], "att is [heads, k / heads]"
        for t, shape in ((xt, (i["m"], i["k"])), (xs, (i["n"], i["k"])), (att, tuple(att.shape))):
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape, "float32 cuda, xt [m, k], xs [n, k]"
        return int(att.shape[0])

    def gatv2_attention(self, xt, xs, att, slope: float = 0.2, out=None, p=None):
        """flex_gatv2_attention: out [m, k] = sum over each row's entries of alpha xs[col] per head, alpha = the softmax over the row of
        <att[h], leaky_relu(xt[row, head h] + xs[col, head h], slope)>, in one launch.  xt: [m, k], xs: [n, k], att: [H, k / H]; float32
        cuda tensors; xt may be xs.  p (optional): a float32 cuda tensor [a.nnz, H] that receives alpha in a's CSR order for the plan's
        rows (entries of other shards keep what it held)."""
        import torch
        i = self.info()
        heads = self._gatv2_operands(xt, xs, att)
        if out is None:  # every row is written, except by a plan without entries, which launches nothing
            out = (torch.empty if i["nnz"] else torch.zeros)((i["m"], i["k"]), dtype=torch.float32, device=xs.device)
        assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (i["m"], i["k"])
        if p is not None:
            self._head_edge_arrays(heads, p)
        self.gatv2_attention_ptr(heads, xt.data_ptr(), xs.data_ptr(), att.data_ptr(), slope, out.data_ptr(), None if p is None else p.data_ptr(),
                                 torch.cuda.current_stream(xs.device).cuda_stream)
        return out

    def gatv2_attention_backward(self, xt, xs, att, p, grad_out, slope: float = 0.2, grad_xt=None, grad_xs=None, grad_att=None, work=None,
                                 want=(True, True, True), att_work=None):
        """flex_gatv2_attention_backward: (gXt [m, k], gXs [n, k], gAtt [H, k / H]) of gatv2_attention()'s out from its p [a.nnz, H] and
        grad_out [m, k], in up to three launches; an output that `want` does not ask for is None and is not computed.  work (optional): a
        float32 cuda tensor [a.nnz, H], not p, that receives dz = p (da - delta) per entry whenever a gradient is wanted.  att_work
        (optional): float32 cuda, at least gatv2_attention_work_size() floats; it is allocated here when gAtt is wanted and it is not passed."""
        import torch
        i = self.info()
        heads = self._gatv2_operands(xt, xs, att)
        assert grad_out.is_cuda and grad_out.dtype == torch.float32 and grad_out.is_contiguous() and tuple(grad_out.shape) == (i["m"], i["k"])
        if work is None:
            work = torch.empty((self.src_nnz, heads), dtype=torch.float32, device=xs.device)
        self._head_edge_arrays(heads, p, work)
        outs = []
        for wanted, t, shape in zip(want, (grad_xt, grad_xs, grad_att), ((i["m"], i["k"]), (i["n"], i["k"]), tuple(att.shape))):
            if wanted and t is None:  # every element is written, except by a plan without entries, which launches nothing
                t = (torch.empty if i["nnz"] else torch.zeros)(shape, dtype=torch.float32, device=xs.device)
            if wanted:
                assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape
            outs.append(t if wanted else None)
        if outs[2] is not None:
            need = self.gatv2_attention_work_size()
            if att_work is None:
                att_work = torch.empty(max(need, 1), dtype=torch.float32, device=xs.device)
            assert att_work.is_cuda and att_work.dtype == torch.float32 and att_work.is_contiguous() and att_work.numel() >= need
        self.gatv2_attention_backward_ptr(heads, xt.data_ptr(), xs.data_ptr(), att.data_ptr(), p.data_ptr(), grad_out.data_ptr(), slope,
                                          *(None if t is None else t.data_ptr() for t in outs), work.data_ptr(),
                                          None if outs[2] is None else att_work.data_ptr(), torch.cuda.current_stream(xs.device).cuda_stream)
        return tuple(outs)

    def gatv2_attention_dropout_ptr(self, heads: int, dXt_ptr: int, dXs_ptr: int, dAtt_ptr: int, slope: float, p: float, seed: int, dOut_ptr: int,
                                    dP_ptr: int | None = None, stream: int = 0):
        """flex_dropout_gatv2_attention; the operands are gatv2_attention_ptr's; dP (optional) receives the UNDROPPED alpha."""
        _check(_values_fn("flex_dropout_gatv2_attention")(self._h, heads, dXt_ptr, dXs_ptr, dAtt_ptr, slope, p, seed, dOut_ptr, dP_ptr, stream),
               "flex_dropout_gatv2_attention")

    def gatv2_attention_dropout(self, xt, xs, att, slope: float, p: float, seed: int, out=None, probs=None):
        """flex_dropout_gatv2_attention: gatv2_attention() whose probabilities are dropped after the softmax with probability p in [0, 1),
        the kept ones scaled by 1 / (1 - p); the mask is binding.dropout_mask(seed, p, e * H + h), a function of the 64-bit seed.  A
        dropped entry stays in the softmax.  probs (optional, float32 [a.nnz, H]) receives the UNDROPPED alpha, which
        gatv2_attention_dropout_backward() starts from."""
        import torch
        i = self.info()
        heads = self._gatv2_operands(xt, xs, att)
        if out is None:  # every row is written, except by a plan without entries, which launches nothing
            out = (torch.empty if i["nnz"] else torch.zeros)((i["m"], i["k"]), dtype=torch.float32, device=xs.device)
        assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (i["m"], i["k"])
        if probs is not None:
            self._head_edge_arrays(heads, probs)
        self.gatv2_attention_dropout_ptr(heads, xt.data_ptr(), xs.data_ptr(), att.data_ptr(), slope, p, int(seed) & 0xFFFFFFFFFFFFFFFF, out.data_ptr(),
                                         None if probs is None else probs.data_ptr(), torch.cuda.current_stream(xs.device).cuda_stream)
        return out

    def gatv2_attention_dropout_backward_ptr(self, heads: int, dXt_ptr: int, dXs_ptr: int, dAtt_ptr: int, dP_ptr: int, dGradOut_ptr: int,
                                             slope: float, p: float, seed: int, dGradXt_ptr: int | None, dGradXs_ptr: int | None,
                                             dGradAtt_ptr: int | None, dWork_ptr: int, dAttWork_ptr: int | None = None, stream: int = 0):
        """flex_dropout_gatv2_attention_backward; the operands are gatv2_attention_backward_ptr's, under the forward's p and seed."""
        _check(_values_fn("flex_dropout_gatv2_attention_backward")(self._h, heads, dXt_ptr, dXs_ptr, dAtt_ptr, dP_ptr, dGradOut_ptr, slope, p, seed,
                                                                   dGradXt_ptr, dGradXs_ptr, dGradAtt_ptr, dWork_ptr, dAttWork_ptr, stream),
               "flex_dropout_gatv2_attention_backward")

    def gatv2_attention_dropout_backward(self, xt, xs, att, probs, grad_out, slope: float, p: float, seed: int, grad_xt=None, grad_xs=None,
                                         grad_att=None, work=None, want=(True, True, True), att_work=None):
        """flex_dropout_gatv2_attention_backward: (gXt [m, k], gXs [n, k], gAtt [H, k / H]) of gatv2_attention_dropout()'s out from its
        probs [a.nnz, H] (the undropped alpha), grad_out [m, k] and the same p and seed, in up to three launches; an output that `want`
        does not ask for is None and is not computed.  work and att_work are gatv2_attention_backward()'s."""
        import torch
        i = self.info()
        heads = self._gatv2_operands(xt, xs, att)
        assert grad_out.is_cuda and grad_out.dtype == torch.float32 and grad_out.is_contiguous() and tuple(grad_out.shape) == (i["m"], i["k"])
        if work is None:
            work = torch.empty((self.src_nnz, heads), dtype=torch.float32, device=xs.device)
        self._head_edge_arrays(heads, probs, work)
        outs = []
        for wanted, t, shape in zip(want, (grad_xt, grad_xs, grad_att), ((i["m"], i["k"]), (i["n"], i["k"]), tuple(att.shape))):
            if wanted and t is None:  # every element is written, except by a plan without entries, which launches nothing
                t = (torch.empty if i["nnz"] else torch.zeros)(shape, dtype=torch.float32, device=xs.device)
            if wanted:
                assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape
            outs.append(t if wanted else None)
        if outs[2] is not None:
            need = self.gatv2_attention_work_size()
            if att_work is None:
                att_work = torch.empty(max(need, 1), dtype=torch.float32, device=xs.device)
            assert att_work.is_cuda and att_work.dtype == torch.float32 and att_work.is_contiguous() and att_work.numel() >= need
        self.gatv2_attention_dropout_backward_ptr(heads, xt.data_ptr(), xs.data_ptr(), att.data_ptr(), probs.data_ptr(), grad_out.data_ptr(), slope, p,
                                                  int(seed) & 0xFFFFFFFFFFFFFFFF, *(None if t is None else t.data_ptr() for t in outs),
                                                  work.data_ptr(), None if outs[2] is None else att_work.data_ptr(),
                                                  torch.cuda.current_stream(xs.device).cuda_stream)
        return tuple(outs)

    def gat_attention_dropout_ptr(self, heads: int, dEl_ptr: int, dEr_ptr: int, dV_ptr: int, slope: float, p: float, seed: int, dOut_ptr: int,
                                  dP_ptr: int | None = None, stream: int = 0):
        """flex_gat_attention_dropout; dEl is rows x H floats, dEr n x H, dP (optional) nnz x H, entry-major: it receives the UNDROPPED
        alpha."""
        _check(_values_fn("flex_gat_attention_dropout")(self._h, heads, dEl_ptr, dEr_ptr, dV_ptr, slope, p, seed, dOut_ptr, dP_ptr, stream),
               "flex_gat_attention_dropout")

    def gat_attention_dropout(self, el, er, V, slope: float, p: float, seed: int, out=None, probs=None):
        """flex_gat_attention_dropout: gat_attention() whose probabilities are dropped after the softmax with probability p in [0, 1), the
        kept ones scaled by 1 / (1 - p); the mask is binding.dropout_mask(seed, p, e * H + h), a function of the 64-bit seed.  probs
        (optional, float32 [a.nnz, H]) receives the UNDROPPED alpha, which gat_attention_dropout_backward() starts from."""
        import torch
        i = self.info()
        heads = self._node_scalars(el, er)
        assert V.is_cuda and V.dtype == torch.float32 and V.is_contiguous() and tuple(V.shape) == (i["n"], i["k"])
        if out is None:  # every row is written, except by a plan without entries, which launches nothing
            out = (torch.empty if i["nnz"] else torch.zeros)((i["m"], i["k"]), dtype=torch.float32, device=V.device)
        assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (i["m"], i["k"])
        if probs is not None:
            self._head_edge_arrays(heads, probs)
        self.gat_attention_dropout_ptr(heads, el.data_ptr(), er.data_ptr(), V.data_ptr(), slope, p, int(seed) & 0xFFFFFFFFFFFFFFFF, out.data_ptr(),
                                       None if probs is None else probs.data_ptr(), torch.cuda.current_stream(V.device).cuda_stream)
        return out

    def gat_attention_dropout_backward_ptr(self, heads: int, dEl_ptr: int, dEr_ptr: int, dV_ptr: int, dP_ptr: int, dGradOut_ptr: int, slope: float,
                                           p: float, seed: int, dGradEl_ptr: int | None, dGradEr_ptr: int | None, dGradV_ptr: int | None,
                                           dWork_ptr: int, stream: int = 0):
        """flex_gat_attention_dropout_backward; dP and dWork are nnz x H floats, entry-major."""
        _check(_values_fn("flex_gat_attention_dropout_backward")(self._h, heads, dEl_ptr, dEr_ptr, dV_ptr, dP_ptr, dGradOut_ptr, slope, p, seed,
                                                                 dGradEl_ptr, dGradEr_ptr, dGradV_ptr, dWork_ptr, stream),
               "flex_gat_attention_dropout_backward")

    def gat_attention_dropout_backward(self, el, er, V, probs, grad_out, slope: float, p: float, seed: int, grad_el=None, grad_er=None,
                                       grad_v=None, work=None, want=(True, True, True)):
        """flex_gat_attention_dropout_backward: (gEl [m, H], gEr [n, H], gV [n, k]) of gat_attention_dropout()'s out from its probs
        [a.nnz, H] (the undropped alpha), grad_out [m, k] and the same p and seed, in two launches; an output that `want` does not ask
        for is None and is not computed.  work (optional): a float32 cuda tensor [a.nnz, H], not probs, that receives the gradient in
        el + er per entry whenever gEl or gEr is wanted."""
        import torch
        i = self.info()
        heads = self._node_scalars(el, er)
        for t, rows in ((V, i["n"]), (grad_out, i["m"])):
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (rows, i["k"])
        if work is None:
            work = torch.empty((self.src_nnz, heads), dtype=torch.float32, device=V.device)
        self._head_edge_arrays(heads, probs, work)
        outs = []
        for wanted, t, shape in zip(want, (grad_el, grad_er, grad_v), ((i["m"], heads), (i["n"], heads), (i["n"], i["k"]))):
            if wanted and t is None:  # every row is written, except by a plan without entries, which launches nothing
                t = (torch.empty if i["nnz"] else torch.zeros)(shape, dtype=torch.float32, device=V.device)
            if wanted:
                assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape
            outs.append(t if wanted else None)
        self.gat_attention_dropout_backward_ptr(heads, el.data_ptr(), er.data_ptr(), V.data_ptr(), probs.data_ptr(), grad_out.data_ptr(), slope, p,
                                                int(seed) & 0xFFFFFFFFFFFFFFFF, *(None if t is None else t.data_ptr() for t in outs),
                                                work.data_ptr(), torch.cuda.current_stream(V.device).cuda_stream)
        return tuple(outs)

    def gat_attention_bf16_ptr(self, heads: int, dEl_ptr: int, dEr_ptr: int, dV_ptr: int, slope: float, dOut_ptr: int, dP_ptr: int | None = None,
                               stream: int = 0):
        """flex_gat_attention_bf16: gat_attention_ptr with bf16 rows V and Out; dEl, dEr and dP (optional) stay floats."""
        _check(_values_fn("flex_gat_attention_bf16")(self._h, heads, dEl_ptr, dEr_ptr, dV_ptr, slope, dOut_ptr, dP_ptr, stream),
               "flex_gat_attention_bf16")

    def gat_attention_bf16_backward_ptr(self, heads: int, dEl_ptr: int, dEr_ptr: int, dV_ptr: int, dP_ptr: int, dGradOut_ptr: int, slope: float,
                                        dGradEl_ptr: int | None, dGradEr_ptr: int | None, dGradV_ptr: int | None, dWork_ptr: int, stream: int = 0):
        """flex_gat_attention_bf16_backward: gat_attention_backward_ptr with bf16 rows V, g and gV; the rest stays floats."""
        _check(_values_fn("flex_gat_attention_bf16_backward")(self._h, heads, dEl_ptr, dEr_ptr, dV_ptr, dP_ptr, dGradOut_ptr, slope, dGradEl_ptr,
                                                              dGradEr_ptr, dGradV_ptr, dWork_ptr, stream), "flex_gat_attention_bf16_backward")

    def gat_attention_bf16_dropout_ptr(self, heads: int, dEl_ptr: int, dEr_ptr: int, dV_ptr: int, slope: float, p: float, seed: int, dOut_ptr: int,
                                       dP_ptr: int | None = None, stream: int = 0):
        """flex_gat_attention_bf16_dropout: gat_attention_dropout_ptr with bf16 rows V and Out."""
        _check(_values_fn("flex_gat_attention_bf16_dropout")(self._h, heads, dEl_ptr, dEr_ptr, dV_ptr, slope, p, seed, dOut_ptr, dP_ptr, stream),
               "flex_gat_attention_bf16_dropout")

    def gat_attention_bf16_dropout_backward_ptr(self, heads: int, dEl_ptr: int, dEr_ptr: int, dV_ptr: int, dP_ptr: int, dGradOut_ptr: int,
                                                slope: float, p: float, seed: int, dGradEl_ptr: int | None, dGradEr_ptr: int | None,
                                                dGradV_ptr: int | None, dWork_ptr: int, stream: int = 0):
        """flex_gat_attention_bf16_dropout_backward: gat_attention_dropout_backward_ptr with bf16 rows V, g and gV."""
        _check(_values_fn("flex_gat_attention_bf16_dropout_backward")(self._h, heads, dEl_ptr, dEr_ptr, dV_ptr, dP_ptr, dGradOut_ptr, slope, p, seed,
                                                                      dGradEl_ptr, dGradEr_ptr, dGradV_ptr, dWork_ptr, stream),
               "flex_gat_attention_bf16_dropout_backward")

    def _gat_bf16(self, run, el, er, V, args, out, p):
        """The forward of the two bf16 GAT calls: run(heads, el, er, V, *args, out, p, stream) on bfloat16 V and out, float32 el, er, p."""
        import torch
        i = self.info()
        heads = self._node_scalars(el, er)
        assert V.is_cuda and V.dtype == torch.bfloat16 and V.is_contiguous() and tuple(V.shape) == (i["n"], i["k"]), "V: bfloat16 cuda [n, k]"
        if out is None:  # every row is written, except by a plan without entries, which launches nothing
            out = (torch.empty if i["nnz"] else torch.zeros)((i["m"], i["k"]), dtype=torch.bfloat16, device=V.device)
        assert out.is_cuda and out.dtype == torch.bfloat16 and out.is_contiguous() and tuple(out.shape) == (i["m"], i["k"])
        if p is not None:
            self._head_edge_arrays(heads, p)
        run(heads, el.data_ptr(), er.data_ptr(), V.data_ptr(), *args, out.data_ptr(), None if p is None else p.data_ptr(),
            torch.cuda.current_stream(V.device).cuda_stream)
        return out

    def _gat_bf16_backward(self, run, el, er, V, p, grad_out, args, grads, work, want):
        """The backward of the two bf16 GAT calls: V, grad_out and gV bfloat16; el, er, gEl, gEr, p and work float32."""
        import torch
        i = self.info()
        heads = self._node_scalars(el, er)
        for t, rows in ((V, i["n"]), (grad_out, i["m"])):
            assert t.is_cuda and t.dtype == torch.bfloat16 and t.is_contiguous() and tuple(t.shape) == (rows, i["k"]), "bfloat16 cuda [rows, k]"
        if work is None:
            work = torch.empty((self.src_nnz, heads), dtype=torch.float32, device=V.device)
        self._head_edge_arrays(heads, p, work)
        outs = []
        shapes = (((i["m"], heads), torch.float32), ((i["n"], heads), torch.float32), ((i["n"], i["k"]), torch.bfloat16))
        for wanted, t, (shape, dtype) in zip(want, grads, shapes):
            if wanted and t is None:  # every row is written, except by a plan without entries, which launches nothing
                t = (torch.empty if i["nnz"] else torch.zeros)(shape, dtype=dtype, device=V.device)
            if wanted:
                assert t.is_cuda and t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == shape
            outs.append(t if wanted else None)
        run(heads, el.data_ptr(), er.data_ptr(), V.data_ptr(), p.data_ptr(), grad_out.data_ptr(), *args,
            *(None if t is None else t.data_ptr() for t in outs), work.data_ptr(), torch.cuda.current_stream(V.device).cuda_stream)
        return tuple(outs)

    def gat_attention_bf16(self, el, er, V, slope: float = 0.2, out=None, p=None):
        """flex_gat_attention_bf16: gat_attention() on torch.bfloat16 V [n, k]; out [m, k] is bfloat16, every sum float32 and each element
        rounded once at its store.  el [m, H], er [n, H] and p (optional, [a.nnz, H]) are float32."""
        return self._gat_bf16(self.gat_attention_bf16_ptr, el, er, V, (slope,), out, p)

    def gat_attention_bf16_backward(self, el, er, V, p, grad_out, slope: float = 0.2, grad_el=None, grad_er=None, grad_v=None, work=None,
                                    want=(True, True, True)):
        """flex_gat_attention_bf16_backward: gat_attention_backward() on torch.bfloat16 V and grad_out; gV is bfloat16, rounded once at its
        store; gEl, gEr, p and work are float32."""
        return self._gat_bf16_backward(self.gat_attention_bf16_backward_ptr, el, er, V, p, grad_out, (slope,), (grad_el, grad_er, grad_v), work, want)

    def gat_attention_bf16_dropout(self, el, er, V, slope: float, p: float, seed: int, out=None, probs=None):
        """flex_gat_attention_bf16_dropout: gat_attention_dropout() on torch.bfloat16 V; out is bfloat16; probs (optional, float32
        [a.nnz, H]) receives the UNDROPPED alpha."""
        return self._gat_bf16(self.gat_attention_bf16_dropout_ptr, el, er, V, (slope, p, int(seed) & 0xFFFFFFFFFFFFFFFF), out, probs)

    def gat_attention_bf16_dropout_backward(self, el, er, V, probs, grad_out, slope: float, p: float, seed: int, grad_el=None, grad_er=None,
                                            grad_v=None, work=None, want=(True, True, True)):
        """flex_gat_attention_bf16_dropout_backward: gat_attention_dropout_backward() on torch.bfloat16 V and grad_out under the same p and
        seed; gV is bfloat16; gEl, gEr, probs and work are float32."""
        return self._gat_bf16_backward(self.gat_attention_bf16_dropout_backward_ptr, el, er, V, probs, grad_out,
                                       (slope, p, int(seed) & 0xFFFFFFFFFFFFFFFF), (grad_el, grad_er, grad_v), work, want)

    def gat_edge_attention_ptr(self, heads: int, dEl_ptr: int, dEr_ptr: int, dEe_ptr: int, dV_ptr: int, slope: float, p: float, seed: int,
                               dOut_ptr: int, dP_ptr: int | None = None, stream: int = 0):
        """flex_edge_gat_attention; dEl is rows x H floats, dEr n x H, dEe and dP (optional) nnz x H, entry-major; dP receives the
        UNDROPPED alpha."""
        _check(_values_fn("flex_edge_gat_attention")(self._h, heads, dEl_ptr, dEr_ptr, dEe_ptr, dV_ptr, slope, p, seed, dOut_ptr, dP_ptr, stream),
               "flex_edge_gat_attention")

    def gat_edge_attention(self, el, er, ee, V, slope: float, drop_p: float = 0.0, seed: int = 0, out=None, probs=None):
        """flex_edge_gat_attention: gat_attention() (drop_p = 0) or gat_attention_dropout() with a per-edge term inside the LeakyReLU, the
        score leaky_relu((el[row, h] + er[col, h]) + ee[e, h], slope).  ee: float32 cuda [a.nnz, H] in a's CSR order; -inf masks one
        entry for one head.  probs (optional, float32 [a.nnz, H]) receives the UNDROPPED alpha."""
        import torch
        i = self.info()
        heads = self._node_scalars(el, er)
        self._head_edge_arrays(heads, ee)
        assert V.is_cuda and V.dtype == torch.float32 and V.is_contiguous() and tuple(V.shape) == (i["n"], i["k"])
        if out is None:  # every row is written, except by a plan without entries, which launches nothing
            out = (torch.empty if i["nnz"] else torch.zeros)((i["m"], i["k"]), dtype=torch.float32, device=V.device)
        assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (i["m"], i["k"])
        if probs is not None:
            self._head_edge_arrays(heads, probs)
        self.gat_edge_attention_ptr(heads, el.data_ptr(), er.data_ptr(), ee.data_ptr(), V.data_ptr(), slope, drop_p, int(seed) & 0xFFFFFFFFFFFFFFFF,
                                    out.data_ptr(), None if probs is None else probs.data_ptr(), torch.cuda.current_stream(V.device).cuda_stream)
        return out

    def gat_edge_attention_backward_ptr(self, heads: int, dEl_ptr: int, dEr_ptr: int, dEe_ptr: int, dV_ptr: int, dP_ptr: int, dGradOut_ptr: int,
                                        slope: float, p: float, seed: int, dGradEl_ptr: int | None, dGradEr_ptr: int | None,
                                        dGradEe_ptr: int | None, dGradV_ptr: int | None, dWork_ptr: int | None, stream: int = 0):
        """flex_edge_gat_attention_backward; dEe, dP, dGradEe and dWork are nnz x H floats, entry-major; the work array is dGradEe where
        it is given, else dWork."""
        _check(_values_fn("flex_edge_gat_attention_backward")(self._h, heads, dEl_ptr, dEr_ptr, dEe_ptr, dV_ptr, dP_ptr, dGradOut_ptr, slope, p, seed,
                                                              dGradEl_ptr, dGradEr_ptr, dGradEe_ptr, dGradV_ptr, dWork_ptr, stream),
               "flex_edge_gat_attention_backward")

    def gat_edge_attention_backward(self, el, er, ee, V, probs, grad_out, slope: float, drop_p: float = 0.0, seed: int = 0,
                                    want=(True, True, True, True), grad_el=None, grad_er=None, grad_ee=None, grad_v=None, work=None):
        """flex_edge_gat_attention_backward: (gEl [m, H], gEr [n, H], gEe [a.nnz, H], gV [n, k]) of gat_edge_attention()'s out from its
        probs (the undropped alpha), grad_out [m, k] and the same drop_p and seed, in two launches; an output that `want` does not ask
        for is None and is not computed.  The gEe tensor is the call's work array: the kernel writes dx into it and nothing is copied.
        work (optional, float32 cuda [a.nnz, H], not probs) is the work array when gEe is not wanted; it is allocated here when needed."""
        import torch
        i = self.info()
        heads = self._node_scalars(el, er)
        for t, rows in ((V, i["n"]), (grad_out, i["m"])):
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (rows, i["k"])
        self._head_edge_arrays(heads, ee, probs)
        shapes = ((i["m"], heads), (i["n"], heads), (self.src_nnz, heads), (i["n"], i["k"]))
        outs = []
        for wanted, t, shape in zip(want, (grad_el, grad_er, grad_ee, grad_v), shapes):
            if wanted and t is None:  # every row is written, except by a plan without entries, which launches nothing
                t = (torch.empty if i["nnz"] else torch.zeros)(shape, dtype=torch.float32, device=V.device)
            if wanted:
                assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape
            outs.append(t if wanted else None)
        if outs[2] is None and work is None:
            work = torch.empty((self.src_nnz, heads), dtype=torch.float32, device=V.device)
        if work is not None:
            self._head_edge_arrays(heads, work)
        self.gat_edge_attention_backward_ptr(heads, el.data_ptr(), er.data_ptr(), ee.data_ptr(), V.data_ptr(), probs.data_ptr(), grad_out.data_ptr(),
                                             slope, drop_p, int(seed) & 0xFFFFFFFFFFFFFFFF, *(None if t is None else t.data_ptr() for t in outs),
                                             None if work is None else work.data_ptr(), torch.cuda.current_stream(V.device).cuda_stream)
        return tuple(outs)

    def destroy(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().flex_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def dropout_mask(seed: int, p: float, first: int, count: int) -> np.ndarray:
    """flex_dropout_mask: the keep bits (uint8, 1 = kept) of the indices first .. first + count - 1 of the attention dropout's mask under
    `seed` and the probability p; index e * heads + h is entry e (a's CSR order), head h.  Host code: no GPU is needed."""
    keep = np.empty(count, np.uint8)
    _check(lib().flex_dropout_mask(seed & 0xFFFFFFFFFFFFFFFF, p, first, count, keep.ctypes.data), "flex_dropout_mask")
    return keep


def gather_rows(dst_ptr: int, src_ptr: int, idx_ptr: int, n: int, k: int, stream: int = 0):
    _check(lib().flex_gather_rows(dst_ptr, src_ptr, idx_ptr, n, k, stream), "flex_gather_rows")
