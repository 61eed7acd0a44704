"""Test infrastructure: libflex_hostsim.so = the library's HOST code (parsers, orderings, generator, planner) linked against
tests/hostsim/shim.cpp instead of the kernels, with "device memory" malloc'ed on the host.  It cannot compute an SpMM (every
launcher reports FLEX_ERR_UNSUPPORTED); it exists so that plans can be created and their image checked without a GPU."""
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_CSRC = os.path.join(_ROOT, "flex_amd", "csrc")
_OUT = os.path.join(_HERE, "_build", "libflex_hostsim.so")
HOST_SOURCES = ["plan.cpp", "plan_build.cpp", "block_plan.cpp", "plan_check.cpp", "dense_tiles.cpp", "ingest.cpp", "reorder.cpp", "cluster.cpp", "rabbit.cpp", "gorder.cpp", "shard.cpp", "synth.cpp"]


def build(extra_flags=(), out=_OUT):
    srcs = [os.path.join(_CSRC, f) for f in HOST_SOURCES] + [os.path.join(_HERE, "shim.cpp")]
    deps = srcs + [os.path.join(_CSRC, h) for h in ("internal.h", "plan.h", "host_parallel.h", "attention_entry.h")] + [os.path.join(_ROOT, "include", "flex_spmm.h")]
    if os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in deps):
        return out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = ["g++", "-std=c++20", "-O1", "-fPIC", "-shared", "-DFLEX_HOSTSIM", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + _CSRC,
           "-Wl,-Bsymbolic-functions", "-o", out] + list(extra_flags) + srcs + ["-lpthread", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"]  # the HIP calls the shim does not replace are never reached
    subprocess.check_call(cmd)
    return out


def binding_on_simulator():
    """The body of a pytest fixture: flex_amd.binding loads the host-simulated library (FLEX_HOSTSIM_LIB, or the one build() makes) until
    the fixture ends, and the fixture's value is that library."""
    from flex_amd import binding
    so = os.environ.get("FLEX_HOSTSIM_LIB") or build()
    old_so, old_lib = binding._SO, binding._lib
    binding._SO, binding._lib = so, None
    yield binding.lib()
    binding._SO, binding._lib = old_so, old_lib


def launch_log(L, fn):
    """The kernel instantiations that fn() launched through L (a host-simulated library), in order, as `nm -C` names them: fn runs with
    the shim's launch log on (tests/hostsim/shim.cpp), where every launcher records what the real one would launch and computes nothing."""
    import ctypes
    L.hostsim_launch_log.argtypes = [ctypes.c_int]
    L.hostsim_launch_log_read.restype = ctypes.c_char_p
    L.hostsim_launch_log(1)
    try:
        fn()
        return L.hostsim_launch_log_read().decode().splitlines()
    finally:
        L.hostsim_launch_log(0)
