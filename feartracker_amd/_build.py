"""Build the gfx950 shared library in-tree (feartracker_amd/libfear_hip.so) with hipcc.

The `.so` is git-ignored but travels to the GPU box with the gpurun snapshot; nothing is
JIT-compiled at run time.
"""
from __future__ import annotations

import glob
import os
import shutil
import subprocess

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(PKG_DIR, "csrc", "fear_engine.hip")
# everything the one translation unit is made of: a header added under csrc/ or include/ is a dependency without being named here
DEPS = sorted(glob.glob(os.path.join(PKG_DIR, "csrc", "*.h")) + glob.glob(os.path.join(PKG_DIR, "csrc", "*.hip")) +
              glob.glob(os.path.join(os.path.dirname(PKG_DIR), "include", "*.h")))
LIB = os.path.join(PKG_DIR, "libfear_hip.so")
# kernels allowed to spill, and how many VGPRs at most (mangled-name substring -> cap): everything else warns
KNOWN_SPILLS = {"headchain_kernel": 16, "headchain_b_kernel": 16,
                # the 3 x 3 stride-1 depthwise backward with BatchNorm1 (one block of the trunk: 32 -> 192 -> 32 at 32 x 32): 16 registers
                # spilled around its tile fill; 2 launches of 69 us per 128-pair training step (0.14 of 24.5 ms of kernel time,
                # profiles/r05_train_kernel_stats.csv) — with __launch_bounds__(256, 1) it does not spill and runs at half the occupancy
                "dw_bwd_kernelILi3ELi1ELi8ELb1ELi0ELi16ELb0E": 16}


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: cannot build libfear_hip.so")


def is_stale() -> bool:
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    return any(os.path.exists(d) and os.path.getmtime(d) > t for d in DEPS)


def build_library(force: bool = False, verbose: bool = False) -> str:
    """Compile csrc/fear_engine.hip for gfx950 (cross-compiles without a GPU)."""
    if not force and not is_stale():
        return LIB
    cmd = [_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC", "-Wno-unused-value", "-fno-honor-nans",
           "-Rpass-analysis=kernel-resource-usage", "-o", LIB + ".tmp", SRC]
    if verbose:
        print(" ".join(cmd))
    res = subprocess.run(cmd, check=True, capture_output=True, text=True)
    os.replace(LIB + ".tmp", LIB)
    spills = check_spills(res.stderr)
    spilled = {name for name, _ in spills}
    for name, nbytes in check_scratch(res.stderr):
        # scratch WITHOUT spilled registers = a private array hipcc could not keep in registers — in this code base that has always
        # been a `#pragma unroll` loop left rolled (its ring / window arrays indexed by a run-time counter): chain32's four-row chain
        # ran at 575-2000 us instead of 250 that way (profiles/r06_chain32_kbench.txt); write such loops with static_for
        if name not in spilled:
            print(f"WARNING: {name} uses {nbytes} B of scratch per lane without spilling registers (a loop left rolled? "
                  "index arrays by compile-time constants: static_for)")
    for name, n in spills:
        # the two chained head kernels are known to carry a handful of spilled registers outside their loops (ten scratch
        # instructions per launch); the tolerance is theirs alone, by name and count — a new spill in any other fused kernel, or a
        # spill STORM (hundreds) in these, is what a compiler regression looks like
        known = next((cap for key, cap in KNOWN_SPILLS.items() if key in name), None)
        if known is not None and n <= known:
            print(f"note: {name} spills {n} VGPRs to scratch (known and priced: KNOWN_SPILLS)")
        else:
            print(f"WARNING: {name} spills {n} VGPRs to scratch (hipcc scheduling is fragile around the fused kernels; "
                  "a spilling build is several times slower)")
    return LIB


def check_spills(remarks: str):
    """Parse hipcc's kernel-resource-usage remarks: [(kernel symbol, spilled VGPRs)] for kernels that spill."""
    import re
    out, name = [], None
    for line in remarks.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"VGPRs Spill: (\d+)", line)
        if m and name and int(m.group(1)) > 0:
            out.append((name, int(m.group(1))))
    return out


def check_scratch(remarks: str):
    """[(kernel symbol, scratch bytes per lane)] for kernels with a non-zero ScratchSize."""
    import re
    out, name = [], None
    for line in remarks.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name and int(m.group(1)) > 0:
            out.append((name, int(m.group(1))))
    return out


def build_debug_library(verbose: bool = False) -> str:
    """Debug target: the same translation unit with the device code built exactly like the product (-O3) and the
    HOST side at -O1 -g, instrumented — UndefinedBehavior-
    Sanitizer (bounds, integer overflow, null, alignment; traps instead of recovering) and libstdc++'s container assertions
    (every std::vector operator[] of the engine's model / plan / workspace bookkeeping is range-checked) — written next to the
    product library as libfear_hip_debug.so (git-ignored).  On the GPU box:
        FEAR_LIB=feartracker_amd/libfear_hip_debug.so python -m pytest tests -m gpu -x -q
    (FEAR_LIB selects the library hip_backend loads).  AddressSanitizer was tried first and is NOT usable here: ROCm's
    compiler-rt intercepts hsa_amd_memory_pool_allocate and aborts inside torch's stock libamdhip64 (it needs an xnack+
    ASan build of the whole runtime); device code is the same in both builds."""
    out = os.path.join(PKG_DIR, "libfear_hip_debug.so")
    # (-fsanitize=function instruments the entry of every function and breaks the launch of HIP kernels through the function
    # pointers the engine's kernel tables hold: wrong maps, no trap — excluded)
    host = ["-O1", "-g", "-fsanitize=undefined", "-fno-sanitize=function,vptr", "-fsanitize-trap=undefined", "-fno-omit-frame-pointer"]
    cmd = [_hipcc(), "--offload-arch=gfx950", "-std=c++17", "-shared", "-fPIC", "-Wno-unused-value", "-fno-honor-nans",
           "-D_GLIBCXX_ASSERTIONS", "-Xarch_device", "-O3"]
    for f in host:
        cmd += ["-Xarch_host", f]
    cmd += ["-o", out, SRC]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return out


if __name__ == "__main__":
    import sys
    if "--debug" in sys.argv:
        print(build_debug_library(verbose=True))
    else:
        print(build_library(force=True, verbose=True))
