#!/usr/bin/env python3
"""What a Fortran host pays per call, three ways, in a FRESH process (where the arrays land moves rates by 3-5 %, DESIGN.md
section 5).  Prints one JSON line.

    python tools/f90_native_bench.py --np 4 --nlev 72 --elems 10000      # one configuration
    python tools/f90_native_bench.py                                      # the three of tools/perf_guard.py, each in a
                                                                          # fresh child process (one JSON line each)

Arms, alternated block by block (HIP events on the launch stream; the adaptive window is off, the cache window at its
default, both layouts from the library's allocator):
  (a) caar_launch on C++-layout arrays;
  (b) caar_launch_f90 on Fortran-ordered arrays (include/caar_f90.h);
  (c) caar_layout_from_f90 + caar_launch + caar_layout_to_f90 (mutated arrays only): the route a Fortran host had before.
After a warm-up, NBLOCK rounds of one block of `--calls` calls per arm; the figure per arm is the best block (ms per call),
the median block next to it."""
import argparse
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = ((4, 72, 10000), (4, 128, 12500), (8, 72, 20000))   # tools/perf_guard.py's

ap = argparse.ArgumentParser()
ap.add_argument("--np", type=int, dest="np_")
ap.add_argument("--nlev", type=int)
ap.add_argument("--elems", type=int)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--rounds", type=int, default=7)
a = ap.parse_args()

if a.np_ is None:
    for np_, nlev, elems in CONFIGS:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--np", str(np_), "--nlev", str(nlev), "--elems",
                            str(elems), "--calls", str(a.calls), "--rounds", str(a.rounds)], capture_output=True, text=True,
                           timeout=600)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit(r.returncode)
        print(r.stdout.strip().splitlines()[-1], flush=True)
    sys.exit(0)

import ctypes as C  # noqa: E402

import torch  # noqa: E402

import tinman_sandbox_amd as tsa  # noqa: E402
from tinman_sandbox_amd import f90_layout as fl  # noqa: E402

L = tsa.library()
lib = L.lib
dev = torch.device("cuda", 0)
st = torch.cuda.current_stream(dev)
lib.caar_set_adaptive_window(0)

np_, nlev, E = a.np_, a.nlev, a.elems
data = tsa.TestData().init_data(E, np_, nlev, device=dev)       # (a): C++ layout, the library's allocator
f90 = fl.F90Arrays.allocate(np_, nlev, E, device=dev)            # (b): the same values in Fortran order, same allocator
fl.egress(data.arrays, f90, all_arrays=True)
work = tsa.ElementArrays(np_, nlev, E, device=dev)               # (c): the C++ copy the conversion route needs
torch.cuda.synchronize(dev)

dims, prm = data.arrays.dims(), data.params(device_constants=True)
dvv = C.c_void_p(data.dvv_device().data_ptr())
sp = C.c_void_p(st.cuda_stream)
p_cpp, p_f90, p_work = data.arrays.pointers(), f90.pointers(), work.pointers()


def arm_a():
    L.check(lib.caar_launch(C.byref(dims), C.byref(p_cpp), dvv, C.byref(prm), sp), "caar_launch")


def arm_b():
    L.check(lib.caar_launch_f90(C.byref(dims), C.byref(p_f90), dvv, C.byref(prm), sp), "caar_launch_f90")


def arm_c():
    L.check(lib.caar_layout_from_f90(C.byref(dims), C.byref(p_f90), C.byref(p_work), 0, E, sp), "caar_layout_from_f90")
    L.check(lib.caar_launch(C.byref(dims), C.byref(p_work), dvv, C.byref(prm), sp), "caar_launch")
    L.check(lib.caar_layout_to_f90(C.byref(dims), C.byref(p_work), C.byref(p_f90), 0, E, 0, sp), "caar_layout_to_f90")


def block_ms(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(n):
        fn()
    e1.record(st)
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) / n


arms = {"a": arm_a, "b": arm_b, "c": arm_c}
for fn in arms.values():      # warm-up: clocks, TLBs, the cache window
    block_ms(fn, 2 * a.calls)
ms = {k: [] for k in arms}
for _ in range(a.rounds):
    for k, fn in arms.items():
        fn()                  # one untimed call: the block starts from its own arrays' cache state
        ms[k].append(block_ms(fn, a.calls))

balg = tsa.algorithmic_bytes(np_, nlev) * E
best = {k: min(v) for k, v in ms.items()}
out = {"np": np_, "nlev": nlev, "elems": E, "calls_per_block": a.calls, "rounds": a.rounds,
       "ms_cpp": best["a"], "ms_f90": best["b"], "ms_convert": best["c"],
       "median_ms_cpp": statistics.median(ms["a"]), "median_ms_f90": statistics.median(ms["b"]),
       "median_ms_convert": statistics.median(ms["c"]),
       "b_over_a": best["b"] / best["a"], "c_over_b": best["c"] / best["b"],
       "algorithmic_bytes": balg, "frac_cpp": balg / (best["a"] * 1e-3) / 8e12, "frac_f90": balg / (best["b"] * 1e-3) / 8e12,
       "kernel_cpp": lib.caar_kernel_name(np_, nlev).decode(), "cache_window": lib.caar_get_cache_window()}
print(json.dumps(out))
