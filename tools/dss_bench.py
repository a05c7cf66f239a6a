#!/usr/bin/env python3
"""The direct stiffness summation of the new time level (include/caar_dss.h) beside the call it follows, in a FRESH process
per configuration.  Prints one JSON line per configuration.

    python tools/dss_bench.py --np 4 --nlev 72 --ne 41 --order face     # one configuration
    python tools/dss_bench.py                                           # the three sizes, face-major and random element
                                                                        # order, each in a fresh child process

A cubed sphere of 6*ne^2 elements (tinman_sandbox_amd.mesh), C++ layout from the library's allocator, the reference's
closed-form initialiser.  --order random permutes the elements (mesh and arrays alike).  Arms, alternated block by block
(HIP events on the launch stream; the adaptive window is off): (a) caar_launch alone, (b) the DSS alone (caar_dss_launch:
pack + unpack), (c) caar_launch + DSS.  After a warm-up, --rounds rounds of one block of --calls calls per arm; the figure
per arm is the best block (ms per call), the median block next to it.  B_dss = 8*(8*nlev*np^2 + np^2) bytes per element:
np1 of T, u, v, dp3d read once and written once, plus rspheremp."""
import argparse
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = ((4, 72, 41), (4, 128, 46), (8, 72, 58))   # 10 086, 12 696 and 20 184 elements

ap = argparse.ArgumentParser()
ap.add_argument("--np", type=int, dest="np_")
ap.add_argument("--nlev", type=int)
ap.add_argument("--ne", type=int)
ap.add_argument("--order", choices=("face", "random"), default="face")
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--rounds", type=int, default=7)
a = ap.parse_args()

if a.np_ is None:
    for np_, nlev, ne in CONFIGS:
        for order in ("face", "random"):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--np", str(np_), "--nlev", str(nlev), "--ne",
                                str(ne), "--order", order, "--calls", str(a.calls), "--rounds", str(a.rounds)],
                               capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                sys.exit(r.returncode)
            print(r.stdout.strip().splitlines()[-1], flush=True)
    sys.exit(0)

import ctypes as C  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

import tinman_sandbox_amd as tsa  # noqa: E402
from tinman_sandbox_amd import mesh  # noqa: E402

L = tsa.library()
lib = L.lib
dev = torch.device("cuda", 0)
st = torch.cuda.current_stream(dev)
lib.caar_set_adaptive_window(0)

np_, nlev = a.np_, a.nlev
gdof = mesh.cubed_sphere_gdof(a.ne, np_)
E = gdof.shape[0]
if a.order == "random":
    gdof = gdof[np.random.default_rng(1).permutation(E)]
data = tsa.TestData().init_data(E, np_, nlev, device=dev)
sph = data.arrays["elem_spheremp"].cpu().numpy()
rsph = torch.from_numpy(mesh.inverse_mass(gdof, sph)).to(dev)
plan = tsa.DssPlan(gdof, nlev, "cxx", dev)
torch.cuda.synchronize(dev)

dims, prm, ptrs = data.arrays.dims(), data.params(device_constants=True), data.arrays.pointers()
dvv = C.c_void_p(data.dvv_device().data_ptr())
sp = C.c_void_p(st.cuda_stream)
tl = data.control.np1


def arm_a():
    L.check(lib.caar_launch(C.byref(dims), C.byref(ptrs), dvv, C.byref(prm), sp), "caar_launch")


def arm_b():
    L.check(lib.caar_dss_launch(plan.handle, C.byref(dims), 0, C.byref(ptrs), tl, C.c_void_p(rsph.data_ptr()), sp),
            "caar_dss_launch")


def arm_c():
    arm_a()
    arm_b()


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

b_dss = 8 * (8 * nlev * np_ * np_ + np_ * np_) * E
best = {k: min(v) for k, v in ms.items()}
info = plan.info()
out = {"np": np_, "nlev": nlev, "ne": a.ne, "elems": E, "order": a.order, "calls_per_block": a.calls, "rounds": a.rounds,
       "ms_caar": best["a"], "ms_dss": best["b"], "ms_caar_dss": best["c"],
       "median_ms_caar": statistics.median(ms["a"]), "median_ms_dss": statistics.median(ms["b"]),
       "median_ms_caar_dss": statistics.median(ms["c"]),
       "dss_over_caar": best["b"] / best["a"], "b_dss": b_dss, "dss_tb_s": b_dss / (best["b"] * 1e-3) / 1e12,
       "dss_frac_8tb": b_dss / (best["b"] * 1e-3) / 8e12, "edge_buffer_mb": E * 4 * (np_ - 1) * 4 * nlev * 8 / 1e6,
       "shared_points": info["shared_points"], "kernel_caar": lib.caar_kernel_name(np_, nlev).decode()}
plan.close()
print(json.dumps(out))
