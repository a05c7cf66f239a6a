#!/usr/bin/env python3
"""HBM-side bytes of the direct stiffness summation (include/caar_dss.h), from two rocprofv3 counter passes.

    rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d out_fetch -- python3 tools/pmc_dss.py --np 4 --nlev 72 --ne 41
    rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d out_write -- python3 tools/pmc_dss.py --np 4 --nlev 72 --ne 41
    python3 tools/pmc_dss.py --parse out_fetch out_write --np 4 --nlev 72 --ne 41     # one JSON line

The workload: three launches of the 8 B/lane stream copy (1 GiB each way: the known byte count each counter is calibrated
on, as for profiles/hbm_traffic.json, tools/pmc_parse.py), then five DSS launches (caar_dss_pack + caar_dss_unpack) on a
face-major cubed sphere of 6*ne^2 elements.  The parse step reports each kernel's calibrated read and write bytes per launch
and per element, and their sum per element against B_dss = 8*(8*nlev*np^2 + np^2)."""
import argparse
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--np", type=int, default=4, dest="np_")
ap.add_argument("--nlev", type=int, default=72)
ap.add_argument("--ne", type=int, default=41)
ap.add_argument("--parse", nargs=2, metavar=("FETCH_DIR", "WRITE_DIR"))
a = ap.parse_args()
N_COPY = 1 << 27


def load(d, counter):
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if r.get("Counter_Name") == counter:
                rows.append((r["Kernel_Name"], float(r["Counter_Value"]) * 1024))   # KiB
    return rows


def mean(xs):
    xs = list(xs)
    return sum(xs) / len(xs) if xs else float("nan")


if a.parse:
    E = 6 * a.ne * a.ne
    b_dss = 8 * (8 * a.nlev * a.np_ ** 2 + a.np_ ** 2)
    out = {"np": a.np_, "nlev": a.nlev, "ne": a.ne, "elems": E, "b_dss_per_element": b_dss}
    total = 0.0
    for counter, d, key in (("FETCH_SIZE", a.parse[0], "read"), ("WRITE_SIZE", a.parse[1], "write")):
        rows = load(d, counter)
        copy = mean(v for k, v in rows if "stream_copy_kernel<double>" in k)
        factor = N_COPY * 8 / copy
        out["factor_%s" % counter] = factor
        for kern in ("pack", "unpack"):
            vals = [v for k, v in rows if "caar_dss_%s<" % kern in k]
            per_launch = mean(vals) * factor
            out["%s_%s_bytes_per_launch" % (kern, key)] = per_launch
            out["%s_%s_bytes_per_element" % (kern, key)] = per_launch / E
            out["%s_launches" % kern] = len(vals)
            total += per_launch / E
    out["hbm_bytes_per_element"] = total
    out["ratio_to_b_dss"] = total / b_dss
    out["method"] = ("rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE in separate passes (KiB), each calibrated on the 8 B/lane "
                     "stream copy of the same run (1 GiB each way); counts what leaves and enters the L2s")
    print(json.dumps(out))
    sys.exit(0)

import ctypes as C  # noqa: E402

import torch  # noqa: E402

import tinman_sandbox_amd as tsa  # noqa: E402
from tinman_sandbox_amd import mesh  # noqa: E402

L = tsa.library()
lib = L.lib
dev = torch.device("cuda", 0)
st = torch.cuda.current_stream(dev)
src = torch.ones(N_COPY, dtype=torch.float64, device=dev)
dst = torch.empty_like(src)
for _ in range(3):
    L.check(lib.caar_stream_copy(C.c_void_p(dst.data_ptr()), C.c_void_p(src.data_ptr()), N_COPY, 8,
                                 C.c_void_p(st.cuda_stream)), "copy")
torch.cuda.synchronize()
del src, dst
gdof = mesh.cubed_sphere_gdof(a.ne, a.np_)
data = tsa.TestData().init_data(gdof.shape[0], a.np_, a.nlev, device=dev)
rsph = torch.from_numpy(mesh.inverse_mass(gdof, data.arrays["elem_spheremp"].cpu().numpy())).to(dev)
plan = tsa.DssPlan(gdof, a.nlev, "cxx", dev)
for _ in range(5):
    tsa.dss(data, plan, rsph)
torch.cuda.synchronize()
plan.close()
print("pmc_dss done: %d elements" % gdof.shape[0])
