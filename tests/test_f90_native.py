"""CPU-side tests of compute_and_apply_rhs on Fortran-ordered arrays (include/caar_f90.h, csrc/caar_f90.hip): the header,
the exported and bound symbols, argument validation (nothing here touches a device), the kernels the code object holds,
and the Fortran host module and program."""
import ctypes as C
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

import tinman_sandbox_amd as tsa
from tinman_sandbox_amd import build as tbuild
from tinman_sandbox_amd import caar as m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tinman_sandbox_amd", "csrc")


@pytest.fixture(scope="module")
def lib():
    tbuild.build_library()
    return tsa.library()


def _declared(header):
    hdr = open(os.path.join(ROOT, "include", header)).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return set(re.findall(r"\b(caar_[a-z_0-9]+)\s*\(", hdr))


def test_header_declares_what_the_library_exports_and_python_binds(lib):
    declared = _declared("caar_f90.h")
    assert declared == {"caar_launch_f90", "caar_launch_steps_f90"}
    assert declared == set(m.CaarLibrary.F90_SYMBOLS)
    # additive: not part of the frozen boundary or the tuning header
    assert not declared & (set(m.CaarLibrary.BOUNDARY_SYMBOLS) | set(m.CaarLibrary.TUNING_SYMBOLS))
    assert not declared & (_declared("caar.h") | _declared("caar_tuning.h"))
    for s in declared:
        assert hasattr(lib.lib, s), s
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(CSRC, "libcaar_hip.so")], check=True,
                        capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (caar_[a-z_0-9]+)\b", nm))
    assert declared <= exported, sorted(declared - exported)


@pytest.mark.parametrize("with_caar_h", [False, True])
def test_header_is_plain_c_and_links(tmp_path, lib, with_caar_h):
    """C99, -Wall -Wextra -Werror, on its own and after caar.h; links against libcaar_hip.so and refuses a bad call before
    touching a device."""
    src = tmp_path / "f90_probe.c"
    src.write_text(("#include \"caar.h\"\n" if with_caar_h else "") + r'''
#include "caar_f90.h"
int main(void) {
  CaarDims d = {4, 72, 1, 3, 10};
  CaarParams p = {0};
  CaarArrays a = {0};
  p.rsplit = 1;
  p.nete = 11; /* > num_elems */
  if (caar_launch_f90(&d, &a, 0, &p, 0) != CAAR_EINVAL) return 1;
  if (caar_launch_steps_f90(&d, &a, 0, &p, 0, 1, 0) != CAAR_EINVAL) return 2;
  return 0;
}
''')
    exe = tmp_path / "f90_probe"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src),
                    "-L" + CSRC, "-lcaar_hip", "-Wl,-rpath," + CSRC, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    subprocess.run([str(exe)], check=True)


def _params(nets=0, nete=4, rsplit=1):
    return m._CaarParams(nets, nete, 0, 1, 2, 0, 1.0, 1.0, 1.0, 461.5, 287.04, 0.28, 10.0, 73.0, None, rsplit, None, None)


def test_launch_f90_validates_without_touching_a_device(lib):
    L = lib.lib
    fake = m._CaarArrays(*[C.cast(8, m._dp)] * 16)          # 8-byte aligned is enough in Fortran order
    dvv = C.c_void_p(64)
    dims = m._CaarDims(4, 72, 1, 3, 4)
    assert L.caar_launch_f90(C.byref(dims), C.byref(m._CaarArrays()), dvv, C.byref(_params()), None) == -1   # null arrays
    assert L.caar_launch_f90(C.byref(dims), C.byref(fake), dvv, C.byref(_params(nete=5)), None) == -1        # nete > num_elems
    assert L.caar_launch_f90(C.byref(dims), C.byref(fake), None, C.byref(_params()), None) == -1             # no Dvv
    assert L.caar_launch_f90(None, None, None, None, None) == -1
    odd = m._CaarArrays(*[C.cast(8, m._dp)] * 15 + [C.cast(12, m._dp)])  # not 8-byte aligned
    assert L.caar_launch_f90(C.byref(dims), C.byref(odd), dvv, C.byref(_params()), None) == -1
    assert L.caar_launch_f90(C.byref(m._CaarDims(6, 72, 1, 3, 4)), C.byref(fake), dvv, C.byref(_params()), None) == -2
    assert L.caar_launch_f90(C.byref(dims), C.byref(fake), dvv, C.byref(_params(rsplit=0)), None) == -2      # Eulerian
    assert L.caar_launch_f90(C.byref(m._CaarDims(4, 257, 1, 3, 4)), C.byref(fake), dvv, C.byref(_params()), None) == -2
    assert L.caar_launch_f90(C.byref(m._CaarDims(8, 128, 1, 3, 4)), C.byref(fake), dvv, C.byref(_params()), None) == -2
    # an empty range is a no-op (nothing enqueued, no device needed)
    assert L.caar_launch_f90(C.byref(dims), C.byref(fake), dvv, C.byref(_params(nets=2, nete=2)), None) == 0
    for nsteps in (0, -3):
        assert L.caar_launch_steps_f90(C.byref(dims), C.byref(fake), dvv, C.byref(_params()), nsteps, 1, None) == -1
    assert L.caar_launch_steps_f90(C.byref(dims), C.byref(fake), dvv, C.byref(_params(rsplit=0)), 3, 1, None) == -2
    assert L.caar_launch_steps_f90(C.byref(m._CaarDims(6, 72, 1, 3, 4)), C.byref(fake), dvv, C.byref(_params()), 3, 1,
                                   None) == -2


def test_python_entry_points_refuse_cpu_arrays():
    from tinman_sandbox_amd import f90_layout as fl
    f90 = fl.F90Arrays(4, 72, 2, device="cpu")
    d = tsa.TestData().init_data(2, 4, 72, device="cpu")
    with pytest.raises(m.CaarError, match="no CPU fallback"):
        fl.compute_and_apply_rhs(f90, d)
    with pytest.raises(m.CaarError, match="no CPU fallback"):
        fl.compute_and_apply_rhs_steps(f90, d, 3)


def test_code_object_holds_the_fortran_order_kernels():
    """caar_np4_f90_kernel at NLEV 72, 128 and the run-time level count, and caar_np8_f90_kernel at 72, moist and dry:
    each within 256 VGPRs (two workgroups per CU where the twin has two) and free of register spills."""
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf") or shutil.which("c++filt") is None:
        pytest.skip("llvm-readelf / c++filt not available")
    tbuild.build_library()
    spec = importlib.util.spec_from_file_location("codeobj_stats", os.path.join(ROOT, "tools", "codeobj_stats.py"))
    cs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cs)
    kernels = [k for _, blob in cs.code_objects(os.path.join(CSRC, "libcaar_hip.so")) for k in cs.kernels_of(blob)]
    f90 = [k for k in kernels if "_f90_kernel<" in k.get("name", "")]
    for prefix in ("caar_np4_f90_kernel<72, ", "caar_np4_f90_kernel<128, ", "caar_np4_f90_kernel<0, ", "caar_np8_f90_kernel<72, "):
        for moist in ("true", "false"):
            assert any(k["name"].startswith(prefix) and (", %s, " % moist) in k["name"] for k in f90), (prefix, moist)
    assert len([k for k in f90 if "np4" in k["name"]]) == 18 and len([k for k in f90 if "np8" in k["name"]]) == 2
    for k in f90:
        assert k["vgprs"] <= 256 and k["vgpr_spills"] == 0 and k["scratch_bytes"] == 0, k


def test_fortran_module_and_resident_program_compile(tmp_path):
    exe = tbuild.build_fortran_resident()
    if exe is None:
        pytest.skip("flang not available")
    assert os.access(exe, os.X_OK)
    # the device module binds what the new header declares, and the frozen module stays within caar.h
    mod = open(os.path.join(ROOT, "tinman_sandbox_amd", "host", "fortran", "caar_device_mod.F90")).read()
    bound = set(re.findall(r'bind\(C,\s*name="(caar_[a-z_0-9]+)"\)', mod))
    assert _declared("caar_f90.h") <= bound and bound <= _declared("caar_f90.h") | _declared("caar.h"), sorted(bound)
    nm = subprocess.run(["nm", "--undefined-only", exe], check=True, capture_output=True, text=True).stdout
    assert "caar_launch_f90" in nm and "caar_arrays_alloc" in nm and "hipMemcpy" in nm
