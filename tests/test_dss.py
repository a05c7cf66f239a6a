"""CPU-side tests of the direct stiffness summation (include/caar_dss.h, csrc/caar_dss.hip): the header and the exported and
bound symbols, the meshes of tinman_sandbox_amd.mesh, the numpy restatement (tests/dss_ref.py) and its invariants, the
host-side plan analysis and argument checks (host-only plans touch no device), the kernels the code object holds, and the
Fortran module."""
import ctypes as C
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import dss_ref
import tinman_sandbox_amd as tsa
from tinman_sandbox_amd import build as tbuild
from tinman_sandbox_amd import caar as m
from tinman_sandbox_amd import mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tinman_sandbox_amd", "csrc")
EINVAL, EUNSUPPORTED, ENODEVICE = -1, -2, -3


@pytest.fixture(scope="module")
def lib():
    tbuild.build_library()
    return tsa.library()


def _declared(header):
    hdr = open(os.path.join(ROOT, "include", header)).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return set(re.findall(r"\b(caar_[a-z_0-9]+)\s*\(", hdr))


def test_header_declares_what_the_library_exports_and_python_binds(lib):
    declared = _declared("caar_dss.h")
    assert declared == set(m.CaarLibrary.DSS_SYMBOLS)
    assert set(m.CaarLibrary.DSS_SYMBOLS) <= set(m.CaarLibrary.SYMBOLS)
    for other in ("caar.h", "caar_tuning.h", "caar_f90.h"):
        assert not declared & _declared(other), other
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(CSRC, "libcaar_hip.so")], check=True,
                        capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (caar_[a-z_0-9]+)\b", nm))
    assert declared <= exported, sorted(declared - exported)


@pytest.mark.parametrize("with_caar_h", [False, True])
def test_header_is_plain_c_and_links(tmp_path, lib, with_caar_h):
    """C99, -Wall -Wextra -Werror, on its own and after caar.h; a host-only plan over a 1x1 periodic plane is analysed and a
    bad launch is refused before any device is touched."""
    src = tmp_path / "dss_probe.c"
    src.write_text(("#include \"caar.h\"\n" if with_caar_h else "") + r'''
#include "caar_dss.h"
int main(void) {
  CaarDims d = {4, 72, 1, 3, 1};
  CaarArrays a = {0};
  long long g[16] = {0, 1, 2, 0, 3, 4, 5, 3, 6, 7, 8, 6, 0, 1, 2, 0};
  long long u = 0, s = 0, o = -1;
  int mx = 0;
  CaarDssPlan *p = 0;
  if (caar_dss_plan_create(&p, &d, g, CAAR_DSS_LAYOUT_CXX, -1) != CAAR_OK || !p) return 1;
  if (caar_dss_plan_info(p, &u, &s, &o, &mx) != CAAR_OK || u != 9 || s != 5 || o != 0 || mx != 4) return 2;
  if (caar_dss_launch(p, &d, CAAR_DSS_LAYOUT_CXX, &a, 1, 0, 0) != CAAR_EINVAL) return 3;
  caar_dss_plan_destroy(p);
  g[5] = -1;
  if (caar_dss_plan_create(&p, &d, g, CAAR_DSS_LAYOUT_CXX, -1) != CAAR_EINVAL || p) return 4;
  return CAAR_DSS_MAX_SHARERS == 8 ? 0 : 5;
}
''')
    exe = tmp_path / "dss_probe"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src),
                    "-L" + CSRC, "-lcaar_hip", "-Wl,-rpath," + CSRC, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    subprocess.run([str(exe)], check=True)


@pytest.mark.parametrize("ne", [1, 2, 3, 5])
@pytest.mark.parametrize("np_", [4, 8])
def test_cubed_sphere_mesh(lib, ne, np_):
    g = mesh.cubed_sphere_gdof(ne, np_)
    assert g.shape == (6 * ne * ne, np_, np_) and g.dtype == np.int64
    assert len(np.unique(g)) == 6 * ne * ne * (np_ - 1) ** 2 + 2
    n = dss_ref.sharer_counts(g)
    corner = np.zeros((np_, np_), dtype=bool)
    corner[[0, 0, -1, -1], [0, -1, 0, -1]] = True
    edge = np.zeros((np_, np_), dtype=bool)
    edge[[0, -1], :] = edge[:, [0, -1]] = True
    edge &= ~corner
    ids3 = np.unique(g[n == 3])
    assert len(ids3) == 8 and np.all(n[:, corner] >= 3)
    assert np.sum(n[:, corner] == 4) == n[:, corner].size - 8 * 3
    assert np.all(n[:, edge] == 2) and np.all(n[:, 1:-1, 1:-1] == 1)
    info = tsa.DssPlan(g, 72, device="host").info()
    assert info == dss_ref.info(g)
    assert info["open_points"] == 0 and info["max_sharers"] == (3 if ne == 1 else 4)


@pytest.mark.parametrize("nx,ny", [(1, 1), (1, 3), (5, 4)])
def test_periodic_plane_mesh(lib, nx, ny):
    g = mesh.periodic_plane_gdof(nx, ny, 4)
    assert len(np.unique(g)) == nx * ny * 9
    n = dss_ref.sharer_counts(g)
    assert np.all(n[:, [0, 0, -1, -1], [0, -1, 0, -1]] == 4) and np.all(n[:, 1:-1, 1:-1] == 1)
    assert np.all(n[:, 0, 1:-1] == 2) and np.all(n[:, 1:-1, -1] == 2)
    info = tsa.DssPlan(g, 17, device="host").info()
    assert info == dss_ref.info(g) and info["open_points"] == 0


def test_slab_of_a_sphere_has_open_points(lib):
    g = mesh.cubed_sphere_gdof(4, 4)
    for a, b in ((0, 16), (20, 50), (95, 96)):
        info = tsa.DssPlan(g[a:b], 72, device="host").info()
        assert info == dss_ref.info(g[a:b]) and info["open_points"] > 0
    # one element: its whole boundary is open
    assert dss_ref.info(g[7:8])["open_points"] == 12


def test_inverse_mass_is_continuous_and_in_contract_order():
    rng = np.random.default_rng(3)
    g = mesh.cubed_sphere_gdof(3, 4)
    w = rng.uniform(0.1, 1.0, size=g.shape)
    r = mesh.inverse_mass(g, w)
    order, starts, counts, group_of = dss_ref.groups(g)
    rf = r.reshape(-1)
    assert np.array_equal(rf, rf[order[starts]][group_of])      # every copy bitwise equal
    S = dss_ref.sum_copies(w.reshape(-1, 1), g)[:, 0]
    assert np.array_equal(rf, (1.0 / S)[group_of])
    # a corner: three sharers summed left to right from the first
    q = np.flatnonzero(counts == 3)[0]
    i = order[starts[q]:starts[q] + 3]
    assert rf[i[0]] == 1.0 / ((w.reshape(-1)[i[0]] + w.reshape(-1)[i[1]]) + w.reshape(-1)[i[2]])


@pytest.mark.parametrize("np_", [4, 8])
def test_restatement_invariants(np_):
    """Copies bitwise equal; DSS(spheremp * f) == f for a continuous f; sum over unique points of (sum spheremp) * out ==
    sum of x over all copies."""
    rng = np.random.default_rng(11)
    g = mesh.cubed_sphere_gdof(4, np_)
    nlev = 9
    w = rng.uniform(0.1, 1.0, size=g.shape)
    r = mesh.inverse_mass(g, w)
    order, starts, counts, group_of = dss_ref.groups(g)
    x = dss_ref.scaled_random((g.shape[0], nlev, np_, np_), rng, (0, 1))
    out = dss_ref.dss_field(x, g, r)
    P = out.transpose(0, 2, 3, 1).reshape(-1, nlev)
    assert np.array_equal(P, P[order[starts]][group_of])
    f = rng.uniform(-1.0, 1.0, size=(counts.size, nlev)) * 10.0 ** rng.integers(-3, 4, size=(1, nlev))
    fc = f[group_of].reshape(g.shape[0], np_, np_, nlev).transpose(0, 3, 1, 2)
    back = dss_ref.dss_field(w[:, None] * fc, g, r)
    assert np.all(np.abs(back - fc) <= 1e-15 * np.abs(fc))
    W = dss_ref.sum_copies(w.reshape(-1, 1), g)
    lhs = np.sum(W * P[order[starts]], axis=0)
    rhs = np.sum(x, axis=(0, 2, 3))
    assert np.all(np.abs(lhs - rhs) <= 1e-14 * np.sum(np.abs(x), axis=(0, 2, 3)))


def test_plan_create_refuses_bad_meshes(lib):
    L = lib.lib
    g = mesh.cubed_sphere_gdof(2, 4)

    def create(gd, np_=4, nlev=72, layout=0, ne=None):
        plan = C.c_void_p()
        gd = np.ascontiguousarray(gd, dtype=np.int64)
        dims = m._CaarDims(np_, nlev, 1, 3, gd.shape[0] if ne is None else ne)
        rc = L.caar_dss_plan_create(C.byref(plan), C.byref(dims), gd.ctypes.data_as(C.c_void_p), layout, -1)
        if plan.value:
            L.caar_dss_plan_destroy(plan)
        return rc, plan.value

    assert create(g)[0] == 0
    bad = g.copy()
    bad[3, 0, 2] = -5
    assert create(bad) == (EINVAL, None)                                   # negative id

    def with_copies(k):  # k more elements with element 0's boundary (and interior points of their own)
        extra = np.repeat(g[:1], k, axis=0)
        extra[:, 1:-1, 1:-1] = 10 ** 6 + np.arange(k * 4).reshape(k, 2, 2)
        return np.concatenate([g, extra])

    # element 0's 4-sharer corners reach 8 sharers with four copies, 9 with five
    assert create(with_copies(4))[0] == 0 and dss_ref.info(with_copies(4))["max_sharers"] == 8
    assert create(with_copies(5)) == (EUNSUPPORTED, None)
    inner = g.copy()
    inner[0, 1, 1] = inner[1, 1, 1]                                        # an interior point shared
    assert create(inner) == (EINVAL, None)
    assert create(g, np_=6) == (EUNSUPPORTED, None) and create(g, nlev=1) == (EUNSUPPORTED, None)
    assert create(g, layout=2) == (EINVAL, None) and create(g, ne=-1) == (EINVAL, None)
    dims = m._CaarDims(4, 72, 1, 3, 4)
    assert L.caar_dss_plan_create(None, C.byref(dims), g.ctypes.data_as(C.c_void_p), 0, -1) == EINVAL
    plan = C.c_void_p()
    assert L.caar_dss_plan_create(C.byref(plan), C.byref(dims), None, 0, -1) == EINVAL and not plan.value
    assert L.caar_dss_plan_info(None, None, None, None, None) == EINVAL
    with pytest.raises(m.CaarError, match="caar_dss_plan_create"):
        tsa.DssPlan(bad, 72, device="host")


def test_launch_validates_without_touching_a_device(lib):
    L = lib.lib
    g = mesh.cubed_sphere_gdof(1, 4)
    plan = tsa.DssPlan(g, 72, device="host")
    fake = m._CaarArrays(*[C.cast(64, m._dp)] * 16)
    rs = C.c_void_p(64)
    h = plan.handle

    def launch(dims=None, layout=0, arrays=fake, tl=1, r=rs, p=h):
        d = m._CaarDims(4, 72, 1, 3, 6) if dims is None else dims
        return L.caar_dss_launch(p, C.byref(d), layout, C.byref(arrays) if arrays is not None else None, tl, r, None)

    assert launch() == ENODEVICE                                   # valid arguments, host-only plan
    assert launch(p=None) == EINVAL and launch(arrays=None) == EINVAL and launch(r=None) == EINVAL
    assert launch(arrays=m._CaarArrays()) == EINVAL
    for dims in (m._CaarDims(4, 72, 1, 3, 5), m._CaarDims(4, 71, 1, 3, 6), m._CaarDims(8, 72, 1, 3, 6),
                 m._CaarDims(4, 72, 1, 0, 6)):
        assert launch(dims=dims) == EINVAL
    assert launch(layout=1) == EINVAL and launch(layout=7) == EINVAL
    assert launch(tl=3) == EINVAL and launch(tl=-1) == EINVAL
    assert launch(dims=m._CaarDims(4, 72, 1, 4, 6), tl=3) == ENODEVICE
    odd = m._CaarArrays(*[C.cast(64, m._dp)] * 8 + [C.cast(68, m._dp)] + [C.cast(64, m._dp)] * 7)   # T not 8-byte aligned
    assert launch(arrays=odd) == EINVAL and launch(r=C.c_void_p(60)) == EINVAL
    plan.close()
    plan.close()


def test_python_entry_points_refuse_cpu_arrays(lib):
    from tinman_sandbox_amd import f90_layout as fl
    g = mesh.cubed_sphere_gdof(1, 4)
    plan = tsa.DssPlan(g, 72, device="host")
    d = tsa.TestData().init_data(6, 4, 72, device="cpu")
    import torch
    r = torch.ones(6, 4, 4, dtype=torch.float64)
    with pytest.raises(m.CaarError, match="no CPU fallback"):
        tsa.dss(d, plan, r)
    with pytest.raises(m.CaarError, match="no CPU fallback"):
        fl.dss(fl.F90Arrays(4, 72, 6, device="cpu"), plan, r, 1)


def test_code_object_holds_the_dss_kernels():
    """caar_dss_pack / caar_dss_unpack for NP 4 and 8 in both layouts, none spilling or using scratch."""
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf") or shutil.which("c++filt") is None:
        pytest.skip("llvm-readelf / c++filt not available")
    tbuild.build_library()
    spec = importlib.util.spec_from_file_location("codeobj_stats", os.path.join(ROOT, "tools", "codeobj_stats.py"))
    cs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cs)
    kernels = [k for _, blob in cs.code_objects(os.path.join(CSRC, "libcaar_hip.so")) for k in cs.kernels_of(blob)]
    dss = [k for k in kernels if k.get("name", "").startswith("caar_dss_")]
    names = {k["name"] for k in dss}
    for kind in ("pack", "unpack"):
        for np_ in (4, 8):
            for f90 in ("false", "true"):
                assert "caar_dss_%s<%d, %s>" % (kind, np_, f90) in names, (kind, np_, f90)
    assert len(dss) == 8
    for k in dss:
        assert "caar_np" not in k["name"] and "_f90_kernel<" not in k["name"]
        assert k["vgpr_spills"] == 0 and k["scratch_bytes"] == 0, k


def test_fortran_module_compiles(tmp_path):
    if not os.path.exists(tbuild.FLANG):
        pytest.skip("flang not available")
    fdir = os.path.join(ROOT, "tinman_sandbox_amd", "host", "fortran")
    subprocess.run([tbuild.FLANG, "-c", "-module-dir", str(tmp_path), os.path.join(fdir, "caar_mod.F90"),
                    os.path.join(fdir, "caar_dss_mod.F90")], check=True, cwd=str(tmp_path), capture_output=True)
    assert (tmp_path / "caar_dss_mod.mod").exists()
    mod = open(os.path.join(fdir, "caar_dss_mod.F90")).read()
    bound = set(re.findall(r'bind\(C,\s*name="(caar_[a-z_0-9]+)"\)', mod))
    assert bound == _declared("caar_dss.h")
