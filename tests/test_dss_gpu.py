"""The direct stiffness summation on the MI355X (include/caar_dss.h, csrc/caar_dss.hip) against the numpy restatement
(tests/dss_ref.py): bit for bit on small meshes and on every element at the benchmark sizes, its invariants, what it must
leave alone, bad input, a plan over a slab, a captured step of caar_launch + DSS against the oracle, and a speed guard."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cases
import dss_ref
import tinman_sandbox_amd as tsa
from tinman_sandbox_amd import caar as m
from tinman_sandbox_amd import f90_layout as fl
from tinman_sandbox_amd import mesh

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE = dss_ref.STATE

MESHES = {"sphere1": lambda np_: mesh.cubed_sphere_gdof(1, np_), "sphere2": lambda np_: mesh.cubed_sphere_gdof(2, np_),
          "sphere3": lambda np_: mesh.cubed_sphere_gdof(3, np_), "plane1x1": lambda np_: mesh.periodic_plane_gdof(1, 1, np_),
          "plane1x3": lambda np_: mesh.periodic_plane_gdof(1, 3, np_),
          "plane5x4": lambda np_: mesh.periodic_plane_gdof(5, 4, np_)}
# NP=4 85 levels fill the 32 KiB LDS image exactly (12 x (4*85 + 1) x 8 B); 87, 129 and 200 end on a shorter pass
# (44 + 43, 65 + 64, 67 + 67 + 66 levels): an overrun past nlev there would land in the next time level
SHAPES = ((4, 72), (4, 128), (4, 17), (4, 2), (8, 72), (4, 85), (4, 87), (4, 129), (4, 200))


def _sparse(gdof):
    """The same mesh with non-dense ids."""
    return gdof * 1000003 + (1 << 40)


def _run(gdof, np_, nlev, timelevels, tl, layout, seed, rsph=None, state=None, fill_all=False):
    """One DSS on the GPU of random (or given) state in `layout`; returns (inputs, outputs, rsph), C++-layout numpy arrays of
    the state (of all 16 arrays with fill_all: every array random)."""
    ne = gdof.shape[0]
    rng = np.random.default_rng(seed + 7)
    if rsph is None:
        rsph = mesh.inverse_mass(gdof, rng.uniform(0.1, 1.0, size=gdof.shape))
    arrs = dict(state if state is not None else dss_ref.random_state(np_, nlev, ne, timelevels, seed))
    if fill_all:
        for n, sh in tsa.array_shapes(np_, nlev, 1, timelevels, ne).items():
            if n not in STATE:
                arrs[n] = rng.standard_normal(sh)
    plan = tsa.DssPlan(gdof, nlev, layout)
    if layout == "cxx":
        ea = tsa.ElementArrays(np_, nlev, ne, 1, timelevels, "cuda", place="torch")
        for n, x in arrs.items():
            ea[n].copy_(torch.from_numpy(x))
        tsa.dss(ea, plan, torch.from_numpy(rsph).cuda(), tl=tl)
        torch.cuda.synchronize()
        out = {n: ea[n].cpu().numpy() for n in arrs}
    else:
        f90 = fl.F90Arrays(np_, nlev, ne, 1, timelevels, "cuda")
        for n, x in fl.to_f90_numpy(arrs).items():
            f90.t[n].copy_(torch.from_numpy(x))
        fl.dss(f90, plan, torch.from_numpy(np.ascontiguousarray(rsph.transpose(0, 2, 1))).cuda(), tl)
        torch.cuda.synchronize()
        out = fl.from_f90_numpy({n: f90.t[n].cpu().numpy() for n in arrs})
    plan.close()
    return arrs, out, rsph


def _check_exact(arrs, out, gdof, rsph, tl):
    want = dss_ref.dss_state(arrs, gdof, rsph, tl)
    for n in STATE:
        assert np.array_equal(out[n], want[n]), (n, np.argwhere(out[n] != want[n])[:5])


@pytest.mark.parametrize("layout", ["cxx", "f90"])
@pytest.mark.parametrize("np_,nlev", SHAPES)
@pytest.mark.parametrize("mesh_name", sorted(MESHES))
def test_bit_for_bit_small_meshes(mesh_name, np_, nlev, layout):
    """Natural and permuted element order, non-dense ids, tl 0/1/2 of 3 and tl 3 of 4 time levels."""
    base = MESHES[mesh_name](np_)
    i = sorted(MESHES).index(mesh_name) + SHAPES.index((np_, nlev))
    for order, (timelevels, tl) in zip(("natural", "permuted"), (((3, 0), (3, 1), (3, 2), (4, 3))[i % 4],
                                                                 ((3, 2), (4, 3), (3, 0), (3, 1))[i % 4])):
        g = base if order == "natural" else base[np.random.default_rng(i).permutation(base.shape[0])]
        g = _sparse(g)
        arrs, out, rsph = _run(g, np_, nlev, timelevels, tl, layout, seed=100 + i)
        _check_exact(arrs, out, g, rsph, tl)


@pytest.mark.parametrize("ne,np_,nlev,layout", [(41, 4, 72, "cxx"), (41, 4, 72, "f90"), (46, 4, 128, "cxx"),
                                                 (58, 8, 72, "cxx")])
def test_every_element_at_benchmark_sizes(ne, np_, nlev, layout):
    g = mesh.cubed_sphere_gdof(ne, np_)
    arrs, out, rsph = _run(g, np_, nlev, 2, 1, layout, seed=ne)
    _check_exact(arrs, out, g, rsph, 1)


@pytest.mark.parametrize("np_", [4, 8])
def test_invariants(np_):
    g = mesh.cubed_sphere_gdof(6, np_)
    nlev, tl = (24 if np_ == 4 else 72), 1   # NP=8: the one level count caar_supported has
    rng = np.random.default_rng(5)
    w = rng.uniform(0.1, 1.0, size=g.shape)
    rsph = mesh.inverse_mass(g, w)
    order, starts, counts, group_of = dss_ref.groups(g)
    # all copies bitwise equal
    arrs, out, _ = _run(g, np_, nlev, 3, tl, "cxx", seed=1, rsph=rsph)
    for n in STATE:
        for c in ((0, 1) if n == "elem_state_v" else (None,)):
            x = out[n][:, tl] if c is None else out[n][:, tl, ..., c]
            P = x.transpose(0, 2, 3, 1).reshape(-1, nlev)
            assert np.array_equal(P, P[order[starts]][group_of]), n
    # DSS(spheremp * f) == f for a continuous f
    f = rng.uniform(-1.0, 1.0, size=(counts.size, nlev)) * 10.0 ** rng.integers(-3, 4, size=(1, nlev))
    fc = f[group_of].reshape(g.shape[0], np_, np_, nlev).transpose(0, 3, 1, 2)
    st = dss_ref.random_state(np_, nlev, g.shape[0], 3, 2)
    st["elem_state_T"][:, tl] = w[:, None] * fc
    _, out2, _ = _run(g, np_, nlev, 3, tl, "cxx", seed=2, rsph=rsph, state=st)
    back = out2["elem_state_T"][:, tl]
    assert np.all(np.abs(back - fc) <= 1e-15 * np.abs(fc))
    # conservation: sum over unique points of (sum spheremp) * out == sum of x over all copies
    x = arrs["elem_state_dp3d"][:, tl]
    P = out["elem_state_dp3d"][:, tl].transpose(0, 2, 3, 1).reshape(-1, nlev)
    W = dss_ref.sum_copies(w.reshape(-1, 1), g)
    lhs = np.sum(W * P[order[starts]], axis=0)
    assert np.all(np.abs(lhs - np.sum(x, axis=(0, 2, 3))) <= 1e-14 * np.sum(np.abs(x), axis=(0, 2, 3)))


@pytest.mark.parametrize("layout", ["cxx", "f90"])
def test_nothing_else_moves(layout):
    g = mesh.cubed_sphere_gdof(2, 4)
    for timelevels, tl in ((3, 0), (4, 2)):
        arrs, out, rsph = _run(g, 4, 72, timelevels, tl, layout, seed=9, fill_all=True)
        for n in tsa.ARRAY_NAMES:
            if n in STATE:
                keep = [t for t in range(timelevels) if t != tl]
                assert np.array_equal(out[n][:, keep], arrs[n][:, keep]), n
            else:
                assert np.array_equal(out[n], arrs[n]), n
        _check_exact(arrs, out, g, rsph, tl)


def test_bad_input_leaves_the_arrays_alone():
    g = mesh.cubed_sphere_gdof(2, 4)
    ne, nlev = g.shape[0], 72
    L = tsa.library().lib
    with pytest.raises(m.CaarError, match="rc=-1"):
        tsa.DssPlan(np.where(g == 5, -2, g), nlev)                      # negative id
    extra = np.repeat(g[:1], 5, axis=0)
    extra[:, 1:-1, 1:-1] = 10 ** 6 + np.arange(20).reshape(5, 2, 2)
    with pytest.raises(m.CaarError, match="rc=-2"):
        tsa.DssPlan(np.concatenate([g, extra]), nlev)                   # 9 sharers
    arrs = {n: np.random.default_rng(1).standard_normal(s) for n, s in tsa.array_shapes(4, nlev, 1, 3, ne).items()}
    ea = tsa.ElementArrays.from_numpy(arrs, "cuda")
    rsph = torch.ones(ne, 4, 4, dtype=torch.float64, device="cuda")
    plan = tsa.DssPlan(g, nlev, "cxx")
    fplan = tsa.DssPlan(g, nlev, "f90")
    h, dims, ptrs = plan.handle, ea.dims(), ea.pointers()
    rp = C.c_void_p(rsph.data_ptr())

    def launch(p=h, d=dims, layout=0, a=ptrs, tl=1, r=rp):
        return L.caar_dss_launch(p, C.byref(d) if d is not None else None, layout, C.byref(a) if a is not None else None,
                                 tl, r, None)

    assert launch(d=m._CaarDims(4, nlev, 1, 3, ne - 1)) == -1 and launch(d=m._CaarDims(4, 128, 1, 3, ne)) == -1
    assert launch(layout=1) == -1 and launch(p=fplan.handle) == -1
    assert launch(tl=3) == -1 and launch(tl=-1) == -1
    assert launch(p=None) == -1 and launch(d=None) == -1 and launch(a=None) == -1 and launch(r=None) == -1
    assert launch(a=m._CaarArrays()) == -1
    with pytest.raises(m.CaarError, match="rc=-1"):
        tsa.dss(ea, fplan, rsph, tl=1)                                   # layout mismatch through Python
    torch.cuda.synchronize()
    after = ea.to_numpy()
    for n in tsa.ARRAY_NAMES:
        assert np.array_equal(after[n], arrs[n]), n
    plan.close()
    fplan.close()


def test_slab_plan():
    g = mesh.cubed_sphere_gdof(4, 4)
    slab = g[20:57]
    plan = tsa.DssPlan(slab, 72)
    assert plan.info() == dss_ref.info(slab) and plan.info()["open_points"] > 0
    plan.close()
    arrs, out, rsph = _run(slab, 4, 72, 3, 1, "cxx", seed=4)
    _check_exact(arrs, out, slab, rsph, 1)


def _oracle_steps(oracle, arrs, Dvv, sc, gdof, rsph, nsteps):
    want = cases.copy_arrays(arrs)
    s = dict(sc)
    for _ in range(nsteps):
        oracle.compute_and_apply_rhs(want, Dvv, s)
        want.update(dss_ref.dss_state(want, gdof, rsph, s["np1"]))
        s["np1"], s["nm1"], s["n0"] = s["nm1"], s["n0"], s["np1"]
    return want


STEP_CASES = ((4, 3, 1e-11), (41, 1, 1e-12))   # (ne, steps, tolerance against the oracle's trajectory)


def _step_case(oracle, ne, nsteps):
    g = mesh.cubed_sphere_gdof(ne, 4)
    arrs = cases.hashed_arrays(4, 72, g.shape[0], seed=ne)
    Dvv, sc = cases.dvv_for(4), oracle_scalars()
    rsph = mesh.inverse_mass(g, arrs["elem_spheremp"])
    return g, arrs, Dvv, sc, rsph, _oracle_steps(oracle, arrs, Dvv, sc, g, rsph, nsteps)


def _run_steps(nsteps, step):
    """`step()` nsteps times: captured in one graph and replayed once if there are several, directly otherwise."""
    if nsteps > 1:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(nsteps):
                step()
        graph.replay()
    else:
        step()
    torch.cuda.synchronize()


def _cxx_steps(g, arrs, Dvv, sc, rsph, nsteps):
    data = tsa.TestData.from_numpy(arrs, Dvv, sc, device="cuda")
    data.dvv_device()
    r = torch.from_numpy(rsph).cuda()
    plan = tsa.DssPlan(g, 72)

    def step():
        tsa.compute_and_apply_rhs(data)
        tsa.dss(data, plan, r)
        data.update_time_levels()

    _run_steps(nsteps, step)
    got = data.arrays.to_numpy()
    plan.close()
    return got


def test_captured_steps_match_the_oracle(oracle):
    """Three steps of caar_launch + DSS with rotating time levels, captured in one graph (ne=4), then one step on every
    element at ne=41."""
    for ne, nsteps, tol in STEP_CASES:
        g, arrs, Dvv, sc, rsph, want = _step_case(oracle, ne, nsteps)
        got = _cxx_steps(g, arrs, Dvv, sc, rsph, nsteps)
        for n in cases.OUTPUT_NAMES:
            assert cases.scaled_err(got[n], want[n]) <= tol, (ne, n, cases.scaled_err(got[n], want[n]))


def test_captured_steps_in_fortran_order_match_the_oracle_and_the_cxx_layout(oracle):
    """What a Fortran host loops over: caar_launch_f90 + the Fortran-order DSS (plan layout "f90", rspheremp(np,np,ne)) with
    rotating time levels — three steps captured in one graph at ne=4 and one step on every element at ne=41, against the
    oracle's trajectory with the tolerances above and, every array, bit for bit against the C++-layout sequence of the same
    steps (each half is bit-identical across the layouts, so the sequence must be)."""
    for ne, nsteps, tol in STEP_CASES:
        g, arrs, Dvv, sc, rsph, want = _step_case(oracle, ne, nsteps)
        E = g.shape[0]
        f90 = fl.F90Arrays.from_numpy(fl.to_f90_numpy(arrs), 4, 72, E, device="cuda")
        scal = tsa.TestData.from_numpy({k: v[:1] for k, v in arrs.items()}, Dvv, sc, device="cuda")   # the scalars only
        scal.control.nete = E
        scal.dvv_device()
        r = torch.from_numpy(np.ascontiguousarray(rsph.transpose(0, 2, 1))).cuda()
        plan = tsa.DssPlan(g, 72, "f90")

        def step():
            fl.compute_and_apply_rhs(f90, scal)
            fl.dss(f90, plan, r, scal)
            scal.update_time_levels()

        _run_steps(nsteps, step)
        got = fl.from_f90_numpy(f90.to_numpy())
        plan.close()
        for n in cases.OUTPUT_NAMES:
            assert cases.scaled_err(got[n], want[n]) <= tol, (ne, n, cases.scaled_err(got[n], want[n]))
        cxx = _cxx_steps(g, arrs, Dvv, sc, rsph, nsteps)
        for n in tsa.ARRAY_NAMES:
            a, b = got[n].view(np.int64), cxx[n].view(np.int64)
            assert np.array_equal(a, b), (ne, n, int((a != b).sum()), np.argwhere(a != b)[:3].tolist())


def oracle_scalars():
    from oracle import pyoracle as po
    return po.default_scalars(72)


def test_speed_guard():
    """tools/dss_bench.py at ne=41 (face-major): the DSS within 1.5x the caar_launch time of the same process."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "dss_bench.py"), "--np", "4", "--nlev", "72", "--ne",
                        "41", "--calls", "10", "--rounds", "3"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["ms_dss"] <= 1.5 * res["ms_caar"], res
