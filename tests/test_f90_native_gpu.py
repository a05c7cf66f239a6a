"""compute_and_apply_rhs directly on Fortran-ordered device arrays (include/caar_f90.h: caar_launch_f90,
caar_launch_steps_f90; csrc/caar_f90.hip).

The Fortran-order kernels run the same element bodies as the C++-layout ones with only the addresses changed, so they are
held to BIT identity with caar_launch on the same values (every array, untouched time levels and read-only inputs
included), and through that and directly to the reference's own outputs."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import cases
from oracle import pyoracle as po

import tinman_sandbox_amd as tsa
from tinman_sandbox_amd import f90_layout as fl

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_cpp(arrs, Dvv, sc):
    data = tsa.TestData.from_numpy(arrs, Dvv, sc, device="cuda")
    tsa.compute_and_apply_rhs(data)
    torch.cuda.synchronize()
    return data.arrays.to_numpy()


def run_f90(arrs, Dvv, sc, nsteps=None, rotate=True):
    """The same call on the arrays in Fortran order (converted on the host by the pinned axis map); results back in the
    C++ layout."""
    ne, tl, nlev, np_, _ = arrs["elem_state_dp3d"].shape
    qd = arrs["elem_state_Qdp"].shape[1]
    f90 = fl.F90Arrays.from_numpy(fl.to_f90_numpy(arrs), np_, nlev, ne, qd, tl, device="cuda")
    scal = tsa.TestData.from_numpy({k: v[:1] for k, v in arrs.items()}, Dvv, sc, device="cuda")  # scalars only
    scal.control.nete = ne if sc.get("nete") is None else sc["nete"]
    if nsteps is None:
        fl.compute_and_apply_rhs(f90, scal)
    else:
        fl.compute_and_apply_rhs_steps(f90, scal, nsteps, rotate)
    torch.cuda.synchronize()
    return fl.from_f90_numpy(f90.to_numpy())


def assert_bit_identical(got, want, tag):
    for n in tsa.ARRAY_NAMES:
        assert got[n].shape == want[n].shape, (tag, n)
        assert np.array_equal(got[n], want[n]), (tag, n, float(np.max(np.abs(got[n] - want[n]))))


# (tag, np, nlev, ne, qsize_d, timelevels, scalar overrides)
BIT_CASES = [
    ("np4_nlev72_moist", 4, 72, 5, 1, 3, dict(n0=2, np1=0, nm1=1, qn0=1, dt2=37.5, eta_ave_w=0.625)),
    ("np4_nlev72_dry", 4, 72, 3, 1, 3, dict(n0=1, np1=2, nm1=0, qn0=-1, dt2=5.0, eta_ave_w=0.5)),
    ("np4_nlev128", 4, 128, 3, 1, 3, dict(n0=1, np1=2, nm1=0, qn0=1, dt2=12.0, eta_ave_w=0.75, rrearth=1e-3)),
    ("np4_nlev27_runtime", 4, 27, 4, 1, 3, dict(n0=0, np1=1, nm1=2, qn0=0, dt2=3.0, eta_ave_w=0.5)),
    ("np4_nlev200_runtime", 4, 200, 3, 1, 3, dict(n0=2, np1=1, nm1=0, qn0=1, dt2=2.0, eta_ave_w=0.25)),
    ("np8_nlev72", 8, 72, 3, 1, 3, dict(n0=2, np1=1, nm1=0, qn0=0, dt2=5.0, eta_ave_w=0.25, rrearth=1e-3)),
    ("np8_nlev72_dry", 8, 72, 2, 1, 3, dict(n0=0, np1=1, nm1=2, qn0=-1, dt2=1.0, eta_ave_w=1.0)),
    ("np4_nlev72_middle_range", 4, 72, 7, 1, 3, dict(n0=1, np1=0, nm1=2, qn0=0, dt2=2.5, nets=2, nete=5)),
    ("np4_nlev72_qsize2_qn0_1", 4, 72, 3, 2, 3, dict(n0=0, np1=1, nm1=2, qn0=1, dt2=4.0, eta_ave_w=0.75)),
    ("np8_nlev72_qsize2_qn0_1", 8, 72, 2, 2, 3, dict(n0=0, np1=1, nm1=2, qn0=1, dt2=4.0, eta_ave_w=0.75)),
    ("np4_nlev72_timelevels4", 4, 72, 3, 1, 4, dict(n0=3, np1=1, nm1=0, qn0=1, dt2=1.5)),
]


@pytest.mark.parametrize("tag,np_,nlev,ne,qd,tl,over", BIT_CASES, ids=[c[0] for c in BIT_CASES])
def test_fortran_order_is_bit_identical_to_cpp_layout(tag, np_, nlev, ne, qd, tl, over):
    arrs = cases.hashed_arrays(np_, nlev, ne, seed=300 + len(tag), qsize_d=qd, timelevels=tl)
    Dvv = cases.dvv_for(np_)
    sc = po.default_scalars(nlev)
    sc.update(over)
    want = run_cpp(arrs, Dvv, sc)
    got = run_f90(arrs, Dvv, sc)
    assert_bit_identical(got, want, tag)
    # the call did something, and nothing outside [nets, nete) changed
    nets, nete = sc.get("nets", 0), sc.get("nete") or ne
    assert not np.array_equal(got["elem_state_T"][nets:nete, sc["np1"]], arrs["elem_state_T"][nets:nete, sc["np1"]])
    for n in tsa.ARRAY_NAMES:
        assert np.array_equal(got[n][:nets], arrs[n][:nets]) and np.array_equal(got[n][nete:], arrs[n][nete:]), (tag, n)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_fortran_order_matches_goldens(name):
    """The nine golden cases in Fortran order: every case's C++ golden, and where the fixture holds what the reference
    FORTRAN routine wrote (f90_* keys), that too — all seven mutated arrays to <= 1e-12 of the field's magnitude."""
    arrs, Dvv, sc = cases.make_case(name)
    gold = cases.load_golden(name)

    def check(got, want, sc, what):
        for n in cases.OUTPUT_NAMES:
            g = got[n][:, sc["np1"]] if n.startswith("elem_state_") else got[n]
            w = want[n] if want[n].shape == g.shape else want[n][:, sc["np1"]]
            assert cases.scaled_err(g, w) <= 1e-12, (name, what, n, cases.scaled_err(g, w))

    check(run_f90(arrs, Dvv, sc), {n: gold[n] for n in cases.OUTPUT_NAMES}, sc, "C++ golden")
    if "f90_elem_state_T" in gold:
        sc2 = dict(sc, nets=0, nete=None)  # the Fortran fixture covers every element
        check(run_f90(arrs, Dvv, sc2), {n: gold["f90_" + n] for n in cases.OUTPUT_NAMES}, sc2, "reference Fortran")


@pytest.mark.parametrize("np_,nlev", [(4, 72), (4, 128), (8, 72)])
def test_steps_match_single_calls_and_the_cpp_step_loop(np_, nlev):
    """caar_launch_steps_f90 (5 calls, with and without the time-level rotation) is bit-identical to five caar_launch_f90
    calls and to caar_launch_steps on the C++ layout (the fused step-loop kernel where one exists)."""
    arrs = cases.hashed_arrays(np_, nlev, 3, seed=77, qsize_d=1)
    Dvv = cases.dvv_for(np_)
    sc = po.default_scalars(nlev)
    sc.update(n0=0, np1=1, nm1=2, qn0=0, dt2=1.0e-3, eta_ave_w=0.5)
    for rotate in (False, True):
        steps = run_f90(arrs, Dvv, sc, nsteps=5, rotate=rotate)
        # five single calls, rotating the indices as update_time_levels does
        f90 = fl.F90Arrays.from_numpy(fl.to_f90_numpy(arrs), np_, nlev, 3, device="cuda")
        scal = tsa.TestData.from_numpy(arrs, Dvv, sc, device="cuda")
        for _ in range(5):
            fl.compute_and_apply_rhs(f90, scal)
            if rotate:
                scal.update_time_levels()
        torch.cuda.synchronize()
        single = fl.from_f90_numpy(f90.to_numpy())
        assert_bit_identical(steps, single, "steps vs singles, rotate=%d" % rotate)
        data = tsa.TestData.from_numpy(arrs, Dvv, sc, device="cuda")
        tsa.compute_and_apply_rhs_steps(data, 5, rotate)
        torch.cuda.synchronize()
        assert_bit_identical(steps, data.arrays.to_numpy(), "f90 steps vs caar_launch_steps, rotate=%d" % rotate)


def test_fortran_order_beyond_4gib_offsets(oracle):
    """100 000 NP=4 NLEV=72 elements held in Fortran order only (18.6 GB): single arrays exceed 4 GiB, so the Fortran-order
    addressing must be 64-bit too.  Elements on both sides of the 4 GiB mark of v and the last one are checked against the
    oracle run on copies of exactly those elements' inputs."""
    E, nlev = 100000, 72
    init = tsa.ElementArrays(4, nlev, E, device="cuda").init_data()
    f90 = fl.F90Arrays.allocate(4, nlev, E)
    fl.egress(init, f90, all_arrays=True)   # the reference's closed-form state, in Fortran order
    torch.cuda.synchronize()
    del init
    torch.cuda.empty_cache()
    per_elem_v = f90.t["elem_state_v"][0].numel() * 8
    mark = (1 << 32) // per_elem_v
    assert mark + 1 < E
    picks = [0, mark - 1, mark, mark + 1, E // 2, E - 1]
    sub = fl.from_f90_numpy({n: f90.t[n][picks].cpu().numpy().copy() for n in tsa.ARRAY_NAMES})
    scal = tsa.TestData().init_data(1, 4, nlev, device="cuda")
    scal.control.nete = E
    scal.control.qn0, scal.control.dt2 = 0, 0.5
    fl.compute_and_apply_rhs(f90, scal)
    torch.cuda.synchronize()
    sc = po.default_scalars(nlev)
    sc.update(qn0=0, dt2=0.5)
    oracle.compute_and_apply_rhs(sub, scal.deriv.Dvv, sc)
    got = fl.from_f90_numpy({n: f90.t[n][picks].cpu().numpy() for n in tsa.ARRAY_NAMES})
    for n in tsa.caar.MUTATED:
        assert cases.scaled_err(got[n], sub[n]) <= 1e-12, n
    assert bool(torch.isfinite(f90.t["elem_state_T"][:, 1]).all())
    del f90
    torch.cuda.empty_cache()


def _bench(np_, nlev, elems):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "f90_native_bench.py"), "--np", str(np_), "--nlev",
                        str(nlev), "--elems", str(elems)], capture_output=True, text=True, timeout=420)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("nlev,elems", [(72, 10000), (128, 12500)])
def test_fortran_order_runs_at_the_cpp_layout_rate(nlev, elems):
    """tools/f90_native_bench.py in a fresh process: (b) caar_launch_f90 on Fortran-ordered arrays within 10 % of (a)
    caar_launch on C++-layout arrays (a floor against gross regressions; the target is 5 %), and
    (c) the conversion route (layout_from_f90 + caar_launch + layout_to_f90) at least 2.5 times slower than (b)."""
    out = _bench(4, nlev, elems)
    assert out["b_over_a"] <= 1.10, out
    assert out["c_over_b"] >= 2.5, out


def test_resident_fortran_program_prints_the_reference_norms():
    """host/fortran/caar_f90_resident.F90: allocates with caar_arrays_alloc, copies the reference driver's state up once in
    Fortran order, calls caar_launch_f90 and prints the norms the reference's own Fortran executable prints
    (tests/golden/fortran_orig_stdout.txt), plus a `ms per call` line."""
    from tinman_sandbox_amd import build
    exe = build.build_fortran_resident()
    if exe is None:
        pytest.skip("flang not available")
    out = subprocess.run([exe, "3"], check=True, capture_output=True, text=True, timeout=300).stdout
    got = [float(x) for x in re.findall(r"\|\|(?:v|T|dp)\|\|_2\s*=\s*([-+0-9.eE]+)", out)]
    txt = open(os.path.join(cases.GOLDEN_DIR, "fortran_orig_stdout.txt")).read().split()
    want = [float(txt[i + 2]) for i, w in enumerate(txt) if w.startswith("||")]
    assert len(got) == 6 and len(want) == 6, out
    assert np.allclose(got[:3], want[:3], rtol=1e-15, atol=0)
    assert np.allclose(got[3:], want[3:], rtol=1e-13, atol=0)
    assert re.search(r"ms per call\s*=?\s*[0-9.]+", out), out
