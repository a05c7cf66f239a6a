"""compute_and_apply_rhs, every kernel family, against an 80-bit truth, slab by slab.

tests/test_parity_gpu.py holds most kernels to 1e-12 of the fp64 C oracle, about 1000x looser than their rounding error, and
measures the exact result only for the fixture cases, field by field.  Here every kernel that caar_supported accepts runs on
inputs whose reference error is known (tests/cases.py TRUTH_*, pinned on the CPU by tests/test_caar_truth.py): the hashed
family, the stratified one (thin top levels, decimal scales of the winds per level), each also with rrearth = 1e-2.

Truth: oracle/np_oracle.py in numpy.longdouble.  A slab is one element at one level of one output (per interface for
eta_dot_dpdn); its error is max|x - truth| / max|truth| over that slab alone.  For every output array:
  (a) every HIP slab error <= 1e-12;
  (b) the worst HIP slab error <= max(4 x the worst slab error of the C oracle, 1e-15) (RATIO and floor of
      tests/test_operators_at_scale_gpu.py);
  (c) where the oracle is exact for the whole output (eta_dot_dpdn when rsplit == 1), HIP is exact too.
Nothing outside np1, the derived accumulators and [nets, nete) may change, bit for bit.

Families: every variant of NP=4 NLEV 72 / 128 and NP=8 NLEV 72 with rsplit 1 and 0 (bit for bit against variant 0 where
DESIGN.md section 4 says they round alike); the run-time-level-count kernel at 22 level counts over every launch_np4_dyn
branch; the default kernels over 1 100 elements; the extra build (libcaar_hip_extra.so) in a child pytest, and its
specialised kernels bit for bit against the run-time kernel of the default library.
Each case prints "TRUTH <family> <case>: hip .. ref .. ratio .." (worst slab of any output) and the largest ratio of one output.

What it sees that test_parity_gpu.py does not (in-bounds mutations, each scaling one intermediate by 1 + 2^-42): the parked
1/p of the run-time kernel only (test_any_level_count_…, test_other_level_counts_…, test_eulerian_vertical_coordinate_…,
test_aliased_time_levels_…, test_element_counts_… pass; 12 cases here fail), the NP=4 Eulerian half_rdp
(test_eulerian_vertical_coordinate_…, test_any_level_count_… pass; 63 fail) and the NP=8 one (every NP=8 test of
test_parity_gpu.py passes; 3 fail).
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import pytest  # noqa: E402

import cases  # noqa: E402
from oracle import np_oracle as npo  # noqa: E402
from oracle import pyoracle as po  # noqa: E402

pytestmark = pytest.mark.gpu

RTOL = 1e-12   # criterion (a)
RATIO = 4.0    # criterion (b)
FLOOR = 1e-15
EXTRA = os.path.join(ROOT, "tinman_sandbox_amd", "csrc", "libcaar_hip_extra.so")
FLAVOURS = cases.TRUTH_FLAVOURS
FID = cases.truth_flavour_name


def lib():
    import tinman_sandbox_amd as tsa
    return tsa.library().lib


def extra_build():
    return lib().caar_num_variants(4, 80) > 1   # -DCAAR_EXTRA_NLEV=1 (caar_kernel_args.h)


def run_gpu(arrs, Dvv, sc):
    import torch
    import tinman_sandbox_amd as tsa
    data = tsa.TestData.from_numpy(arrs, Dvv, sc, device="cuda")
    tsa.compute_and_apply_rhs(data)
    torch.cuda.synchronize()
    return data.arrays.to_numpy()


def reference_and_truth(arrs, Dvv, sc):
    ref = cases.copy_arrays(arrs)
    po.Oracle().compute_and_apply_rhs(ref, Dvv, sc)        # bit-identical to the reference C++ (tests/test_oracle.py)
    truth = npo.compute_and_apply_rhs(arrs, Dvv, sc, dtype=np.longdouble)
    return cases.slab_errors(ref, truth, sc), truth


def check_truth(got, ref_err, truth, arrs, sc, family, tag):
    """Criteria (a)-(c) for every output and the bits outside the outputs; prints and returns the worst (hip, ref)."""
    hip_err = cases.slab_errors(got, truth, sc)
    worst_h, worst_r, top = 0.0, 0.0, (0.0, "")
    for n in cases.OUTPUT_NAMES:
        eh, er = float(hip_err[n].max()), float(ref_err[n].max())
        assert eh <= RTOL, (tag, n, "slab", int(np.argmax(hip_err[n])), eh)                       # (a)
        assert eh <= max(RATIO * er, FLOOR), (tag, n, "hip %.3e ref %.3e" % (eh, er))              # (b)
        if er == 0.0:
            assert eh == 0.0, (tag, n, "the oracle is exact here", eh)                            # (c)
        worst_h, worst_r = max(worst_h, eh), max(worst_r, er)
        if er > 0 and eh / er >= top[0]:
            top = (eh / er, n)
    check_untouched(got, arrs, sc, tag)
    print("TRUTH %s %s: hip %.3e ref %.3e ratio %.2f (largest ratio of one output %.2f, %s)"
          % (family, tag, worst_h, worst_r, worst_h / worst_r, top[0], top[1]))
    return worst_h, worst_r


def check_untouched(got, arrs, sc, tag):
    ne = arrs["elem_fcor"].shape[0]
    e0, e1 = sc["nets"], (ne if sc.get("nete") is None else sc["nete"])
    bits = lambda x: np.ascontiguousarray(x).view(np.int64)  # noqa: E731
    for n in po.ARRAY_NAMES:
        g, a = got[n], arrs[n]
        if n not in cases.OUTPUT_NAMES:
            assert np.array_equal(bits(g), bits(a)), (tag, n)
            continue
        assert np.array_equal(bits(g[:e0]), bits(a[:e0])) and np.array_equal(bits(g[e1:]), bits(a[e1:])), (tag, n, "range")
        if n.startswith("elem_state_"):
            for t in range(a.shape[1]):
                if t != sc["np1"]:
                    assert np.array_equal(bits(g[:, t]), bits(a[:, t])), (tag, n, "time level", t)


def dyn_branch(nlev, rsplit):
    """The launch_np4_dyn branch (csrc/caar_np4.hip) that serves this level count."""
    tiles = (nlev + 3) // 4
    for lim, tpw in ((8, 2), (12, 3), (16, 4), (20, 5)):
        if tiles <= lim:
            return "dyn 4w x %d" % tpw
    if tiles <= 32 and rsplit == 0:
        return "dyn eulerian 8w x 4"
    if tiles <= 24:
        return "dyn 4w x 6"
    return "dyn 4w x 8 parked" if tiles <= 32 else "dyn 8w x 8 parked"


def same_form(np_, info):
    """test_parity_gpu.py::test_every_tuning_variant_matches_oracle: which variants must give variant 0's bits."""
    return np_ == 4 or (("MFMA" in info or "mfma" in info) and "8 waves x 9" in info)


def every_variant_against_truth(np_, nlev, flavour, family):
    """Every variant of (np_, nlev) on one flavour against the truth; the same-form variants bit for bit against variant 0."""
    L = lib()
    arrs, Dvv, sc = cases.truth_case(np_, nlev, flavour)
    ref_err, truth = reference_and_truth(arrs, Dvv, sc)
    n = L.caar_num_variants(np_, nlev)
    first = None
    try:
        for v in range(n):
            assert L.caar_select_variant(np_, nlev, v) == 0
            info = L.caar_variant_info(np_, nlev, v).decode()
            got = run_gpu(arrs, Dvv, sc)
            check_truth(got, ref_err, truth, arrs, sc, family, "np%d_nlev%d_%s_v%d" % (np_, nlev, FID(flavour), v))
            if first is None:
                first = got
            elif same_form(np_, info):
                for nm in cases.OUTPUT_NAMES:
                    assert np.array_equal(got[nm].view(np.int64), first[nm].view(np.int64)), (np_, nlev, v, nm)
    finally:
        L.caar_select_variant(np_, nlev, 0)
    return n


# ------------------------------------------------------------------------------------------------ B.1 default kernels
@pytest.mark.parametrize("flavour", FLAVOURS, ids=FID)
@pytest.mark.parametrize("np_,nlev", cases.TRUTH_DEFAULT_SHAPES)
def test_every_variant_of_the_default_kernels_against_truth(np_, nlev, flavour):
    family = ("np%d %d variants" % (np_, nlev)) + (" eulerian" if flavour[1] == 0 else "")
    assert every_variant_against_truth(np_, nlev, flavour, family) >= 2


# ------------------------------------------------------------------------------------------------ B.2 run-time level count
@pytest.mark.parametrize("flavour", FLAVOURS, ids=FID)
@pytest.mark.parametrize("nlev", cases.TRUTH_NP4_NLEV)
def test_np4_level_counts_against_truth(nlev, flavour):
    """The run-time-level-count kernel in the default library (every launch_np4_dyn branch, partly empty last tiles, the
    Eulerian form up to 128 levels); with the extra build, its specialised kernels (every variant) and the Eulerian form
    beyond 128 levels."""
    import tinman_sandbox_amd as tsa
    L = lib()
    extra = extra_build()
    specialised = b"<0," not in L.caar_kernel_name(4, nlev)
    assert specialised == (extra and nlev in cases.TRUTH_SPECIALISED_NLEV), L.caar_kernel_name(4, nlev)
    if flavour[1] == 0 and nlev > 128 and not extra:
        arrs, Dvv, sc = cases.truth_case(4, nlev, flavour)
        # the Eulerian form beyond 128 levels spills registers and is not in the default build: refused, not faked
        with pytest.raises(tsa.caar.CaarError, match="no kernel compiled"):
            run_gpu(arrs, Dvv, sc)
        return
    family = ("extra nlev%d" % nlev) if specialised else (("extra " if extra else "") + dyn_branch(nlev, flavour[1]))
    every_variant_against_truth(4, nlev, flavour, family)


# ------------------------------------------------------------------------------------------------ B.3 over 1 000 elements
@pytest.mark.parametrize("np_,nlev,ne,nets,nete", cases.TRUTH_WIDE)
def test_default_kernels_over_a_thousand_elements_against_truth(np_, nlev, ne, nets, nete):
    """Slabs in every XCD chunk of the element grid; elements outside [nets, nete) unchanged bit for bit."""
    L = lib()
    assert L.caar_selected_variant(np_, nlev) == 0
    arrs, Dvv, sc = cases.truth_case(np_, nlev, cases.TRUTH_WIDE_FLAVOUR, ne=ne, nets=nets, nete=nete)
    ref_err, truth = reference_and_truth(arrs, Dvv, sc)
    got = run_gpu(arrs, Dvv, sc)
    check_truth(got, ref_err, truth, arrs, sc, "np%d %d wide" % (np_, nlev), "np%d_nlev%d_e%d" % (np_, nlev, ne))


# ------------------------------------------------------------------------------------------------ B.4 / C the extra build
def _child(args, timeout):
    env = dict(os.environ, CAAR_LIBRARY_PATH=EXTRA)
    r = subprocess.run([sys.executable] + args, capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    return r, (r.stdout + r.stderr)[-3000:]


def _need_extra():
    if not os.path.exists(EXTRA):
        pytest.skip("libcaar_hip_extra.so not built (python -m tinman_sandbox_amd.build)")
    if os.environ.get("CAAR_LIBRARY_PATH"):
        pytest.skip("already running against an explicitly chosen library")


def test_extra_library_against_truth():
    """test_np4_level_counts_against_truth once more with the extra build: every specialised level count with every variant,
    the Eulerian form at NLEV 129, 200, 256."""
    _need_extra()
    r, tail = _child(["-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-s", "-m", "gpu", "-k",
                      "test_np4_level_counts_against_truth", "-p", "no:cacheprovider"], 900)
    print("\n".join(line.lstrip(".") for line in r.stdout.splitlines() if "TRUTH" in line))
    assert r.returncode == 0, tail
    last = r.stdout.strip().splitlines()[-1]
    assert "%d passed" % (len(cases.TRUTH_NP4_NLEV) * len(FLAVOURS)) in last and "skipped" not in last, tail
    # every variant (two each) of every specialised level count on every flavour
    assert r.stdout.count("TRUTH extra nlev") >= 2 * len(cases.TRUTH_SPECIALISED_NLEV) * len(FLAVOURS), tail


def dump_outputs(outdir):
    """(child, extra build) every variant of every specialised level count on every flavour -> outdir/*.npz + index.json."""
    L = lib()
    index = {}
    try:
        for nlev in cases.TRUTH_SPECIALISED_NLEV:
            n = L.caar_num_variants(4, nlev)
            index[str(nlev)] = dict(variants=n, kernel=L.caar_kernel_name(4, nlev).decode())
            for v in range(n):
                assert L.caar_select_variant(4, nlev, v) == 0
                for i, flavour in enumerate(FLAVOURS):
                    arrs, Dvv, sc = cases.truth_case(4, nlev, flavour)
                    got = run_gpu(arrs, Dvv, sc)
                    np.savez(os.path.join(outdir, "nlev%d_v%d_f%d.npz" % (nlev, v, i)), **{k: got[k] for k in cases.OUTPUT_NAMES})
            L.caar_select_variant(4, nlev, 0)
    finally:
        with open(os.path.join(outdir, "index.json"), "w") as f:
            json.dump(index, f)


def test_runtime_kernel_is_bit_identical_to_the_specialised_kernels(tmp_path):
    """the NP=4 kernels round alike.  The default library runs NLEV 26, 30, 32, 60, 64, 80, 96 through
    the run-time-level-count kernel; the extra build has kernels of their own (two variants each).  Every output array of
    every flavour (rsplit 1 and 0, moist and dry, both families), compared by its int64 view."""
    _need_extra()
    r, tail = _child([os.path.abspath(__file__), "--dump", str(tmp_path)], 600)
    assert r.returncode == 0, tail
    with open(tmp_path / "index.json") as f:
        index = json.load(f)
    L = lib()
    compared, differ = 0, []
    for nlev in cases.TRUTH_SPECIALISED_NLEV:
        assert b"<0," in L.caar_kernel_name(4, nlev)
        info = index[str(nlev)]
        assert info["variants"] >= 2 and "<0," not in info["kernel"], (nlev, info)
        for i, flavour in enumerate(FLAVOURS):
            arrs, Dvv, sc = cases.truth_case(4, nlev, flavour)
            mine = run_gpu(arrs, Dvv, sc)
            for v in range(info["variants"]):
                with np.load(tmp_path / ("nlev%d_v%d_f%d.npz" % (nlev, v, i))) as z:
                    for n in cases.OUTPUT_NAMES:
                        a, b = z[n].view(np.int64), mine[n].view(np.int64)
                        if not np.array_equal(a, b):
                            lev = np.unique(np.argwhere(a != b)[:, 1 + n.startswith("elem_state_")])
                            differ.append((nlev, v, FID(flavour), n, int((a != b).sum()), int(np.abs(a - b).max()),
                                           lev[:8].tolist()))
                compared += 1
    for d in differ:
        print("DIFFER nlev %d variant %d %s %s: %d values, <= %d ulp, levels %s" % d)
    assert not differ, differ[:10]
    assert compared >= 2 * len(cases.TRUTH_SPECIALISED_NLEV) * len(FLAVOURS)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--dump":
        dump_outputs(sys.argv[2])
    else:
        sys.exit("usage: %s --dump OUTDIR" % sys.argv[0])
