"""The conditioning of the inputs of tests/test_caar_truth_gpu.py and tests/test_f90_truth_gpu.py (no GPU): for every flavour and shape it runs, the C oracle
(fp64, bit-identical to the reference C++) is within 1e-13 of the 80-bit truth (oracle/np_oracle.py in numpy.longdouble) in
every slab of every output, 10x below that file's criterion (a).  A condition on the inputs, not a measurement of the
kernels: a family whose reference error were close to 1e-12 could not tell a wrong kernel from a right one."""
import numpy as np
import pytest

import cases
from oracle import np_oracle as npo

BOUND = 1e-13


def _worst_reference_error(oracle, np_, nlev, flavour, **kw):
    arrs, Dvv, sc = cases.truth_case(np_, nlev, flavour, **kw)
    ref = cases.copy_arrays(arrs)
    oracle.compute_and_apply_rhs(ref, Dvv, sc)
    truth = npo.compute_and_apply_rhs(arrs, Dvv, sc, dtype=np.longdouble)
    errs = cases.slab_errors(ref, truth, sc)
    return max(errs.items(), key=lambda kv: kv[1].max())


SHAPES = list(cases.TRUTH_DEFAULT_SHAPES) + [(4, nlev) for nlev in cases.TRUTH_NP4_NLEV]


@pytest.mark.parametrize("flavour", cases.TRUTH_SEEDED_FLAVOURS, ids=cases.truth_flavour_name)
@pytest.mark.parametrize("np_,nlev", SHAPES)
def test_reference_error_of_the_truth_inputs_is_small(oracle, np_, nlev, flavour):
    name, e = _worst_reference_error(oracle, np_, nlev, flavour)
    assert e.max() <= BOUND, (name, int(np.argmax(e)), float(e.max()))


@pytest.mark.parametrize("np_,nlev,ne,nets,nete", cases.TRUTH_F90_WIDE)
def test_reference_error_of_the_wide_truth_inputs_is_small(oracle, np_, nlev, ne, nets, nete):
    name, e = _worst_reference_error(oracle, np_, nlev, cases.TRUTH_WIDE_FLAVOUR, ne=ne, nets=nets, nete=nete)
    assert e.max() <= BOUND, (name, int(np.argmax(e)), float(e.max()))


def test_stratified_family_is_stratified():
    """What the family promises: dp3d thin at the top and thick at the bottom, decimal scales of v, vn0, omega_p."""
    a = cases.stratified_arrays(4, 72, 3, seed=5)
    h = cases.hashed_arrays(4, 72, 3, seed=5)
    prof = np.geomspace(2.0, 2000.0, 72) / 1000.0
    assert np.array_equal(a["elem_state_dp3d"], h["elem_state_dp3d"] * prof[None, None, :, None, None])
    assert a["elem_state_dp3d"][:, :, 0].max() < 3.01 and a["elem_state_dp3d"][:, :, -1].min() > 999.0
    for n, axes in (("elem_state_v", 3), ("elem_derived_vn0", 2), ("elem_derived_omega_p", 2)):
        k = np.round(np.log10(np.abs(a[n] / h[n]).reshape(a[n].shape[:axes] + (-1,))[..., 0]))
        scale = (10.0 ** k).reshape(k.shape + (1,) * (a[n].ndim - axes))
        assert np.array_equal(a[n], h[n] * scale), n                      # one decimal scale per slab
        assert set(k.astype(int).ravel()) == {-3, -2, -1, 0, 1}, n
    for n in a:
        if n not in ("elem_state_dp3d", "elem_state_v", "elem_derived_vn0", "elem_derived_omega_p"):
            assert np.array_equal(a[n], h[n]), n
