"""Seeded input cases shared by the fixture generator (tests/golden/make_golden.py)
and the parity tests.  Inputs are never stored: they are rebuilt here from
integer-hash pseudo-random numbers (splitmix64 on uint64: exactly reproducible on
every platform) or from the reference's closed-form initialiser; only the
reference's OUTPUTS live in tests/golden/*.npz.
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import pyoracle as po  # noqa: E402  (tests may use the oracle)

GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")
OUTPUT_NAMES = ("elem_state_dp3d", "elem_state_v", "elem_state_T",
                "elem_derived_eta_dot_dpdn", "elem_derived_omega_p",
                "elem_derived_phi", "elem_derived_vn0")


def splitmix64(idx, seed):
    """uint64 -> uint64, vectorised; pure integer arithmetic (wraps mod 2^64)."""
    with np.errstate(over="ignore"):
        z = idx.astype(np.uint64) + np.uint64(seed) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return z


def uniform(shape, seed, lo=0.0, hi=1.0):
    n = int(np.prod(shape))
    u = (splitmix64(np.arange(n, dtype=np.uint64), seed) >> np.uint64(11)).astype(np.float64) * (1.0 / (1 << 53))
    return (lo + (hi - lo) * u).reshape(shape)


def hashed_arrays(np_, nlev, ne, seed, qsize_d=1, timelevels=3):
    """Physically plausible pseudo-random element arrays with a FULL (non-diagonal)
    D/Dinv, non-zero eta_dot_dpdn and every time level / Qdp slot populated, so
    that index or component mix-ups cannot cancel (the closed-form initialiser has
    diagonal D and symmetric fields)."""
    sh = po.array_shapes(np_, nlev, qsize_d, timelevels, ne)
    a = {}
    s = seed * 100
    D = uniform(sh["elem_D"], s + 1, -1.0, 1.0)
    D[..., 0, 0] += 2.0
    D[..., 1, 1] += 2.5
    a["elem_D"] = D
    det = D[..., 0, 0] * D[..., 1, 1] - D[..., 0, 1] * D[..., 1, 0]
    Dinv = np.empty_like(D)
    Dinv[..., 0, 0] = D[..., 1, 1] / det
    Dinv[..., 0, 1] = -D[..., 0, 1] / det
    Dinv[..., 1, 0] = -D[..., 1, 0] / det
    Dinv[..., 1, 1] = D[..., 0, 0] / det
    a["elem_Dinv"] = Dinv
    a["elem_fcor"] = uniform(sh["elem_fcor"], s + 2, -1.5e-4, 1.5e-4)
    a["elem_spheremp"] = uniform(sh["elem_spheremp"], s + 3, 0.1, 1.0)
    a["elem_metdet"] = uniform(sh["elem_metdet"], s + 4, 0.5, 2.0)
    a["elem_rmetdet"] = 1.0 / a["elem_metdet"]
    a["elem_state_dp3d"] = uniform(sh["elem_state_dp3d"], s + 5, 500.0, 1500.0)
    a["elem_state_v"] = uniform(sh["elem_state_v"], s + 6, -40.0, 40.0)
    a["elem_state_T"] = uniform(sh["elem_state_T"], s + 7, 200.0, 310.0)
    a["elem_state_phis"] = uniform(sh["elem_state_phis"], s + 8, 0.0, 3.0e4)
    a["elem_state_Qdp"] = uniform(sh["elem_state_Qdp"], s + 9, 0.0, 20.0)
    a["elem_derived_eta_dot_dpdn"] = uniform(sh["elem_derived_eta_dot_dpdn"], s + 10, -1.0, 1.0)
    a["elem_derived_omega_p"] = uniform(sh["elem_derived_omega_p"], s + 11, -1e-3, 1e-3)
    a["elem_derived_phi"] = uniform(sh["elem_derived_phi"], s + 12, 0.0, 1e5)
    a["elem_derived_pecnd"] = uniform(sh["elem_derived_pecnd"], s + 13, -50.0, 50.0)
    a["elem_derived_vn0"] = uniform(sh["elem_derived_vn0"], s + 14, -1e4, 1e4)
    return {k: np.ascontiguousarray(v) for k, v in a.items()}


def decimal_scales(shape, seed, lo=-3, hi=1):
    """10**k with integer k in [lo, hi], one per entry of `shape`, from the splitmix hash (the same on every platform)."""
    n = int(np.prod(shape))
    k = (splitmix64(np.arange(n, dtype=np.uint64), seed) % np.uint64(hi - lo + 1)).astype(np.int64) + lo
    return (10.0 ** k.astype(np.float64)).reshape(shape)


def stratified_arrays(np_, nlev, ne, seed, qsize_d=1, timelevels=3):
    """hashed_arrays with slabs of very different sizes: dp3d times the per-level profile geomspace(2, 2000, nlev)/1000 (top
    levels ~1-3 Pa thick, bottom ones ~3000 Pa), v times 10**k per (element, time level, level) and vn0, omega_p times 10**k
    per (element, level), k in [-3, 1].  An error confined to a thin level or a weak wind is then large next to its own slab
    while it stays small next to the field's largest value."""
    a = hashed_arrays(np_, nlev, ne, seed, qsize_d, timelevels)
    s = seed * 100 + 50
    prof = np.geomspace(2.0, 2000.0, nlev) / 1000.0
    a["elem_state_dp3d"] = a["elem_state_dp3d"] * prof[None, None, :, None, None]
    a["elem_state_v"] = a["elem_state_v"] * decimal_scales((ne, timelevels, nlev), s + 1)[..., None, None, None]
    a["elem_derived_vn0"] = a["elem_derived_vn0"] * decimal_scales((ne, nlev), s + 2)[..., None, None, None]
    a["elem_derived_omega_p"] = a["elem_derived_omega_p"] * decimal_scales((ne, nlev), s + 3)[..., None, None]
    return {k: np.ascontiguousarray(v) for k, v in a.items()}


FAMILIES = {"hashed": hashed_arrays, "stratified": stratified_arrays}


def dvv_for(np_, kind="double"):
    O = po.Oracle()
    if np_ == 4 and kind == "double":
        return O.dvv_np4(False)
    if np_ == 4 and kind == "f32":
        return O.dvv_np4(True)
    return O.dvv_gll(np_)


# name -> dict(np, nlev, ne, init, dvv, overrides of default scalars)
CASES = {
    # the reference's own configuration (data_structures.cpp:117-163), double-literal Dvv
    "np4_nlev72_closed": dict(np=4, nlev=72, ne=3, init="closed", dvv="double", sc={}),
    # the Fortran driver's configuration: float32-rounded Dvv (main.F90:83-96)
    "np4_nlev72_closed_f32dvv": dict(np=4, nlev=72, ne=3, init="closed", dvv="f32", sc={}),
    # dry branch (P:128-139)
    "np4_nlev72_closed_dry": dict(np=4, nlev=72, ne=2, init="closed", dvv="double", sc=dict(qn0=-1)),
    # full metric tensors, permuted time levels, second Qdp slot, element sub-range,
    # non-unit dt2 / eta_ave_w
    "np4_nlev72_hashed": dict(np=4, nlev=72, ne=4, init="hashed", seed=1, dvv="double",
                              sc=dict(n0=2, np1=0, nm1=1, qn0=1, dt2=37.5, eta_ave_w=0.625,
                                      nets=1, nete=3)),
    # same with the horizontal-operator terms amplified (rrearth 1e-2 instead of 1.6e-7)
    # so that an error in any Dvv contraction is O(1) in the outputs
    "np4_nlev72_hashed_amplified": dict(np=4, nlev=72, ne=2, init="hashed", seed=2, dvv="double",
                                        sc=dict(n0=1, np1=2, nm1=0, qn0=0, dt2=0.01,
                                                eta_ave_w=0.5, rrearth=1e-2)),
    "np4_nlev128_closed": dict(np=4, nlev=128, ne=2, init="closed", dvv="double", sc={}),
    "np4_nlev128_hashed": dict(np=4, nlev=128, ne=2, init="hashed", seed=3, dvv="double",
                               sc=dict(n0=1, np1=2, nm1=0, qn0=1, dt2=12.0, eta_ave_w=0.75,
                                       rrearth=1e-3)),
    # NP=8: the reference has no derivative matrix for it; GLL matrix of this repo
    "np8_nlev72_closed": dict(np=8, nlev=72, ne=1, init="closed", dvv="gll", sc={}),
    "np8_nlev72_hashed": dict(np=8, nlev=72, ne=2, init="hashed", seed=4, dvv="gll",
                              sc=dict(n0=2, np1=1, nm1=0, qn0=0, dt2=5.0, eta_ave_w=0.25,
                                      rrearth=1e-3)),
}


def make_case(name):
    """-> (arrays dict, Dvv, scalars dict)"""
    c = CASES[name]
    if c["init"] == "closed":
        arrs = po.Oracle().init_arrays(c["np"], c["nlev"], 1, 3, c["ne"])
    else:
        arrs = hashed_arrays(c["np"], c["nlev"], c["ne"], c["seed"])
    sc = po.default_scalars(c["nlev"])
    sc.update(c["sc"])
    return arrs, dvv_for(c["np"], c["dvv"]), sc


def golden_path(name):
    return os.path.join(GOLDEN_DIR, name + ".npz")


def load_golden(name):
    with np.load(golden_path(name), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def copy_arrays(arrs):
    return {k: v.copy() for k, v in arrs.items()}


def rel_err(got, want):
    """max |got-want| / max(|want|, tiny), elementwise; 0 where both are 0."""
    d = np.abs(got - want)
    den = np.maximum(np.abs(want), np.finfo(np.float64).tiny)
    return float(np.max(np.where(d == 0, 0.0, d / den))) if d.size else 0.0


def scaled_err(got, want):
    """max |got-want| / max|want|: error relative to the field's magnitude (used for
    accumulated diagnostics whose individual entries can cancel to ~0)."""
    m = float(np.max(np.abs(want)))
    return float(np.max(np.abs(got - want))) / (m if m > 0 else 1.0)


# ---- the live-reference checks of tests/test_oracle.py.  Their inputs are built here, and reference_results() computes
#      what the reference returns for them through oracle/_ref (where it is built); tests/golden/make_golden.py --digests
#      records the digests of those results in REFERENCE_DIGESTS, so that the checks also run where oracle/_ref is not.
REFERENCE_DIGESTS = os.path.join(GOLDEN_DIR, "reference_digests.json")
OPERATOR_NPS = (4, 8)
ALIASED_LEVELS = ((0, 1, 0), (1, 1, 0), (0, 1, 1), (2, 2, 2))
INIT_SCALARS = ("n0", "np1", "nm1", "qn0", "dt2", "rrearth", "eta_ave_w", "Rwater_vapor", "Rgas", "kappa", "ps0")


def digest(a):
    """SHA-256 of an array's float64 values in C order, -0.0 read as 0.0: two arrays have the same digest exactly when
    np.array_equal holds for them (finite values)."""
    return hashlib.sha256((np.ascontiguousarray(a, dtype=np.float64) + 0.0).tobytes()).hexdigest()


def reference_digests():
    with open(REFERENCE_DIGESTS) as f:
        return json.load(f)


def operator_case(np_):
    """-> (arrays, Dvv, rrearth, [(element, scalar field, vector field), ...])"""
    arrs = hashed_arrays(np_, 72, 2, seed=11)
    fields = [(ie, uniform((np_, np_), 77 + ie, -3, 5), uniform((np_, np_, 2), 99 + ie, -3, 5)) for ie in range(2)]
    return arrs, dvv_for(np_, "double" if np_ == 4 else "gll"), 0.37, fields


def aliased_case(levels):
    """Coinciding time-level indices (n0, np1, nm1) = levels -> (arrays, Dvv, scalars)"""
    arrs = hashed_arrays(4, 72, 2, seed=140)
    sc = po.default_scalars(72)
    sc.update(n0=levels[0], np1=levels[1], nm1=levels[2], qn0=1, dt2=0.25, eta_ave_w=0.5)
    return arrs, dvv_for(4), sc


def aliased_key(levels):
    return "aliased_%d%d%d" % tuple(levels)


def reference_operators(R, np_):
    """gradient / divergence / vorticity of operator_case(np_) by the reference (R: po.Reference(np_, 72))"""
    arrs, Dvv, rr, fields = operator_case(np_)
    out = {}
    for ie, s, v in fields:
        k = "operators_np%d/%d/" % (np_, ie)
        out[k + "gradient"] = R.sphere_operator(0, s, arrs, ie, rr, Dvv)
        out[k + "divergence"] = R.sphere_operator(1, v, arrs, ie, rr, Dvv)
        out[k + "vorticity"] = R.sphere_operator(2, v, arrs, ie, rr, Dvv)
    return out


def reference_init(R, ne=5):
    """The reference's TestData::init_data for `ne` elements and its compute_norm of one field (R: po.Reference(4, 72))"""
    arrs, Dvv, sc = R.init_data(ne)
    out = {"init/" + n: arrs[n] for n in po.ARRAY_NAMES}
    out.update({"init/Dvv": Dvv, "init/hyai": sc["hyai"], "init/scalars": np.array([sc[k] for k in INIT_SCALARS], dtype=float),
                "init/norm": np.array([R.compute_norm(arrs["elem_state_v"][0, 1])])})
    return out


def reference_aliased(R, levels):
    """Every array after one reference call on aliased_case(levels) (R: po.Reference(4, 72))"""
    arrs, Dvv, sc = aliased_case(levels)
    b = copy_arrays(arrs)
    R.compute_and_apply_rhs(b, Dvv, sc)
    return {aliased_key(levels) + "/" + n: b[n] for n in po.ARRAY_NAMES}


# ---- compute_and_apply_rhs against an 80-bit truth, slab by slab (tests/test_caar_truth_gpu.py; the conditioning of these
#      inputs: tests/test_caar_truth.py).  A flavour: (input family, rsplit, qn0, amplified (rrearth 1e-2), (n0, np1, nm1),
#      element range (nets, nete) of a 3-element case).
TRUTH_FLAVOURS = (
    ("hashed", 1, 0, False, (2, 0, 1), (0, None)),
    ("stratified", 1, -1, True, (1, 2, 0), (0, None)),
    ("hashed", 0, -1, True, (0, 1, 2), (0, None)),
    ("stratified", 0, 1, False, (2, 1, 0), (1, 3)),
    ("stratified", 0, 0, True, (0, 1, 2), (0, None)),
)
TRUTH_DEFAULT_SHAPES = ((4, 72), (4, 128), (8, 72))      # every variant of the default kernels
TRUTH_ANY_NLEV = (2, 3, 5, 17, 26, 47, 50, 64, 65, 79, 85, 96, 97, 100, 127, 129, 200, 256)   # the run-time-level-count kernel
TRUTH_SPECIALISED_NLEV = (26, 30, 32, 60, 64, 80, 96)    # the extra build's own kernels
TRUTH_NP4_NLEV = tuple(sorted(set(TRUTH_ANY_NLEV + TRUTH_SPECIALISED_NLEV)))
TRUTH_NE = 3
# one case per default kernel over more than 1 000 elements: (np, nlev, ne, nets, nete)
TRUTH_WIDE = ((4, 72, 1100, 37, 1061), (4, 128, 1100, 37, 1061), (8, 72, 1100, 37, 1061))
TRUTH_WIDE_FLAVOUR = ("stratified", 1, 0, True, (2, 0, 1), None)
# the Fortran-order kernels (tests/test_f90_truth_gpu.py): caar_launch_f90 refuses rsplit == 0, so the two Lagrangian flavours
# above and two more: every kernel meets moist and dry, both Qdp slots, both families, four orders of the time levels, a range
# that starts and one that ends inside the array
TRUTH_F90_FLAVOURS = (
    TRUTH_FLAVOURS[0],
    TRUTH_FLAVOURS[1],
    ("stratified", 1, 1, False, (0, 1, 2), (1, 3)),
    ("hashed", 1, -1, True, (0, 2, 1), (0, 2)),
)
# ... and over more than 1 000 elements: the three specialised kernels and one run-time shape per PARK setting
TRUTH_F90_WIDE = TRUTH_WIDE + ((4, 50, 1100, 37, 1061), (4, 100, 1100, 37, 1061))
# the flavours with a seed of their own (truth_case), in the order that fixes it: appended to, never reordered
TRUTH_SEEDED_FLAVOURS = TRUTH_FLAVOURS + tuple(f for f in TRUTH_F90_FLAVOURS if f not in TRUTH_FLAVOURS)


def truth_case(np_, nlev, flavour, ne=TRUTH_NE, nets=None, nete=None):
    """-> (arrays, Dvv, scalars) of one flavour; the seed follows from (np, nlev, flavour)."""
    family, rsplit, qn0, amplified, (n0, np1, nm1), rng = flavour
    seed = 1000 + 10 * nlev + np_ + (3000 * (1 + TRUTH_SEEDED_FLAVOURS.index(flavour)) if flavour in TRUTH_SEEDED_FLAVOURS else 0)
    arrs = FAMILIES[family](np_, nlev, ne, seed)
    sc = po.default_scalars(nlev)
    sc.update(n0=n0, np1=np1, nm1=nm1, qn0=qn0, dt2=0.25, eta_ave_w=0.5, rsplit=rsplit,
              hybi=(np.arange(nlev + 1) / nlev) ** 2)
    if rng is not None:
        sc["nets"], sc["nete"] = rng
    if nets is not None:
        sc["nets"], sc["nete"] = nets, nete
    if amplified:
        sc["rrearth"] = 1e-2
    return arrs, dvv_for(np_), sc


def truth_flavour_name(flavour):
    family, rsplit, qn0, amplified, (n0, np1, nm1), rng = flavour
    return "%s_r%d_%s%s_%d%d%d%s" % (family, rsplit, "dry" if qn0 < 0 else "moist", "_amp" if amplified else "", n0, np1, nm1,
                                     "" if rng is None or rng == (0, None) else "_e%d-%d" % rng)


def output_slabs(name, x, sc):
    """Output `name` of a full array set as [slab][point]: one element at one level (interface for eta_dot_dpdn) of the
    state at np1 or of a derived array, over the elements [nets, nete)."""
    if name.startswith("elem_state_"):
        x = x[:, sc["np1"]]
    x = x[sc["nets"]:(x.shape[0] if sc.get("nete") is None else sc["nete"])]
    return x.reshape(x.shape[0] * x.shape[1], -1)


def slab_errors(got, truth, sc):
    """name -> the relative error of every slab, max|got - truth| / max|truth| over that slab alone (in longdouble), for
    each output; inf where a slab whose truth is all zero is not zero."""
    out = {}
    for n in OUTPUT_NAMES:
        t = output_slabs(n, truth[n], sc)
        d = np.abs(np.asarray(output_slabs(n, got[n], sc), dtype=np.longdouble) - t).max(axis=1)
        s = np.abs(t).max(axis=1)
        e = np.where(d == 0, 0.0, np.where(s > 0, d / np.where(s > 0, s, 1), np.inf))
        out[n] = e.astype(np.float64)
    return out


def reference_results():
    """Everything the live-reference checks compare with, computed by oracle/_ref."""
    out = {}
    for np_ in OPERATOR_NPS:
        out.update(reference_operators(po.Reference(np_, 72), np_))
    R = po.Reference(4, 72)
    out.update(reference_init(R))
    for levels in ALIASED_LEVELS:
        out.update(reference_aliased(R, levels))
    return out
