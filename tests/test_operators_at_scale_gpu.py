"""The stand-alone kernels at the shapes the benchmarks run them at, against an 80-bit (numpy.longdouble) truth.

tests/test_sphere_ops.py holds caar_sphere_operator_ex / caar_euler_step / caar_preq_* against the C oracle at shapes
where the launch logic has little to do (<= 11 levels, <= 7 elements).  This file runs the paths those shapes never
reach (csrc/caar_operators_ex.hip, caar_operators.hip, caar_membench.hip):
  * deep columns: at NP=4 a wave covers 4 levels per step and the 4 waves of a workgroup loop only past 16 levels:
    the prefetch of the next tile (load_in(st + nw)), the accumulators the *_update forms carry with it, the
    in-place read of laplace_tensor_replace one tile ahead of its write, the matrix-core lane mapping of the
    composites (mfma4_point / mfma4_level);
  * wide grids: more than 65536 elements, so the grid-stride element loop takes a second trip; the vertical
    integrals past their 65536 x 64 column cap;
  * every byte of the copy kernels behind bench.py's bandwidth ceiling (stream_copy_GBs).

Truth: oracle/np_oracle.py ops_apply / ops_euler_step in longdouble on the kernels' own fp64 inputs, with the stored
rmetdet multiplying as in the kernels, i.e. the exact operator to 64 mantissa bits.  Every (element, level) slab of
an input is scaled by its own 10**k, k in [-6, 6], so a read from the wrong slab or an error confined to a small
slab is an O(1) relative error of that slab.  Per operator and shape:
  (a) every slab: max|hip - truth| <= 1e-12 max|truth| over that slab alone;
  (b) the worst slab's relative error of HIP <= max(4 x that of a plain fp64 evaluation of the same statement,
      1e-15): the kernels round no worse than straightforward code does.  Measured on an MI355X: worst HIP slab error
      1.3e-15, ratio at most 1.6 for every operator and shape (DPP, matrix-core composites and the Euler step alike).
Guard bands: outputs are interior slices of sentinel-filled buffers whose guard slabs must come back bit for bit;
inputs must come back unchanged (but for the in-place operator).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import cases
from oracle import np_oracle as npo

pytestmark = pytest.mark.gpu

RRS = (0.37, 1.5e-7)  # of order one (every term matters) and the physical 1/rearth of tools/operator_bench.py
WIDE = 65536 + 517    # past the 65536-workgroup grid of the operators and the Euler step
SENTINEL = -1.2345678912345e300
RATIO = 4.0           # criterion (b)
LD = np.longdouble


def dvv(np_):
    return cases.dvv_for(np_, "double" if np_ == 4 else "gll")


@functools.lru_cache(maxsize=4)
def geometry(np_, ne, seed):
    """tests/test_sphere_ops.py::geometry's arrays and ranges, distinct per element (numpy's generator: fast enough
    for the wide grids)."""
    r = np.random.default_rng(seed)
    u = lambda shape, lo, hi: r.uniform(lo, hi, (ne, np_, np_) + shape)  # noqa: E731
    D = u((2, 2), -1.0, 1.0)
    D[..., 0, 0] += 2.0
    D[..., 1, 1] += 2.5
    g = {"D": D, "Dinv": np.linalg.inv(D), "metdet": u((), 0.5, 2.0), "spheremp": u((), 0.1, 1.0),
         "mp": u((), 0.05, 0.6)}
    g["rmetdet"] = 1.0 / g["metdet"]
    mi = u((2, 2), -0.4, 0.4)
    mi[..., 0, 0] += 1.5
    mi[..., 1, 1] += 1.2
    g["metinv"] = 0.5 * (mi + mi.swapaxes(-1, -2))
    tv = u((2, 2), -0.3, 0.3)
    tv[..., 0, 0] += 1.0
    tv[..., 1, 1] += 0.8
    g["tensorVisc"] = tv
    g["vec_sph2cart"] = u((3, 2), -1.0, 1.0)
    return {k: np.ascontiguousarray(v) for k, v in g.items()}


def slab_scaled(shape, seed, lo=-3.0, hi=5.0, slab_axes=2):
    """Uniform [lo, hi) field, each slab (the first `slab_axes` indices) scaled by its own 10**k, k in [-6, 6]."""
    r = np.random.default_rng(seed)
    k = r.integers(-6, 7, shape[:slab_axes]).astype(np.float64)
    return r.uniform(lo, hi, shape) * (10.0 ** k).reshape(shape[:slab_axes] + (1,) * (len(shape) - slab_axes))


def slab_err(got, truth, slab_axes=2):
    """Relative error per slab: max|got - truth| / max|truth| over each slab alone (longdouble)."""
    sh = truth.shape[:slab_axes] + (-1,)
    d = np.abs(np.asarray(got, dtype=LD) - truth).reshape(sh).max(axis=-1)
    s = np.abs(truth).reshape(sh).max(axis=-1)
    assert np.all(s > 0)
    return (d / s).astype(np.float64)


def check_errors(what, hip, fp64, truth, slab_axes=2):
    """Criteria (a) and (b); returns (worst HIP slab error, worst fp64 slab error) for the report."""
    eh, ef = slab_err(hip, truth, slab_axes), slab_err(fp64, truth, slab_axes)
    worst = np.unravel_index(np.argmax(eh), eh.shape)
    assert eh.max() <= 1e-12, (what, "slab", worst, float(eh.max()))
    assert eh.max() <= max(RATIO * ef.max(), 1e-15), (what, float(eh.max()), float(ef.max()))
    print("%s: hip %.3e fp64 %.3e ratio %.2f" % (what, eh.max(), ef.max(), eh.max() / ef.max()))
    return float(eh.max()), float(ef.max())


def guarded(torch, shape, fill=None):
    """A sentinel buffer with one guard slab before and after; returns (buffer, interior view)."""
    buf = torch.full((shape[0] + 2,) + tuple(shape[1:]), SENTINEL, dtype=torch.float64, device="cuda")
    if fill is not None:
        buf[1:-1].copy_(torch.from_numpy(fill))
    return buf, buf[1:-1]


def assert_guards(torch, buf, what):
    torch.cuda.synchronize()
    sent = torch.full(buf.shape[1:], SENTINEL, dtype=torch.float64, device="cuda").view(torch.int64)
    assert torch.equal(buf[0].view(torch.int64), sent), (what, "guard before")
    assert torch.equal(buf[-1].view(torch.int64), sent), (what, "guard after")


def bits_equal(torch, t, a):
    return torch.equal(t.view(torch.int64).cpu(), torch.from_numpy(np.ascontiguousarray(a)).view(torch.int64))


# ------------------------------------------------------------------------------------------------ sphere operators
def run_operator(name, np_, ne, nl, e0, rr, seed, alpha=1.0, beta=0.0, nu_ratio=1.0, geo_ne=None):
    """caar_sphere_operator_ex on elements e0 .. e0+ne-1 of a geo_ne-element geometry, output (and, in place, input)
    inside guard slabs; returns (hip, fp64, longdouble truth)."""
    import torch
    import tinman_sandbox_amd as tsa
    _, vin, vout = tsa.SPHERE_OPERATORS[name]
    g = geometry(np_, geo_ne or e0 + ne + 3, 1000 + np_)
    ge = {k: v[e0:e0 + ne] for k, v in g.items()}
    x = slab_scaled((ne, nl, np_, np_) + ((2,) if vin else ()), seed)
    oshape = (ne, nl, np_, np_) + ((2,) if vout else ())
    old = None
    if name in ("gradient_sphere_update", "divergence_sphere_update"):
        # the accumulated-into field at the scale of the operator's own output in that slab (~ rr max|x|), so that
        # neither term hides the other
        xs = np.abs(x).reshape(ne, nl, -1).max(-1).reshape((ne, nl) + (1,) * (len(oshape) - 2))
        old = np.random.default_rng(seed + 1).uniform(-1.0, 1.0, oshape) * xs * rr
    dev = {k: torch.from_numpy(v).cuda() for k, v in g.items() if k in npo.OPS[name][2]}
    d = torch.from_numpy(dvv(np_)).cuda()
    if name == "laplace_tensor_replace":
        fbuf, field = guarded(torch, x.shape, x)
        got = tsa.sphere_operator_ex(name, field, dev, d, rr, e0=e0)
        assert got.data_ptr() == field.data_ptr()
        obuf = fbuf
    else:
        field = torch.from_numpy(x).cuda()
        obuf, out = guarded(torch, oshape, old)
        got = tsa.sphere_operator_ex(name, field, dev, d, rr, out=out, alpha=alpha, beta=beta, nu_ratio=nu_ratio, e0=e0)
        assert got.data_ptr() == out.data_ptr()
        torch.cuda.synchronize()
        assert bits_equal(torch, field, x), (name, "input modified")
    assert_guards(torch, obuf, name)
    hip = got.cpu().numpy()
    kw = dict(old=old, alpha=alpha, beta=beta, nu_ratio=nu_ratio)
    fp64 = npo.ops_apply(name, x, dvv(np_), ge, rr, dtype=np.float64, **kw)
    truth = npo.ops_apply(name, x, dvv(np_), ge, rr, dtype=LD, **kw)
    return hip, fp64, truth


OPERATORS = ("gradient_sphere", "divergence_sphere", "vorticity_sphere", "divergence_sphere_wk", "laplace_simple",
             "laplace_tensor", "curl_sphere_wk_testcov", "grad_sphere_wk_testcov", "vlaplace_sphere_wk_contra",
             "vlaplace_sphere_wk_cartesian", "gradient_sphere_update", "divergence_sphere_update",
             "vlaplace_sphere_wk_cartesian_damped", "laplace_tensor_replace")
DEEP = [(4, n) for n in (17, 33, 70, 72, 73, 128)] + [(8, n) for n in (5, 72, 128)]
DIV_UPDATE_PAIRS = ((0.75, -1.5), (-0.6, 1.0))  # (alpha, beta); the second is the Euler step's form (-dt, 1)


@pytest.mark.parametrize("name", OPERATORS)
@pytest.mark.parametrize("np_,nlev", DEEP)
def test_operator_deep_columns(np_, nlev, name):
    """All 14 operators on 24 (NP=4) / 12 (NP=8) elements from e0 = 5 of a larger geometry, at level counts that make
    each NP=4 wave take several steps and leave the last tile partly filled; both rrearth values."""
    ne, e0 = (24, 5) if np_ == 4 else (12, 5)
    pairs = DIV_UPDATE_PAIRS if name == "divergence_sphere_update" else ((1.0, 0.0),)
    for i, rr in enumerate(RRS):
        for alpha, beta in pairs:
            hip, fp64, truth = run_operator(name, np_, ne, nlev, e0, rr, 100 * nlev + 10 * i + np_, alpha=alpha,
                                            beta=beta, nu_ratio=1.75)
            check_errors("%s np%d nlev%d rr%g a%g b%g" % (name, np_, nlev, rr, alpha, beta), hip, fp64, truth)


# one operator per code path of sphere_operator_ex_kernel at NP=4: DPP, DPP update, matrix-core scalar / vector, in place
WIDE_OPS = [("gradient_sphere", 3, RRS[1]), ("divergence_sphere_update", 3, RRS[0]), ("laplace_tensor", 3, RRS[1]),
            ("vlaplace_sphere_wk_cartesian_damped", 2, RRS[0]), ("laplace_tensor_replace", 2, RRS[1])]


@pytest.mark.parametrize("name,nlev,rr", WIDE_OPS)
def test_operator_wide_grid(name, nlev, rr):
    """65536 + 517 elements from e0 = 3: the grid-stride loop's second trip; every element checked."""
    hip, fp64, truth = run_operator(name, 4, WIDE, nlev, 3, rr, 7 + nlev, alpha=0.75, beta=-1.5)
    check_errors("%s np4 wide nlev%d" % (name, nlev), hip, fp64, truth)


@pytest.mark.parametrize("np_", (4, 8))
def test_sphere_operator_range_wide_grid(np_):
    """caar_sphere_operator_range (gradient / divergence / vorticity of the CAAR path's geometry) on 65536 + 517
    elements from e0 = 3, 2 levels."""
    import torch
    import tinman_sandbox_amd as tsa
    from tinman_sandbox_amd import caar as m
    L = tsa.library()
    ne, e0, nl, rr = WIDE, 3, 2, RRS[1]
    g = geometry(np_, ne + 5, 2000 + np_)
    ge = {k: v[e0:e0 + ne] for k, v in g.items()}
    dev = {k: torch.from_numpy(g[k]).cuda() for k in ("D", "Dinv", "metdet", "rmetdet")}
    ptrs = m._CaarArrays()
    for k, t in dev.items():
        setattr(ptrs, "elem_" + k, C.cast(C.c_void_p(t.data_ptr()), m._dp))
    dims = m._CaarDims(np_, nl, 1, 1, ne + 5)
    d = torch.from_numpy(dvv(np_)).cuda()
    for which, name in enumerate(("gradient_sphere", "divergence_sphere", "vorticity_sphere")):
        vin = which != 0
        x = slab_scaled((ne, nl, np_, np_) + ((2,) if vin else ()), 50 + which)
        field = torch.from_numpy(x).cuda()
        obuf, out = guarded(torch, (ne, nl, np_, np_) + (() if vin else (2,)))
        L.check(L.lib.caar_sphere_operator_range(C.byref(dims), C.byref(ptrs), C.c_void_p(d.data_ptr()), which, e0,
                                                 e0 + ne, nl, C.c_void_p(field.data_ptr()), C.c_void_p(out.data_ptr()),
                                                 rr, None), "caar_sphere_operator_range")
        assert_guards(torch, obuf, name)
        assert bits_equal(torch, field, x), (name, "input modified")
        hip = out.cpu().numpy()
        fp64 = npo.ops_apply(name, x, dvv(np_), ge, rr, dtype=np.float64)
        truth = npo.ops_apply(name, x, dvv(np_), ge, rr, dtype=LD)
        check_errors("range %s np%d wide" % (name, np_), hip, fp64, truth)


# ------------------------------------------------------------------------------------------------ the Euler step
def run_euler(np_, ne, nlev, e0, qsize_d, qsize, geo_ne, seed, rr=RRS[0], dt=0.6):
    import torch
    import tinman_sandbox_amd as tsa
    g = geometry(np_, geo_ne, 3000 + np_)
    vstar = slab_scaled((ne, nlev, np_, np_, 2), seed)
    # Qdp slabs: (element, tracer, time level, level), each scaled on its own
    r = np.random.default_rng(seed + 1)
    k = r.integers(-6, 7, (geo_ne, qsize_d, 2, nlev)).astype(np.float64)
    qdp = r.uniform(0.5, 2.0, (geo_ne, qsize_d, 2, nlev, np_, np_)) * (10.0 ** k)[..., None, None]
    dev = {k_: torch.from_numpy(g[k_]).cuda() for k_ in ("Dinv", "metdet", "rmetdet")}
    vs, qd = torch.from_numpy(vstar).cuda(), torch.from_numpy(qdp).cuda()
    d = torch.from_numpy(dvv(np_)).cuda()
    ge = {k_: g[k_][e0:e0 + ne] for k_ in ("Dinv", "metdet", "rmetdet")}
    for qn0 in (0, 1):
        obuf, out = guarded(torch, (ne, qsize, nlev, np_, np_))
        got = tsa.euler_step(vs, qd, dev, d, qsize, qn0, dt, rr, e0=e0, out=out)
        assert got.data_ptr() == out.data_ptr()
        what = "euler np%d nlev%d ne%d qsize %d/%d qn0 %d" % (np_, nlev, ne, qsize, qsize_d, qn0)
        assert_guards(torch, obuf, what)
        assert bits_equal(torch, vs, vstar) and bits_equal(torch, qd, qdp), (what, "input modified")
        hip = got.cpu().numpy()
        Dv = dvv(np_)
        q = qdp[e0:e0 + ne]
        fp64 = npo.ops_euler_step(vstar, q, qsize, qn0, dt, Dv, ge["Dinv"], ge["metdet"], rr, rmetdet=ge["rmetdet"])
        truth = npo.ops_euler_step(vstar.astype(LD), q.astype(LD), qsize, qn0, LD(dt), Dv.astype(LD),
                                   ge["Dinv"].astype(LD), ge["metdet"].astype(LD), LD(rr),
                                   rmetdet=ge["rmetdet"].astype(LD))
        # slabs of qtens: (element, tracer, level)
        check_errors(what, hip, fp64, truth, slab_axes=3)


@pytest.mark.parametrize("np_,nlev", [(4, 17), (4, 72), (4, 128), (8, 72)])
@pytest.mark.parametrize("qsize_d,qsize", [(4, 4), (4, 2)])
def test_euler_step_deep_columns(np_, nlev, qsize_d, qsize):
    run_euler(np_, 12, nlev, 4, qsize_d, qsize, 20, 40 + nlev + qsize)


def test_euler_step_wide_grid():
    run_euler(4, WIDE, 2, 3, 3, 2, WIDE + 5, 77, rr=RRS[1])


# ------------------------------------------------------------------------------------------------ vertical integrals
@pytest.mark.parametrize("np_,ne,nlev", [(4, 262144 + 37, 2), (8, 65536 + 37, 2), (4, 300, 128)])
def test_vertical_integrals_past_the_grid_cap(np_, ne, nlev):
    """caar_preq_hydrostatic / caar_preq_omega_ps cap their grid at 65536 x 64 columns: the first two shapes have more
    columns than that.  Bit-identical to np_oracle.preq_* (which tests/test_sphere_ops.py ties to the C oracle)."""
    import torch
    import tinman_sandbox_amd as tsa
    from tinman_sandbox_amd import caar as m
    r = np.random.default_rng(ne + nlev)
    sh = (ne, nlev, np_, np_)
    a = dict(phis=r.uniform(0, 3e4, (ne, np_, np_)), Tv=r.uniform(200, 310, sh),
             p=np.cumsum(r.uniform(500, 1500, sh), axis=1), dp=r.uniform(500, 1500, sh), vg=r.uniform(-50, 50, sh),
             dd=r.uniform(-5, 5, sh))
    t = {k: torch.from_numpy(v).cuda() for k, v in a.items()}
    L = tsa.library()
    dims = m._CaarDims(np_, nlev, 1, 1, ne)
    V = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    pbuf, phi = guarded(torch, sh)
    obuf, om = guarded(torch, sh)
    L.check(L.lib.caar_preq_hydrostatic(C.byref(dims), ne, V(t["phis"]), V(t["Tv"]), V(t["p"]), V(t["dp"]), 287.04,
                                        V(phi), None), "caar_preq_hydrostatic")
    L.check(L.lib.caar_preq_omega_ps(C.byref(dims), ne, V(t["p"]), V(t["vg"]), V(t["dd"]), V(om), None),
            "caar_preq_omega_ps")
    assert_guards(torch, pbuf, "preq_hydrostatic")
    assert_guards(torch, obuf, "preq_omega_ps")
    for k, v in a.items():
        assert bits_equal(torch, t[k], v), (k, "input modified")
    assert np.array_equal(phi.cpu().numpy(), npo.preq_hydrostatic(a["phis"], a["Tv"], a["p"], a["dp"], 287.04))
    assert np.array_equal(om.cpu().numpy(), npo.preq_omega_ps(a["p"], a["vg"], a["dd"]))


# ------------------------------------------------------------------------------------------------ the copy ceiling
GUARD = 8192  # doubles after n: more than the largest chunk (8 loads x 256 lanes x 2 doubles)
COPY_SIZES = (2, 510, 512) + tuple(c + d for c in (512, 1024, 2048, 4096) for d in (-2, 2)) + (
    2 * (3 * (1 << 18) + 37),  # 6 MiB plus an odd number (37) of 16-byte pairs
    (1 << 26) + 2 * 37,        # 64 Mi doubles: every resident workgroup walks several chunks, plus a tail
    1 << 27)                   # bench.py's size


@pytest.fixture(scope="module")
def copy_buffers():
    import torch
    nmax = max(COPY_SIZES) + 1
    src = torch.arange(nmax, dtype=torch.float64, device="cuda") * 0.5 + 0.25  # distinct, not ones
    dst = torch.empty(nmax + GUARD, dtype=torch.float64, device="cuda")
    yield src, dst
    del src, dst
    torch.cuda.empty_cache()


def _copy_case(torch, src, dst, n, call):
    dst[:n + GUARD].fill_(SENTINEL)
    rc = call(n)
    torch.cuda.synchronize()
    return rc, torch.equal(dst[:n].view(torch.int64), src[:n].view(torch.int64)), bool(
        (dst[n:n + GUARD].view(torch.int64) == torch.tensor(SENTINEL, dtype=torch.float64).view(torch.int64).item()).all())


def test_stream_copy_copies_every_element(copy_buffers):
    """caar_stream_copy at 8 and 16 bytes per lane: dst[:n] == src[:n] bit for bit, nothing written past n; the
    16-byte form falls back to 8-byte lanes on odd n."""
    import torch
    import tinman_sandbox_amd as tsa
    L = tsa.library()
    src, dst = copy_buffers
    sp, dp = C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr())
    for lane_bytes in (8, 16):
        for n in COPY_SIZES + (1, 511, 2 * (3 * (1 << 18) + 37) + 1):
            rc, same, guard = _copy_case(torch, src, dst, n, lambda n_: L.lib.caar_stream_copy(dp, sp, n_, lane_bytes, None))
            assert rc == 0 and same and guard, (lane_bytes, n, rc, same, guard)
    assert torch.equal(src, torch.arange(src.numel(), dtype=torch.float64, device="cuda") * 0.5 + 0.25)


@pytest.mark.parametrize("variant", range(16))
def test_stream_copy_tuned_copies_every_element(copy_buffers, variant):
    """Each caar_stream_copy_tuned variant (bench.py times them all and quotes the fastest as stream_copy_GBs): a variant
    that skipped work would look fastest.  dst[:n] == src[:n] bit for bit, nothing written past n; odd n refused with
    dst untouched."""
    import torch
    import tinman_sandbox_amd as tsa
    L = tsa.library()
    assert L.lib.caar_stream_copy_tuned_variants() == 16
    src, dst = copy_buffers
    sp, dp = C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr())
    call = lambda n_: L.lib.caar_stream_copy_tuned(dp, sp, n_, variant, None)  # noqa: E731
    for n in COPY_SIZES:
        rc, same, guard = _copy_case(torch, src, dst, n, call)
        assert rc == 0 and same and guard, (variant, n, rc, same, guard)
    for n in (1, 511, 4097):
        dst[:n + GUARD].fill_(SENTINEL)
        assert call(n) == -1, (variant, n)  # CAAR_EINVAL
        torch.cuda.synchronize()
        assert bool((dst[:n + GUARD] == SENTINEL).all()), (variant, n)
