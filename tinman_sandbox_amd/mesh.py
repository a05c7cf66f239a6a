"""Meshes for hosts that have no HOMME mesh (tests, tools, Python users): global GLL-point ids in the form the direct
stiffness summation takes (include/caar_dss.h, caar.DssPlan), gdof[ie][a][b] as int64, and the inverse mass matrix.

    gdof = cubed_sphere_gdof(ne, np_)           # 6*ne^2 elements, face-major
    gdof = periodic_plane_gdof(nx, ny, np_)     # nx*ny elements on a doubly periodic plane
    rspheremp = inverse_mass(gdof, spheremp)    # 1 / (sum of spheremp over the copies of each point)

Everything here is plain numpy on the host; the summation itself runs on the device."""
import numpy as np


def _lattice(n_i, n_j, np_):
    """Lattice coordinates (u, v) of GLL point (a, b) of element (i, j), element index i*n_j + j: arrays [ne][np][np]."""
    s = np_ - 1
    i = np.arange(n_i).reshape(n_i, 1, 1, 1)
    j = np.arange(n_j).reshape(1, n_j, 1, 1)
    a = np.arange(np_).reshape(1, 1, np_, 1)
    b = np.arange(np_).reshape(1, 1, 1, np_)
    u = np.broadcast_to(i * s + a, (n_i, n_j, np_, np_)).reshape(n_i * n_j, np_, np_)
    v = np.broadcast_to(j * s + b, (n_i, n_j, np_, np_)).reshape(n_i * n_j, np_, np_)
    return u, v


def cubed_sphere_gdof(ne, np_):
    """Global ids of the GLL points of an ne x ne cubed sphere: 6*ne^2 elements in face-major order (element
    f*ne^2 + i*ne + j is element (i, j) of face f; its point (a, b) sits at lattice point (i*(np-1)+a, j*(np-1)+b) of the
    face).  A point is identified by its integer lattice coordinates on the surface of the cube [0, N]^3, N = ne*(np-1),
    so points on cube edges and corners are shared between faces; the ids are those coordinates numbered densely in
    lattice order: 6*N^2 + 2 of them."""
    if ne < 1 or np_ < 2:
        raise ValueError("cubed_sphere_gdof needs ne >= 1 and np >= 2")
    N = ne * (np_ - 1)
    u, v = _lattice(ne, ne, np_)
    zero, full = np.zeros_like(u), np.full_like(u, N)
    faces = ((u, v, zero), (u, v, full), (u, zero, v), (u, full, v), (zero, u, v), (full, u, v))
    code = np.concatenate([(x * (N + 1) + y) * (N + 1) + z for x, y, z in faces]).astype(np.int64)
    _, ids = np.unique(code, return_inverse=True)
    return ids.reshape(6 * ne * ne, np_, np_).astype(np.int64)


def periodic_plane_gdof(nx, ny, np_):
    """Global ids of an nx x ny doubly periodic plane (element i*ny + j is element (i, j)): point (a, b) of element (i, j)
    is lattice point ((i*(np-1)+a) mod Nx, (j*(np-1)+b) mod Ny), Nx = nx*(np-1), Ny = ny*(np-1).  With nx or ny equal to 1
    an element meets itself: its two opposite edges are one edge."""
    if nx < 1 or ny < 1 or np_ < 2:
        raise ValueError("periodic_plane_gdof needs nx, ny >= 1 and np >= 2")
    Nx, Ny = nx * (np_ - 1), ny * (np_ - 1)
    u, v = _lattice(nx, ny, np_)
    return ((u % Nx) * Ny + (v % Ny)).astype(np.int64)


def _groups(gdof):
    """The points of gdof [ne][np][np] grouped by id, each group in the order of the summation contract (ie, a*np+b)
    ascending: (flat point indices sorted by (id, index), start of each group, group of every flat point)."""
    g = np.asarray(gdof, dtype=np.int64).reshape(-1)
    order = np.argsort(g, kind="stable")       # stable: equal ids keep ascending flat index = (ie, a*np+b)
    gs = g[order]
    first = np.ones(gs.size, dtype=bool)
    first[1:] = gs[1:] != gs[:-1]
    starts = np.flatnonzero(first)
    group_of = np.empty(g.size, dtype=np.int64)
    group_of[order] = np.cumsum(first) - 1
    return order, starts, group_of


def inverse_mass(gdof, spheremp):
    """rspheremp[ie][a][b] = 1 / S, S the sum of spheremp over the copies of the point, accumulated from the first sharer
    left to right in the order of the summation contract; equal across the copies of every point, so a DSS with it leaves
    continuous fields bitwise continuous.  gdof and spheremp [ne][np][np] (C++ index order)."""
    gdof = np.asarray(gdof, dtype=np.int64)
    w = np.asarray(spheremp, dtype=np.float64).reshape(-1)
    if w.size != gdof.size:
        raise ValueError("gdof and spheremp must have the same shape")
    order, starts, group_of = _groups(gdof)
    counts = np.diff(np.append(starts, order.size))
    S = w[order[starts]].copy()
    for j in range(1, int(counts.max()) if counts.size else 0):
        m = counts > j
        S[m] = S[m] + w[order[starts[m] + j]]
    return (1.0 / S)[group_of].reshape(gdof.shape)
