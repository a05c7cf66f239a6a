"""numpy restatement of the direct stiffness summation (include/caar_dss.h), the definition the kernels are tested against.

For each global id, its sharers are ordered by (ie, a*np+b) ascending; S = ((x0 + x1) + x2) + ... from the first sharer;
every copy receives rspheremp[ie][a][b] * S.  Arrays in logical (C++) index order: gdof, rspheremp [ne][np][np], fields
[ne][nlev][np][np]."""
import numpy as np

STATE = ("elem_state_T", "elem_state_v", "elem_state_dp3d")


def groups(gdof):
    """(order, starts, counts, group_of): flat point indices ie*np*np + a*np + b sorted by (id, index); the first position
    and the size of each id's run in `order`; the group of every flat point."""
    g = np.asarray(gdof, dtype=np.int64).reshape(-1)
    order = np.lexsort((np.arange(g.size), g))
    gs = g[order]
    first = np.ones(g.size, dtype=bool)
    first[1:] = gs[1:] != gs[:-1]
    starts = np.flatnonzero(first)
    counts = np.diff(np.append(starts, g.size))
    group_of = np.empty(g.size, dtype=np.int64)
    group_of[order] = np.cumsum(first) - 1
    return order, starts, counts, group_of


def sum_copies(P, gdof):
    """P [ne*np*np][...]: per id, the left-to-right sum over its sharers, [n_ids][...]."""
    order, starts, counts, _ = groups(gdof)
    S = P[order[starts]].copy()
    for j in range(1, int(counts.max())):
        m = counts > j
        S[m] = S[m] + P[order[starts[m] + j]]
    return S


def dss_field(X, gdof, rsph):
    """One field [ne][nlev][np][np] -> its DSS (a new array)."""
    ne, nlev, np_, _ = X.shape
    P = np.ascontiguousarray(X.transpose(0, 2, 3, 1)).reshape(ne * np_ * np_, nlev)
    _, _, _, group_of = groups(gdof)
    S = sum_copies(P, gdof)
    out = np.asarray(rsph, dtype=np.float64).reshape(-1, 1) * S[group_of]
    return np.ascontiguousarray(out.reshape(ne, np_, np_, nlev).transpose(0, 3, 1, 2))


def dss_state(arrs, gdof, rsph, tl):
    """C++-layout state arrays (elem_state_T / dp3d [ne][TL][nlev][np][np], elem_state_v [...][2]) -> copies with time
    level tl replaced by its DSS."""
    out = {n: arrs[n].copy() for n in STATE}
    out["elem_state_T"][:, tl] = dss_field(arrs["elem_state_T"][:, tl], gdof, rsph)
    out["elem_state_dp3d"][:, tl] = dss_field(arrs["elem_state_dp3d"][:, tl], gdof, rsph)
    for c in (0, 1):
        out["elem_state_v"][:, tl, ..., c] = dss_field(arrs["elem_state_v"][:, tl, ..., c], gdof, rsph)
    return out


def sharer_counts(gdof):
    """Number of sharers of every point, [ne][np][np]."""
    _, _, counts, group_of = groups(gdof)
    return counts[group_of].reshape(np.shape(gdof))


def info(gdof):
    """What caar_dss_plan_info reports for a plan over `gdof`: distinct ids, ids with more than one sharer, open points
    (ends of an element-boundary segment — two neighbouring points of one element edge, as an unordered pair of ids —
    that only one element has), the largest sharer count."""
    g = np.asarray(gdof, dtype=np.int64)
    _, _, counts, _ = groups(g)
    np_ = g.shape[1]
    t = np.arange(np_ - 1)
    ends = [(g[:, 0, t], g[:, 0, t + 1]), (g[:, -1, t], g[:, -1, t + 1]), (g[:, t, 0], g[:, t + 1, 0]),
            (g[:, t, -1], g[:, t + 1, -1])]
    x = np.concatenate([e[0].reshape(-1) for e in ends])
    y = np.concatenate([e[1].reshape(-1) for e in ends])
    seg = np.stack([np.minimum(x, y), np.maximum(x, y)], axis=1)
    uniq, cnt = np.unique(seg, axis=0, return_counts=True)
    open_ids = np.unique(uniq[cnt == 1].reshape(-1))
    return {"unique_points": int(counts.size), "shared_points": int(np.sum(counts > 1)), "open_points": int(open_ids.size),
            "max_sharers": int(counts.max()) if counts.size else 0}


def scaled_random(shape, rng, per_level_axes):
    """Uniform(-1, 1) values times 10^k, k in [-3, 3] drawn separately for every index of the axes `per_level_axes`
    (e.g. element and level), so that a wrong sharer or row shows in the sum."""
    x = rng.uniform(-1.0, 1.0, size=shape)
    kshape = [shape[i] if i in per_level_axes else 1 for i in range(len(shape))]
    return x * 10.0 ** rng.integers(-3, 4, size=kshape)


def random_state(np_, nlev, ne, timelevels, seed):
    """C++-layout T, v, dp3d with a separate decimal scale per element, time level and level."""
    rng = np.random.default_rng(seed)
    return {"elem_state_T": scaled_random((ne, timelevels, nlev, np_, np_), rng, (0, 1, 2)),
            "elem_state_v": scaled_random((ne, timelevels, nlev, np_, np_, 2), rng, (0, 1, 2)),
            "elem_state_dp3d": scaled_random((ne, timelevels, nlev, np_, np_), rng, (0, 1, 2))}
