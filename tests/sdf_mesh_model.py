"""The surface-nets rule of rm_sdf_mesh (include/rm_api.h) in numpy
float32: from a distance volume d[nz][ny][nx] and the grid's origin and step to
(pos, quads).  Every float operation is one IEEE single-precision operation in
the order the contract writes it; only active cells and emitting edges are
visited, so mostly empty grids stay fast.

    inside(d)      d < 0 (NaN, +0 and -0 are outside)
    coords         origin[a] + float32(idx) * step[a]
    mesh           pos [V][3] float32, quads [Q][4] uint32
    triangles      the RM_MESH_TRIANGLES split of quads
"""
import numpy as np

F32 = np.float32
# cell offsets (du, dv) of the four cells around an edge, and of an edge's start in its cell
RING = ((-1, -1), (0, -1), (0, 0), (-1, 0))
STARTS = ((0, 0), (1, 0), (0, 1), (1, 1))


def coords(origin, step, dims):
    with np.errstate(all="ignore"):
        return [F32(origin[a]) + np.arange(dims[a], dtype=F32) * F32(step[a]) for a in range(3)]


def _at(arr, idx):
    """arr[z][y][x] at idx = [x, y, z] index arrays."""
    return arr[idx[2], idx[1], idx[0]]


def mesh(d, origin, step):
    d = np.asarray(d, F32)
    nz, ny, nx = d.shape
    n = (nx, ny, nz)
    empty = np.zeros((0, 3), F32), np.zeros((0, 4), np.uint32)
    if min(n) < 2:
        return empty
    ax = coords(origin, step, n)
    inside = d < 0  # a NaN compares false
    cnt = np.zeros((nz - 1, ny - 1, nx - 1), np.int32)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                cnt += inside[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]
    active = (cnt > 0) & (cnt < 8)
    index = np.cumsum(active.reshape(-1)).reshape(active.shape) - 1  # cell order: x fastest, then y, then z
    cz, cy, cx = np.nonzero(active)  # in that order
    cell = [cx, cy, cz]
    nv = len(cx)
    # vertices: the mean of the crossings on the 12 edges, summed in edge order
    acc = np.zeros((nv, 3), F32)
    num = np.zeros(nv, np.int32)
    with np.errstate(all="ignore"):
        for a in range(3):
            u, v = (a + 1) % 3, (a + 2) % 3
            for du, dv in STARTS:
                A = [None] * 3
                A[a], A[u], A[v] = cell[a], cell[u] + du, cell[v] + dv
                B = list(A)
                B[a] = A[a] + 1
                dA, dB = _at(d, A), _at(d, B)
                cross = _at(inside, A) != _at(inside, B)
                t = dA / (dA - dB)
                cA, cB = ax[a][A[a]], ax[a][B[a]]
                p = [None] * 3
                p[a] = cA + t * (cB - cA)
                p[u], p[v] = ax[u][A[u]], ax[v][A[v]]
                for k in range(3):
                    acc[:, k] = np.where(cross, acc[:, k] + p[k], acc[:, k])
                num += cross
        pos = (acc / num.astype(F32)[:, None]).astype(F32)
    # quads: every interior sign-changing edge, in point order, then axis order
    keys, recs = [], []
    for a in range(3):
        u, v = (a + 1) % 3, (a + 2) % 3
        if n[u] < 3 or n[v] < 3:
            continue
        sl = [None] * 3  # indexed x, y, z
        sl[a], sl[u], sl[v] = slice(0, n[a] - 1), slice(1, n[u] - 1), slice(1, n[v] - 1)
        sb = list(sl)
        sb[a] = slice(1, n[a])
        iA, iB = inside[sl[2], sl[1], sl[0]], inside[sb[2], sb[1], sb[0]]
        ez, ey, ex = np.nonzero(iA != iB)
        if not len(ex):
            continue
        A = [ex, ey, ez]
        A[u], A[v] = A[u] + 1, A[v] + 1  # the slices start at 1 on u and v
        q = np.empty((len(ex), 4), np.int64)
        for c, (du, dv) in enumerate(RING):
            C_ = list(A)
            C_[u], C_[v] = A[u] + du, A[v] + dv
            q[:, c] = _at(index, C_)
            assert _at(active, C_).all()
        a_in = _at(inside, A)
        q = np.where(a_in[:, None], q, q[:, [0, 3, 2, 1]])
        keys.append(((A[2].astype(np.int64) * ny + A[1]) * nx + A[0]) * 3 + a)
        recs.append(q)
    if not keys:
        return pos, empty[1]
    keys, recs = np.concatenate(keys), np.concatenate(recs)
    return pos, recs[np.argsort(keys, kind="stable")].astype(np.uint32)


def triangles(quads):
    """[Q][6]: (q0, q1, q2), (q0, q2, q3) of every quad."""
    return np.ascontiguousarray(quads[:, [0, 1, 2, 0, 2, 3]])


def topology(pos, quads):
    """(closed, all_referenced, euler, signed_volume): every directed quad edge once with
    its reverse once; every vertex in a quad; V - E + Q; the divergence-theorem volume."""
    q = quads.astype(np.int64)
    a, b = q.reshape(-1), np.roll(q, -1, axis=1).reshape(-1)
    V = len(pos)
    directed = a * max(V, 1) + b
    uniq, counts = np.unique(directed, return_counts=True)
    rev = np.unique(b * max(V, 1) + a)
    closed = bool((counts == 1).all() and len(uniq) == len(rev) and (uniq == rev).all())
    referenced = len(np.unique(q)) == V
    edges = len(np.unique(np.minimum(a, b) * max(V, 1) + np.maximum(a, b)))
    P = pos.astype(np.float64)
    vol = 0.0
    for i, j, k in ((0, 1, 2), (0, 2, 3)):
        vol += np.einsum("ij,ij->i", P[q[:, i]], np.cross(P[q[:, j]], P[q[:, k]])).sum() / 6.0
    return closed, referenced, V - edges + len(q), vol
