"""Contact against a shell known only by its nodes and normals, and the
closest approach between groups of points — an ENGINE EXTENSION, opt-in.

The reference stubs GenericPeriphery (periphery.cpp:264-335: check_collision
returns false, fiber_interaction zeros), so on a surface-of-revolution shell
such as the oocyte nothing keeps the fibers inside. Everything here rests on
one primitive, backend.nearest(r_src, r_trg, src_group=None, trg_group=None)
-> (d2, index): for every target the nearest eligible source (HipBackend: the
Nearest pair kernel; any object with that method on numpy arrays serves).

Normals are the shell's stored ones and point INWARD (into the fluid the
fibers live in), as in every shell geometry this engine reads.

Accuracy. The gap is the distance to the tangent plane at the nearest node,
not to the surface. On a sphere of radius R a point at radius r whose nearest
node lies at angle theta_k has gap = R - r cos(theta_k) exactly: never below
the true R - r, by at most r (1 - cos(theta_k)). So the force is never larger
than the analytic one, and the collision test can miss a point that lies
outside by less than that excess; `threshold` is chosen with the node spacing
in mind ("Nearest source and generic-periphery contact")."""

import numpy as np


def _points(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1, 3))


def shell_gap(points, nodes, normals, backend):
    """(gap, k): k the nearest shell node of every point (n, 3) and
    gap = (p - x_k) . n_k, the signed distance to the tangent plane there,
    positive inside. k is -1 and gap +inf for a point without a nearest node
    (an empty shell, a NaN coordinate)."""
    points, nodes, normals = _points(points), _points(nodes), _points(normals)
    _, k = backend.nearest(nodes, points)
    k = np.asarray(k, dtype=np.int64)
    found = k >= 0
    gap = np.full(len(points), np.inf)
    kf = k[found]
    gap[found] = np.einsum("ij,ij->i", points[found] - nodes[kf], normals[kf])
    return gap, k


def generic_periphery_force(points, nodes, normals, f_0, l_0, backend):
    """(n, 3) steric force of the shell on the points:
    f = f_0 exp(-gap / l_0) n_k where gap > 0, zero elsewhere — the
    reference's sphere law (periphery.cpp:140-162: a collided node gets no
    force) for a surface known by its nodes. On a radial line through a node
    of a spherical shell it equals FiberFD.periphery_repulsion(kind="sphere")."""
    normals = _points(normals)
    gap, k = shell_gap(points, nodes, normals, backend)
    inside = (gap > 0) & (k >= 0)
    f = np.zeros((len(gap), 3))
    f[inside] = (f_0 * np.exp(-gap[inside] / l_0))[:, None] * normals[k[inside]]
    return f


def generic_points_collide(points, nodes, normals, threshold, backend):
    """any(gap <= threshold): the inequality of fiber_fd.points_collide for a
    sphere (r >= R - threshold), on the tangent-plane gap."""
    gap, _ = shell_gap(points, nodes, normals, backend)
    return bool(np.any(gap <= threshold))


def min_group_gap(points, group, backend):
    """(d_min, i, j): the closest pair of points (n, 3) that lie in different
    groups (integer ids (n,)), i < j, from one grouped nearest launch with the
    points as targets and sources. (inf, -1, -1) when no two points are in
    different groups."""
    points = _points(points)
    group = np.ascontiguousarray(np.asarray(group).reshape(-1)).astype(np.int64, copy=False)
    if len(group) != len(points):
        raise ValueError(f"group: {len(group)} ids for {len(points)} points")
    d2, idx = backend.nearest(points, points, group, group)
    d2, idx = np.asarray(d2), np.asarray(idx)
    if not len(d2) or not np.any(idx >= 0):
        return np.inf, -1, -1
    # the first minimum; its partner has the same d2, so this is the lower one
    # of a closest pair unless an equal pair comes earlier
    t = int(np.argmin(d2))
    s = int(idx[t])
    return float(np.sqrt(d2[t])), min(t, s), max(t, s)
