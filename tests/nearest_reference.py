"""numpy brute force of the nearest-source search (skelly_nearest_*), and a
stand-in backend that serves skellysim_amd.contact from it off the GPU.

d2 = dx*dx + dy*dy + dz*dz per pair, chunked over targets; np.argmin returns
the first minimum, which is the library's tie rule (lowest source index). A
source in the target's group, or with a NaN coordinate, is not eligible; a
target without an eligible source (or with a NaN coordinate) gets +inf / -1."""

import numpy as np

CHUNK = 512  # targets a block of the (targets x sources) distance matrix


def nearest(r_src, r_trg, src_group=None, trg_group=None):
    """(d2 float64 (n_trg,), index int64 (n_trg,))."""
    src = np.asarray(r_src, float).reshape(-1, 3)
    trg = np.asarray(r_trg, float).reshape(-1, 3)
    assert (src_group is None) == (trg_group is None)
    d2 = np.full(len(trg), np.inf)
    index = np.full(len(trg), -1, dtype=np.int64)
    if not len(src):
        return d2, index
    for a in range(0, len(trg), CHUNK):
        t = trg[a:a + CHUNK]
        m = 0.0
        for c in range(3):  # dx*dx + dy*dy + dz*dz, in this order
            d = t[:, c, None] - src[None, :, c]
            m = m + d * d
        m[np.isnan(m)] = np.inf  # a NaN compare is false: never better
        if src_group is not None:
            own = np.asarray(trg_group)[a:a + CHUNK, None] == np.asarray(src_group)[None, :]
            m[own] = np.inf
        k = np.argmin(m, axis=1)
        best = m[np.arange(len(t)), k]
        found = np.isfinite(best)
        d2[a:a + CHUNK] = np.where(found, best, np.inf)
        index[a:a + CHUNK] = np.where(found, k, -1)
    return d2, index


def distances(r_src, r_trg):
    """The full (n_trg, n_src) matrix of d2, for the tie checks of small cases."""
    d = np.asarray(r_trg, float)[:, None, :] - np.asarray(r_src, float)[None, :, :]
    return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]


class NumpyNearestBackend:
    """A host backend for contact.py and SystemFD's contact methods: numpy
    arrays in and out, no device."""

    def __init__(self):
        self.calls = 0

    def nearest(self, r_src, r_trg, src_group=None, trg_group=None):
        self.calls += 1
        return nearest(r_src, r_trg, src_group, trg_group)
