"""numpy reference of exposure gain compensation (include/mcs.h "Exposure"): the overlap
statistics of a plan, the gain solve, and the quantised gain on source bytes.

The statistics are built from tests/lens_ref.py: a camera slot's position per mosaic pixel
(chain_positions / cyl_positions, lenses included), its coverage (distances >= 0) and its
replicate-border sample (sample_replicate, the blend's I_s), taken at the points (gx << k, gy << k)
of the 2^k grid.  Everything is integer, so the library must match exactly.
"""
import numpy as np

import lens_ref


def grid(a, k):
    """The 2^k grid points of a per-pixel array: (gx << k, gy << k)."""
    return a[::1 << k, ::1 << k]


def overlap_stats(pos, slot_cams, captures, k, n_cams):
    """(N, S) of per-slot positions `pos` (lens_ref.*_positions), slot cameras `slot_cams` and
    `captures` = [[frame of camera 0, 1, ...], ...]: N (n, n) and S (F, n, n), int64."""
    sizes = {}
    for c, im in enumerate(captures[0]):
        im = np.asarray(im)
        sizes[c] = (im.shape[1], im.shape[0])
    dist = lens_ref.distances(pos, slot_cams, sizes)
    live = [s for s, cam in enumerate(slot_cams) if cam is not None and cam < n_cams and
            sizes[cam][0] > 0]
    cover = {s: grid(dist[s], k) >= 0 for s in live}
    gpos = {s: (grid(pos[s][0], k), grid(pos[s][1], k)) for s in live}
    N = np.zeros((n_cams, n_cams), np.int64)
    S = np.zeros((len(captures), n_cams, n_cams), np.int64)
    for s in live:
        for t in live:
            N[slot_cams[s], slot_cams[t]] = int((cover[s] & cover[t]).sum())
    for f, frames in enumerate(captures):
        for s in live:
            i = slot_cams[s]
            lum = lens_ref.sample_replicate(frames[i], *gpos[s]).astype(np.int64).sum(axis=-1)
            for t in live:
                S[f, i, slot_cams[t]] = int(lum[cover[s] & cover[t]].sum())
    return N, S


def chain_stats(flat, captures, k, interp=lens_ref.INTER_LINEAR, lenses=None):
    """Statistics of a chain plan (flat = Plan.describe())."""
    pos, slot_cams, _ = lens_ref.chain_positions(flat, interp, lenses)
    n = len(flat["cam_w"])
    # (a slot's camera is covered only inside its own frame; slot 0 is camera 0)
    return overlap_stats(pos, slot_cams, captures, k, n)


def cyl_stats(rig, geom, captures, k, interp=lens_ref.INTER_LINEAR, lenses=None):
    pos, slot_cams = lens_ref.cyl_positions(rig, geom["out_w"], geom["out_h"], geom["f_cyl"],
                                            geom["u0"], geom["v0"], interp, lenses)
    return overlap_stats(pos, slot_cams, captures, k, len(rig))


def means(N, S, channels):
    N = np.asarray(N, np.float64)
    with np.errstate(all="ignore"):
        return np.where(N > 0, np.asarray(S, np.float64) / (channels * np.where(N > 0, N, 1)), 0.0)


def solve(N, S, channels, alpha=0.01, beta=100.0):
    """Brown & Lowe's gains as OpenCV's GainCompensator builds the system; cameras with
    N[i, i] == 0 are left out and get gain 1."""
    N = np.asarray(N, np.int64)
    n = N.shape[0]
    act = [i for i in range(n) if N[i, i] > 0]
    g = np.ones(n)
    if not act:
        return g
    I = means(N, S, channels)
    A = np.zeros((len(act), len(act)))
    b = np.zeros(len(act))
    for a, i in enumerate(act):
        for c, j in enumerate(act):
            nij = float(N[i, j])
            b[a] += beta * nij
            A[a, a] += beta * nij
            if j == i:
                continue
            A[a, a] += 2 * alpha * I[i, j] ** 2 * nij
            A[a, c] -= 2 * alpha * I[i, j] * I[j, i] * nij
    g[act] = np.linalg.solve(A, b)
    return g


def mismatch(N, S, channels, g):
    """sum N_ij (g_i I_ij - g_j I_ji)^2: the data term the gains reduce."""
    I = means(N, S, channels)
    g = np.asarray(g, np.float64)
    d = g[:, None] * I - g[None, :] * I.T
    return float((np.asarray(N, np.float64) * d * d).sum())


def quantise(g):
    """q = clamp(round-half-even(256 g), 1, 65535)."""
    return int(min(max(np.rint(256.0 * float(g)), 1.0), 65535.0))


def apply_q(img, q):
    """p' = min(255, (p q + 128) >> 8) on every byte."""
    p = np.asarray(img, np.uint8).astype(np.int64)
    return np.minimum(255, (p * int(q) + 128) >> 8).astype(np.uint8)


def apply_gain(img, g):
    return apply_q(img, quantise(g))
