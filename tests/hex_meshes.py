"""Hexahedral numberings shared by tests/test_gpu_hex.py and
tests/test_hex_plan_host.py."""
import numpy as np


def permute_local(e2n, rng, frac=0.5):
    """Re-orient a fraction of the elements (swap / reverse local axes): the
    mesh is the same, the xi0 chains break wherever orientations differ."""
    e2n = e2n.copy()
    for e in np.flatnonzero(rng.random(e2n.shape[0]) < frac):
        perm = rng.permutation(3)
        flips = rng.random(3) < 0.5
        # orientation-preserving only (a reflection would make detJ < 0)
        sign = np.linalg.det(np.eye(3)[perm]) * (-1) ** int(flips.sum())
        if sign < 0:
            flips[0] = not flips[0]
        t = np.transpose(e2n[e], perm)
        for ax in range(3):
            if flips[ax]:
                t = np.flip(t, axis=ax)
        e2n[e] = t
    return e2n
