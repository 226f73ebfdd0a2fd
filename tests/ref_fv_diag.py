"""Numpy restatement of interpolate_vertical, written from tools/fv_diagnostics.F90:4910-4948.

Vectorised over the columns, sequential in k, every expression in the reference's order (left to right, its parentheses), so the
result is that of the compiled Fortran bit for bit: no exp or log runs per column (log(plev) is taken once, :4922).  Arrays are on
the compute domain: a3 (nx, ny, km), peln (nx, km+1, ny).  The columns that took each branch are counted into `cnt`."""
from __future__ import annotations

import numpy as np

LEVS = (1, 2, 3, 5, 7, 10, 20, 30, 50, 70, 100, 150, 200, 250, 300, 350, 400, 450, 500, 550, 600, 650, 700, 750, 800, 850, 900, 925,
        950, 975, 1000)      # the reference's default levs, hPa (:361)


def _count(cnt, name, mask):
    if cnt is not None:
        cnt[name] = cnt.get(name, 0) + int(np.count_nonzero(mask))


def interpolate_vertical(km, plev, peln, a3, cnt=None):
    """-> a2 (nx, ny)"""
    nx, ny = a3.shape[:2]
    logp = np.log(plev)
    pm = np.zeros((nx, ny, km))
    for k in range(km):
        pm[:, :, k] = 0.5 * (peln[:, k, :] + peln[:, k + 1, :])
    a2 = np.zeros((nx, ny), order="F")
    top = logp <= pm[:, :, 0]
    bot = ~top & (logp >= pm[:, :, km - 1])
    a2[top] = a3[:, :, 0][top]
    a2[bot] = a3[:, :, km - 1][bot]
    found = top | bot
    for k in range(1, km):
        hit = ~found & (logp <= pm[:, :, k]) & (logp >= pm[:, :, k - 1])
        if hit.any():
            with np.errstate(all="ignore"):
                val = a3[:, :, k - 1] + (a3[:, :, k] - a3[:, :, k - 1]) * (logp - pm[:, :, k - 1]) / (pm[:, :, k] - pm[:, :, k - 1])
            a2[hit] = val[hit]
            found |= hit
    _count(cnt, "above_top", top)
    _count(cnt, "below_bottom", bot)
    _count(cnt, "interior", found & ~top & ~bot)
    assert found.all()
    return a2
