"""Seeded inputs of the fv_diag checks (tests/parity_diag.py): columns whose surface pressure runs from about 670 to 1055 hPa over
a model top at 3 hPa, so that the standard levels of the reference lie above the first layer mean (1, 2 hPa), inside the column, and
below the last layer mean (the high ground)."""
from __future__ import annotations

import numpy as np

import parity_phys as H
import ref_fv_diag as R
from gfdl_atmos_cubed_sphere_amd.layout import Bounds

PTOP = 300.0       # Pa
PLEVS = np.array(R.LEVS, dtype=np.float64) * 100.0      # Pa


def checksum(st):
    return H.checksum(st, with_shape=True)      # this package's goldens were recorded with the shapes hashed as well


def columns(nx, ny, km, seed):
    """-> (bd, state): pt (A x km, the halo holds other values), vort (CC x km), peln (nx, km+1, ny)"""
    rng = np.random.default_rng(seed)
    bd = Bounds(1, nx, 1, ny)
    i = np.arange(nx)[:, None] / max(nx - 1, 1)
    j = np.arange(ny)[None, :] / max(ny - 1, 1)
    zs = 3300.0 * np.clip(1.6 * i * (0.4 + 0.6 * j) - 0.15, 0.0, 1.0) + 40.0 * rng.uniform(0, 1, (nx, ny))
    ps = 103500.0 * np.exp(-zs / 7800.0) * (1.0 + 0.02 * rng.uniform(-1, 1, (nx, ny)))
    s = (np.arange(km + 1) / km) ** 1.7      # 0 at the top, 1 at the ground
    pe = np.zeros((nx, km + 1, ny), order="F")
    for k in range(km + 1):
        pe[:, k, :] = PTOP + s[k] * (ps - PTOP)
    pm = 0.5 * (pe[:, 1:, :] + pe[:, :-1, :]).transpose(0, 2, 1)      # (nx, ny, km)
    T = np.maximum(205.0, 290.0 * (pm / ps[:, :, None]) ** 0.19) + 2.0 * rng.uniform(-1, 1, (nx, ny, km))
    st = {"peln": np.asfortranarray(np.log(pe))}
    st["pt"] = np.asfortranarray(rng.uniform(150.0, 350.0, bd.shape("A", km)))
    bd.view(st["pt"], "A", 1, nx, 1, ny)[...] = T
    st["vort"] = np.asfortranarray(1.0e-4 * rng.uniform(-1, 1, (nx, ny, km)))
    return bd, st
