"""numpy restatement of Held_Suarez_Tend and age_of_air (driver/solo/hswf.F90:41-207, :209-245), written from the Fortran: the same
operations in the same order, level by level from the bottom up over whole (i, j) planes, and a count of every branch.
tests/test_held_suarez_hostemu.py holds it to the outputs of the reference's compiled Fortran (tests/golden/held_suarez_*.npz): u_dt,
v_dt bit for bit (no transcendental stands between their inputs and them: peln is an input), t_dt at the measured bound (numpy's log
and exp are not the compiled reference's).  The library tests use it at the shapes the goldens do not have.  The latitude table is
formed with the host's libm (math.sin, math.cos, math.pow), as the library forms it."""
from __future__ import annotations

import math

import numpy as np

COUNTS = ("meso", "strat", "tropo", "friction", "no_friction", "teq_t0", "teq_free")
T0, H0, SIGB, AKAP = 200.0, 7.0, 0.7, 2.0 / 7.0
RAKAP = 1.0 / AKAP
TY, TZ, P0, SDAY = 60.0, 10.0, 100000.0, 24.0 * 3600.0


def scalars(pdt, radius, rd_zur, pi):
    """hswf.F90:101-133 in its order"""
    s = dict(pdt=pdt, rdt=1.0 / pdt)
    rad_ratio = radius / 6371.0e3
    kf_day = SDAY * rad_ratio
    s["rkv"] = pdt / kf_day
    s["rka"] = pdt / (40.0 * kf_day)
    s["rks"] = pdt / (4.0 * kf_day)
    s["t_ms"] = 10.0 * rad_ratio
    t_st = 40.0 * rad_ratio
    s["tau"] = (t_st - s["t_ms"]) / math.log(100.0)
    s["rms"] = pdt / (s["t_ms"] * SDAY)
    s["rmr"] = 1.0 / (1.0 + s["rms"])
    s["rsgb"] = 1.0 / (1.0 - SIGB)
    s["ap0k"] = 1.0 / math.pow(P0, AKAP)
    s["algpk"] = math.log(s["ap0k"])
    s["rd_zur_rad"] = rd_zur * pi / 180.0
    return s


def lat_table(lat):
    """the five planes fv3_grid_upload_lat forms, each in the reference's expression (:152, :180-184)"""
    ap0k = 1.0 / math.pow(P0, AKAP)
    f = lambda fn: np.vectorize(fn, otypes=[np.float64])(lat)      # noqa: E731
    return dict(lat=np.asarray(lat, dtype=np.float64), cos=f(math.cos), tey=f(lambda a: TY * math.sin(a) * math.sin(a)),
                tez=f(lambda a: TZ * (ap0k / AKAP) * math.cos(a) * math.cos(a)), cos4=f(lambda a: math.pow(math.cos(a), 4.0)))


def held_suarez_tend(bd, km, pr, o, teq_out=None):
    """in place on o["t_dt"], o["u_dt"], o["v_dt"] (compute domain).  pr: pdt, strat, zurita, rd_zur, radius, pi.  -> counts.
    teq_out (nx, ny, km): receives teq"""
    s = scalars(pr["pdt"], pr["radius"], pr["rd_zur"], pr["pi"])
    tab = lat_table(o["lat"])
    r = (bd.is_, bd.ie, bd.js, bd.je)
    A = lambda a: bd.view(a, "A", *r)      # noqa: E731
    delp, pt, ua, va, u_dt, v_dt = (A(o[n]) for n in ("delp", "pt", "ua", "va", "u_dt", "v_dt"))
    t_dt, pkz, peln = o["t_dt"], o["pkz"], o["peln"]
    pes = o["pe"][1:-1, km, 1:-1]
    cnt = {n: 0 for n in COUNTS}
    nx, ny = pes.shape
    pl1, teq1 = np.zeros((nx, ny)), np.zeros((nx, ny))
    tey_z = None
    if pr["zurita"]:
        tmp = tab["lat"] / s["rd_zur_rad"]
        tey_z = 1.0 - 0.19 * (1.0 - np.exp(-(tmp * tmp)))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for k in range(km - 1, -1, -1):
            pl = delp[:, :, k] / (peln[:, k + 1, :] - peln[:, k, :])
            p, td = pt[:, :, k], t_dt[:, :, k]
            meso = (pl <= 1.0e2) if pr["strat"] else np.zeros((nx, ny), dtype=bool)
            strat = ((pl > 1.0e2) & (pl <= 100.0e2)) if pr["strat"] else np.zeros((nx, ny), dtype=bool)
            tropo = ~(meso | strat)
            dz = H0 * np.log(pl1 / pl)
            # mesosphere (:149-154)
            teq_m = teq1 + (-(2.25 * tab["cos"]) * dz)
            new_m = td + ((p + s["rms"] * teq_m) * s["rmr"] - p) * s["rdt"]
            # stratosphere (:156-165)
            relx = s["t_ms"] + s["tau"] * np.log(0.01 * pl)
            relx = s["pdt"] / (relx * SDAY)
            teq_s = teq1 + 2.25 * tab["cos"] * dz
            new_s = td + relx * (teq_s - p) / (1.0 + relx) * s["rdt"]
            # troposphere (:167-186)
            sigl = pl / pes
            if pr["zurita"]:
                tmp = np.exp(AKAP * np.log(sigl))
                tez = 0.1 * (1.0 - tmp) * RAKAP
                tmp = tmp * 315.0
                free = tmp * (tey_z + tez)
                rkt = s["rka"]
            else:
                f1 = np.maximum(0.0, (sigl - SIGB) * s["rsgb"])
                tey = s["ap0k"] * (315.0 - tab["tey"])
                tmp = tey - tab["tez"] * (np.log(pkz[:, :, k]) + s["algpk"])
                free = tmp * pkz[:, :, k]
                rkt = s["rka"] + (s["rks"] - s["rka"]) * f1 * tab["cos4"]
            teq_t = np.maximum(T0, free)
            new_t = td + rkt * (teq_t - p) / (1.0 + rkt) * s["rdt"]
            teq = np.where(meso, teq_m, np.where(strat, teq_s, teq_t))
            t_dt[:, :, k] = np.where(meso, new_m, np.where(strat, new_s, new_t))
            # bottom friction (:187-196), the troposphere branch only
            sg = (sigl - SIGB) * s["rsgb"] * s["rkv"]
            fr = tropo & (sg > 0.0)
            tmp = sg / (1.0 + sg) * s["rdt"]
            u1, v1 = ua[:, :, k] + u_dt[:, :, k], va[:, :, k] + v_dt[:, :, k]
            u_dt[:, :, k] = np.where(fr, u_dt[:, :, k] - u1 * tmp, u_dt[:, :, k])
            v_dt[:, :, k] = np.where(fr, v_dt[:, :, k] - v1 * tmp, v_dt[:, :, k])
            cnt["meso"] += int(meso.sum())
            cnt["strat"] += int(strat.sum())
            cnt["tropo"] += int(tropo.sum())
            cnt["friction"] += int(fr.sum())
            cnt["no_friction"] += int((~fr).sum())
            cnt["teq_t0"] += int((tropo & (free <= T0)).sum())
            cnt["teq_free"] += int((tropo & (free > T0)).sum())
            if teq_out is not None:
                teq_out[:, :, k] = teq
            pl1, teq1 = pl, teq
    return cnt


def friction_mask(bd, km, pr, o):
    """True where the bottom friction acts: the troposphere branch with sigl > sigb"""
    c = {n: o[n].copy(order="F") for n in o}
    before = bd.view(c["u_dt"], "A", bd.is_, bd.ie, bd.js, bd.je).copy()
    s = scalars(pr["pdt"], pr["radius"], pr["rd_zur"], pr["pi"])
    delp = bd.view(c["delp"], "A", bd.is_, bd.ie, bd.js, bd.je)
    pes = c["pe"][1:-1, km, 1:-1]
    m = np.zeros(before.shape, dtype=bool)
    for k in range(km):
        pl = delp[:, :, k] / (c["peln"][:, k + 1, :] - c["peln"][:, k, :])
        tropo = ~(pl <= 100.0e2) if pr["strat"] else np.ones(pl.shape, dtype=bool)
        m[:, :, k] = tropo & ((pl / pes - SIGB) * s["rsgb"] * s["rkv"] > 0.0)
    return m


def age_of_air(bd, km, time, pe, q):
    """:209-245, in place on q (A x km)"""
    qa = bd.view(q, "A", bd.is_, bd.ie, bd.js, bd.je)
    if time < 1.0e-6:
        qa[...] = 0.0
        return
    ascale = 5.0e-6 / 60.0
    for k in range(km):
        src = pe[1:-1, k, 1:-1] >= 75000.0
        qa[:, :, k] = np.where(src, ascale * time, qa[:, :, k])
