"""numpy restatement of the Reed-Jablonowski simple physics and the terminator chemistry (driver/solo/fv_phys.F90: the column loop
:551-602, reed_sim_physics :2332-2817, DCMIP2016_terminator_advance :2819-2894), written from the Fortran: the same expressions in the
same order of floating-point operations, vectorised over the columns, the k-loops as loops.  tests/test_reed_hostemu.py holds it to
the outputs of the reference's compiled Fortran (tests/golden/reed/*.npz).

Every log, exp and x**y goes through a Math object.  Math() is numpy's; Math(seed) perturbs each result by one unit in the last place
for log and exp and by (1 + |y ln x|) units for the power, with seeded signs -- what tests/test_fv3_math.py allows include/fv3_math.h
and what exp(y log x) composes to: tests/golden/make_reed_golden.py --measure runs it to find what a last bit of the reference's own
libm is worth in each output, the figure the tests' bounds are ten times of.

Where the reference branches -- q > qsat, wind < v20, pint >= pbltop, zint > pbltopz -- the branch is decided by inputs alone (pint, zint
from peln or delz, wind through an exact sqrt) or is continuous across its threshold (q > qsat: tmp -> 0), so a last-bit difference of
a transcendental moves no result by more than its own size; reed_sim_physics counts the cells whose qsat comparison a perturbation
could flip (|q - qsat| within 4 ulp) in cnt["qsat_edge"]."""
from __future__ import annotations

import numpy as np


class Math:
    def __init__(self, seed=None):
        self.rng = None if seed is None else np.random.default_rng(seed)

    def _p(self, y, ulps):
        if self.rng is None:
            return y
        y = np.asarray(y, dtype=np.float64)
        sign = self.rng.choice([-1.0, 1.0], size=y.shape)
        return y + sign * ulps * np.spacing(np.abs(y))

    def log(self, x):
        return self._p(np.log(x), 1.0)

    def exp(self, x):
        return self._p(np.exp(x), 1.0)

    def pow(self, x, y):
        return self._p(np.power(x, y), 1.0 + np.abs(y * np.log(x)))


def module_consts(k):
    """fv_phys.F90:74-85"""
    tice = 273.16
    dc_vap = k["cp_vapor"] - k["c_liq"]
    return dict(e0=610.71, tice=tice, dc_vap=dc_vap, Lv0=k["hlv"] - dc_vap * tice)


def reed_planes(lat, test, k, M=None):
    """Tsurf (:2571-2586) and the SST factor of qsats (:2719) -> (Tsurf, sstf)"""
    M = M or Math()
    lat = np.asarray(lat, dtype=np.float64)
    mc = module_consts(k)
    pi, rair, a, omega_r = k["pi"], k["rdgas"], k["radius"], k["omega"]
    zvir = (461.5 / rair) - 1.0
    T00, u0, latw, eta0, q0 = 288.0, 35.0, 2.0 * pi / 9.0, 0.252, 0.021
    etav = (1.0 - eta0) * 0.5 * pi
    if test == 1:
        sl, cl = np.sin(lat), np.cos(lat)
        s2 = sl * sl
        s3 = s2 * sl
        s6 = s3 * s3                                                       # x**6 as the reference's compiler forms it
        c2 = cl * cl
        c3 = c2 * cl
        x = lat / latw
        x2 = x * x
        Tsurf = (T00 + pi * u0 / rair * 1.5 * np.sin(etav) * np.power(np.cos(etav), 0.5) *
                 ((-(2.0 * s6 * (c2 + 1.0 / 3.0)) + 10.0 / 63.0) * u0 * np.power(np.cos(etav), 1.5) +
                  (8.0 / 5.0 * c3 * (s2 + 2.0 / 3.0) - pi / 4.0) * a * omega_r * 0.5)) / (1.0 + zvir * q0 * np.exp(-(x2 * x2)))
    elif test == 0:
        Tsurf = np.full(lat.shape, 302.15)
    else:
        Tsurf = np.full(lat.shape, 1.0e25)
    tice = mc["tice"]
    sstf = M.exp((mc["dc_vap"] * M.log(Tsurf / tice) + mc["Lv0"] * (Tsurf - tice) / (Tsurf * tice)) / k["rvgas"])
    return Tsurf, sstf


def reed_sim_physics(pr, lat, t, q, u, v, pmid, pint, pdel, rpdel, ps, zint, precl, M, cnt):
    """reed_sim_physics on (n, pver) arrays; t, q, u, v, precl are updated in place -> (dudt, dvdt, dtdt, dqdt), or None for test 2"""
    k = pr["consts"]
    test = pr["reed_test"]
    if test == 2:                                                          # :2506
        return None
    n, pver = t.shape
    dtime = pr["pdt"]
    mc = module_consts(k)
    e0 = mc["e0"]
    gravit, rair, cpair = k["grav"], k["rdgas"], k["cp_air"]
    rh2o, latvap = 461.5, 2.5e6
    epsilo = rair / rh2o
    zvir = (rh2o / rair) - 1.0
    C, sqC, T0, rhow = 0.0011, np.sqrt(0.0011), 273.16, 1000.0
    Cd0, Cd1, Cm, v20, p0 = 0.0007, 0.000065, 0.002, 20.0, 100000.0
    pbltop, pbltopz, pblconst = 85000.0, 1000.0, 10000.0
    dlnpint = M.log(ps) - M.log(pint[:, pver - 1])                        # :2562-2563
    za = rair / gravit * t[:, pver - 1] * (1.0 + zvir * q[:, pver - 1]) * 0.5 * dlnpint
    Tsurf, sstf = reed_planes(lat, test, k, M)
    dtdt, dqdt, dudt, dvdt = (np.zeros((n, pver)) for _ in range(4))
    if pr["do_reed_cond"]:                                                 # :2608-2632
        for kk in range(pver):
            qsat = epsilo * e0 / pmid[:, kk] * M.exp(-(latvap / rh2o * ((1.0 / t[:, kk]) - 1.0 / T0)))
            sat = q[:, kk] > qsat
            cnt["sat"] += int(sat.sum())
            cnt["unsat"] += int((~sat).sum())
            cnt["qsat_edge"] += int((np.abs(q[:, kk] - qsat) <= 4.0 * np.spacing(qsat)).sum())
            with np.errstate(all="ignore"):
                tmp = 1.0 / dtime * (q[:, kk] - qsat) / (1.0 + (latvap / cpair) * (epsilo * latvap * qsat / (rair * (t[:, kk] * t[:, kk]))))
            dtdt[:, kk] = np.where(sat, dtdt[:, kk] + latvap / cpair * tmp, dtdt[:, kk])
            dqdt[:, kk] = np.where(sat, dqdt[:, kk] - tmp, dqdt[:, kk])
            precl[:] = np.where(sat, precl + tmp * pdel[:, kk] / (gravit * rhow), precl)
        for kk in range(pver):
            t[:, kk] = t[:, kk] + dtdt[:, kk] * dtime
            q[:, kk] = q[:, kk] + dqdt[:, kk] * dtime
    if pr["reed_cond_only"]:                                               # :2635
        return dudt, dvdt, dtdt, dqdt
    b = pver - 1
    wind = np.sqrt(u[:, b] * u[:, b] + v[:, b] * v[:, b])                  # :2655
    slow = wind < v20
    cnt["wind_lt_v20"] += int(slow.sum())
    cnt["wind_ge_v20"] += int((~slow).sum())
    Cd = np.where(slow, Cd0 + Cd1 * wind, Cm)
    Km, Ke = np.zeros((n, pver + 1)), np.zeros((n, pver + 1))
    if pr["reed_alt_mxg"]:                                                 # :2660-2678
        for kk in range(pver + 1):
            hi = zint[:, kk] > pbltopz
            if 1 <= kk <= pver - 1:                                        # the interfaces the solve reads
                cnt["z_above"] += int(hi.sum())
                cnt["z_below"] += int((~hi).sum())
            f = 1.0 - zint[:, kk] / pbltopz
            Km[:, kk] = np.where(hi, 0.0, 0.4 * np.sqrt(Cd) * wind * zint[:, kk] * (f * f))
            Ke[:, kk] = np.where(hi, 0.0, 0.4 * sqC * wind * zint[:, kk] * (f * f))
    else:                                                                  # :2682-2703
        Ke[:, pver] = C * wind * za
        Km[:, pver] = np.where(slow, Cd * wind * za, Cm * wind * za)
        for kk in range(pver):
            low = pint[:, kk] >= pbltop
            if 1 <= kk <= pver - 1:
                cnt["p_below"] += int(low.sum())
                cnt["p_above"] += int((~low).sum())
            d = pbltop - pint[:, kk]
            e = M.exp(-((d * d) / (pblconst * pblconst)))
            Km[:, kk] = np.where(low, Km[:, pver], Km[:, pver] * e)
            Ke[:, kk] = np.where(low, Ke[:, pver], Ke[:, pver] * e)
    # :2717-2733
    qsats = epsilo * e0 / ps * sstf
    den_m = 1.0 + Cd * wind * dtime / za
    den_e = 1.0 + C * wind * dtime / za
    dudt[:, b] = dudt[:, b] + (u[:, b] / den_m - u[:, b]) / dtime
    dvdt[:, b] = dvdt[:, b] + (v[:, b] / den_m - v[:, b]) / dtime
    u[:, b] = u[:, b] / den_m
    v[:, b] = v[:, b] / den_m
    a_t = C * wind * Tsurf * dtime / za
    dtdt[:, b] = dtdt[:, b] + ((t[:, b] + a_t) / den_e - t[:, b]) / dtime
    t[:, b] = (t[:, b] + a_t) / den_e
    a_q = C * wind * qsats * dtime / za
    dqdt[:, b] = dqdt[:, b] + ((q[:, b] + a_q) / den_e - q[:, b]) / dtime
    q[:, b] = (q[:, b] + a_q) / den_e
    # :2743-2767
    CA, CC, CAm, CCm = (np.zeros((n, pver)) for _ in range(4))
    CE, CEm, CFu, CFv, CFt, CFq = (np.zeros((n, pver + 1)) for _ in range(6))
    for kk in range(pver - 1):
        rho = pint[:, kk + 1] / (rair * (t[:, kk + 1] + t[:, kk]) / 2.0)
        dpm = pmid[:, kk + 1] - pmid[:, kk]
        CAm[:, kk] = rpdel[:, kk] * dtime * gravit * gravit * Km[:, kk + 1] * rho * rho / dpm
        CCm[:, kk + 1] = rpdel[:, kk + 1] * dtime * gravit * gravit * Km[:, kk + 1] * rho * rho / dpm
        CA[:, kk] = rpdel[:, kk] * dtime * gravit * gravit * Ke[:, kk + 1] * rho * rho / dpm
        CC[:, kk + 1] = rpdel[:, kk + 1] * dtime * gravit * gravit * Ke[:, kk + 1] * rho * rho / dpm
    kap = rair / cpair
    # the reference forms (p0/pmid(k))**kap at :2776 and again at :2807 and :2810, (pmid(k)/p0)**kap at :2809 and :2811 (:2793-2794): the
    # same operands each time, so one call each here -- a perturbed Math then perturbs every use alike, as a libm would
    pwi = [M.pow(p0 / pmid[:, kk], kap) for kk in range(pver)]
    pwf = [M.pow(pmid[:, kk] / p0, kap) for kk in range(pver)]
    for kk in range(pver - 1, -1, -1):                                     # :2769-2781
        den = 1.0 + CA[:, kk] + CC[:, kk] - CA[:, kk] * CE[:, kk + 1]
        denm = 1.0 + CAm[:, kk] + CCm[:, kk] - CAm[:, kk] * CEm[:, kk + 1]
        CE[:, kk] = CC[:, kk] / den
        CEm[:, kk] = CCm[:, kk] / denm
        CFu[:, kk] = (u[:, kk] + CAm[:, kk] * CFu[:, kk + 1]) / denm
        CFv[:, kk] = (v[:, kk] + CAm[:, kk] * CFv[:, kk + 1]) / denm
        CFt[:, kk] = (pwi[kk] * t[:, kk] + CA[:, kk] * CFt[:, kk + 1]) / den
        CFq[:, kk] = (q[:, kk] + CA[:, kk] * CFq[:, kk + 1]) / den
    pw = pwf[0]                                                            # :2788-2797
    dudt[:, 0] = dudt[:, 0] + (CFu[:, 0] - u[:, 0]) / dtime
    dvdt[:, 0] = dvdt[:, 0] + (CFv[:, 0] - v[:, 0]) / dtime
    u[:, 0] = CFu[:, 0]
    v[:, 0] = CFv[:, 0]
    dtdt[:, 0] = dtdt[:, 0] + (CFt[:, 0] * pw - t[:, 0]) / dtime
    t[:, 0] = CFt[:, 0] * pw
    dqdt[:, 0] = dqdt[:, 0] + (CFq[:, 0] - q[:, 0]) / dtime
    q[:, 0] = CFq[:, 0]
    for kk in range(1, pver):                                              # :2801-2815
        un = CEm[:, kk] * u[:, kk - 1] + CFu[:, kk]
        vn = CEm[:, kk] * v[:, kk - 1] + CFv[:, kk]
        dudt[:, kk] = dudt[:, kk] + (un - u[:, kk]) / dtime
        dvdt[:, kk] = dvdt[:, kk] + (vn - v[:, kk]) / dtime
        u[:, kk] = un
        v[:, kk] = vn
        tn = (CE[:, kk] * t[:, kk - 1] * pwi[kk - 1] + CFt[:, kk]) * pwf[kk]
        dtdt[:, kk] = dtdt[:, kk] + (tn - t[:, kk]) / dtime
        t[:, kk] = tn
        qn = CE[:, kk] * q[:, kk - 1] + CFq[:, kk]
        dqdt[:, kk] = dqdt[:, kk] + (qn - q[:, kk]) / dtime
        q[:, kk] = qn
    return dudt, dvdt, dtdt, dqdt


def new_counts():
    return {n: 0 for n in ("sat", "unsat", "qsat_edge", "wind_lt_v20", "wind_ge_v20", "z_above", "z_below", "p_above", "p_below", "q_neg")}


def reed_wrapper(bd, km, pr, o, M=None):
    """the column loop of do_reed_sim_phys (:551-602) on the library's layouts, in place: o["u_dt"], o["v_dt"] (A x km), o["t_dt"],
    o["q_dt"] (is:ie, js:je, km; the sphum plane), o["rain"] (is:ie, js:je).  o["q"] is the sphum tracer (A x km).  -> branch counts"""
    M = M or Math()
    k = pr["consts"]
    cnt = new_counts()
    c = lambda a: bd.view(a, "A", bd.is_, bd.ie, bd.js, bd.je)      # noqa: E731
    n = bd.nx * bd.ny
    col = lambda a: np.ascontiguousarray(a).reshape(n, -1).copy()      # noqa: E731   (i, j, k) -> (column, k)
    zvir = k["rvgas"] / k["rdgas"] - 1.0
    rgrav = 1.0 / k["grav"]
    dp2 = col(c(o["delp"]))
    rdelp = 1.0 / dp2
    u2, v2, t2 = col(c(o["ua"])), col(c(o["va"])), col(c(o["pt"]))
    qraw = col(c(o["q"]))
    cnt["q_neg"] += int((qraw < 0.0).sum())
    q2 = np.maximum(0.0, qraw)
    peln = col(np.transpose(o["peln"], (0, 2, 1)))                         # (column, km + 1)
    pe = col(np.transpose(o["pe"][1:-1, :, 1:-1], (0, 2, 1)))
    pm = dp2 / (peln[:, 1:] - peln[:, :-1])
    zint = np.zeros((n, km + 1))
    zint[:, km] = col(c(o["phis"]))[:, 0] * rgrav                          # :565, with the k the loop above leaves
    ptr = col(c(o["pt"]))
    for kk in range(km - 1, -1, -1):
        if pr["hydrostatic"]:
            zint[:, kk] = zint[:, kk + 1] + k["rdgas"] * rgrav * ptr[:, kk] * (1.0 + zvir * qraw[:, kk]) * (peln[:, kk + 1] - peln[:, kk])
        else:
            zint[:, kk] = zint[:, kk + 1] - col(o["delz"])[:, kk]
    rain2 = np.zeros(n)
    lat = np.ascontiguousarray(o["lat"]).reshape(n)
    out = reed_sim_physics(pr, lat, t2, q2, u2, v2, pm, pe, dp2, rdelp, pe[:, km], zint, rain2, M, cnt)
    if out is not None:                                                    # (test 2: the reference adds undefined values)
        shp = (bd.nx, bd.ny, km)
        du2, dv2, dt2, dq2 = (a.reshape(shp) for a in out)
        c(o["u_dt"])[...] = c(o["u_dt"]) + du2
        c(o["v_dt"])[...] = c(o["v_dt"]) + dv2
        o["t_dt"][...] = o["t_dt"] + dt2
        o["q_dt"][...] = o["q_dt"] + dq2
    if pr["do_reed_cond"]:
        o["rain"][...] = (rain2 * 8.64e7).reshape(bd.nx, bd.ny)
    return cnt


def term_k1(agrid, pi):
    """k1 of :2873 over the A layout"""
    lc, thc = 5.0 * pi / 3.0, pi / 9.0
    lon, lat = agrid[..., 0], agrid[..., 1]
    return np.maximum(0.0, np.sin(lat) * np.sin(thc) + np.cos(lat) * np.cos(thc) * np.cos(lon - lc))


def terminator_advance(pdt, fill, k1, cl, cl2, M=None):
    """DCMIP2016_terminator_advance on the whole planes cl, cl2 (A x km), in place; k1 (A) -> count of night cells (el = 4 k2)"""
    M = M or Math()
    k2 = 1.0
    rdt = 1.0 / pdt
    qCl, qCl2 = cl.copy(), cl2.copy()
    if fill:
        dq = np.minimum(qCl2, 0.0) * 2.0 - np.minimum(qCl, 0.0)
        qCl = qCl + dq
        qCl2 = qCl2 - dq * 0.5
    r = (k1 / k2 * 0.25)[:, :, None]
    qcly = qCl + 2.0 * qCl2
    D = np.sqrt(r * r + 2.0 * r * qcly)
    expdt = M.exp(-4.0 * k2 * D * pdt)
    day = np.abs(D * k2 * pdt) > 1e-16
    with np.errstate(all="ignore"):
        el = np.where(day, (1.0 - expdt) / D * rdt, 4.0 * k2)
    cl_f = -el * (qCl - D + r) * (qCl + D + r) / (1.0 + expdt + pdt * el * (qCl + r))
    cl[...] = qCl + cl_f * pdt
    cl2[...] = qCl2 - cl_f * 0.5 * pdt
    return int((~day).sum())
