"""numpy restatement of the Kessler warm-rain microphysics (driver/solo/fv_phys.F90: K_warm_rain :1992-2196, kessler_imp :2202-2291;
driver/solo/qs_tables.F90: qs_wat :67-93, qs_wat_init and qs_table_w :95-132), written from the Fortran: the same expressions in
the same order of floating-point operations, vectorised over the columns, the k-loops as loops and in the reference's own
structure -- every level's array of length km, four loops per cycle -- not the one sweep of the kernel.
tests/test_kessler_hostemu.py holds it to the outputs of the reference's compiled Fortran (tests/golden/kessler/*.npz).

Every log, exp, x**y and sqrt goes through a Math object.  Math() is numpy's; Math(seed) perturbs each result by one unit in the
last place for log, exp and sqrt and by (1 + |y ln x|) units for the power, with seeded signs:
tests/golden/make_kessler_golden.py --measure runs it to find what a last bit of the reference's own libm is worth in each output,
the figure the tests' bounds are ten times of.

k_warm_rain returns the counts of the branches taken, which the recorder and one test assert to be non-zero over the recorded
set."""
from __future__ import annotations

import numpy as np

QS_LENGTH = 2621
TICE = 273.16


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

    def sqrt(self, x):
        return self._p(np.sqrt(x), 1.0)

    def pow(self, x, y):
        x = np.asarray(x, dtype=np.float64)
        with np.errstate(divide="ignore"):
            ulps = np.where(x > 0.0, 1.0 + np.abs(y * np.log(np.where(x > 0.0, x, 1.0))), 0.0)
        return self._p(np.power(x, y), ulps)


def module_consts(k):
    """fv_phys.F90:74-85 = qs_tables.F90:32-43"""
    cp_vap = k["cp_vapor"]
    dc_vap = cp_vap - k["c_liq"]
    return dict(e0=610.71, tice=TICE, cv_vap=cp_vap - k["rvgas"], cv_air=k["cp_air"] - k["rdgas"], dc_vap=dc_vap, Lv0=k["hlv"] - dc_vap * TICE)


def qs_table(k, M=None):
    """qs_wat_init, qs_table_w (qs_tables.F90:95-132) -> (table_w, des_w)"""
    M = M or Math()
    mc = module_consts(k)
    tmin = TICE - 160.0
    tem = tmin + 0.1 * np.arange(QS_LENGTH, dtype=np.float64)
    table_w = mc["e0"] * M.exp((mc["dc_vap"] * M.log(tem / TICE) + mc["Lv0"] * (tem - TICE) / (tem * TICE)) / k["rvgas"])
    des_w = np.empty(QS_LENGTH)
    des_w[:-1] = np.maximum(0.0, table_w[1:] - table_w[:-1])
    des_w[-1] = des_w[-2]
    return table_w, des_w


def qs_wat(ta, den, tab, rvgas, cnt=None):
    """qs_wat (qs_tables.F90:67-93) -> (qs, dqdt).  it = int(ap1 - 0.5) = 0 reads the word before des_w in the reference: 0. here"""
    table_w, des_w = tab
    tmin = TICE - 160.0
    ap1 = 10.0 * np.maximum(ta - tmin, 0.0) + 1.0
    if cnt is not None:
        cnt["ta_below_tmin"] += int(np.count_nonzero(ta < tmin))
        cnt["ap1_capped"] += int(np.count_nonzero(ap1 > 2621.0))
    ap1 = np.minimum(2621.0, ap1)
    it = ap1.astype(np.int64)
    es = table_w[it - 1] + (ap1 - it) * des_w[it - 1]
    dem = rvgas * ta * den
    it = (ap1 - 0.5).astype(np.int64)
    assert it.min() >= 0 and it.max() + 1 <= QS_LENGTH
    d0 = np.where(it >= 1, des_w[np.maximum(it, 1) - 1], 0.0)
    dqdt = 10.0 * (d0 + (ap1 - it) * (des_w[it] - d0)) / dem
    return es / dem, dqdt


def fix_negative(q2, q3, cnt):
    """:2052-2062 = :2091-2102, in place"""
    qcon = q2 + q3
    pos = qcon > 0.0
    a = pos & (q2 < 0.0)
    b = pos & ~a & (q3 < 0.0)
    cnt["q2_neg_fixed"] += int(a.sum())
    cnt["q3_neg_fixed"] += int(b.sum())
    cnt["qcon_nonpos"] += int((~pos).sum())
    q3[a] = qcon[a]
    q2[a] = 0.0
    q2[b] = qcon[b]
    q3[b] = 0.0
    return qcon


def kessler_imp(T, qv, qc, qr, drym, dt, dz, moist_kappa, k, tab, cnt, M):
    """kessler_imp (:2202-2291) on arrays (nx, ny, nz), in place -> vr"""
    mc = module_consts(k)
    grav, rdgas = k["grav"], k["rdgas"]
    nz = T.shape[2]
    qr_min, vr_min = 1.0e-8, 1.0e-3
    rho = drym / (grav * dz)
    pc = 3.8e2 / (rho * rdgas * T)
    r = 0.001 * rho
    rqr = r * np.maximum(qr, qr_min)
    vr = 36.34 * M.sqrt(rho[:, :, nz - 1:nz] / rho) * M.exp(0.1364 * M.log(rqr))
    cnt["vr_at_min"] += int(np.count_nonzero(vr < vr_min))
    cnt["vr_above_min"] += int(np.count_nonzero(vr >= vr_min))
    vr = np.maximum(vr_min, vr)
    qr[:, :, 0] = dz[:, :, 0] * qr[:, :, 0] / (dz[:, :, 0] + dt * vr[:, :, 0])
    for l in range(1, nz):
        qr[:, :, l] = (dz[:, :, l] * qr[:, :, l] + qr[:, :, l - 1] * r[:, :, l - 1] * dt * vr[:, :, l - 1] / r[:, :, l]) / (dz[:, :, l] + dt * vr[:, :, l])
    cnt["qr_zero_at_pow"] += int(np.count_nonzero(qr == 0.0))
    assert qr.min() >= 0.0, "qr < 0 reaches qr**.875"
    auto = np.maximum(0.001 * (qc - 0.001), 0.0)
    cnt["autoconversion"] += int(np.count_nonzero(auto > 0.0))
    qrprod = qc - (qc - dt * auto) / (1.0 + dt * 2.2 * M.pow(qr, 0.875))
    qc[...] = qc - qrprod
    qr[...] = qr + qrprod
    rqr = r * np.maximum(qr, qr_min)
    qvs, dqsdt = qs_wat(T, rho, tab, k["rvgas"], cnt)
    if moist_kappa:
        hlvm = (mc["Lv0"] + mc["dc_vap"] * T) / (mc["cv_air"] + qv * mc["cv_vap"] + (qc + qr) * k["c_liq"])
    else:
        hlvm = k["hlv"] / mc["cv_air"]
    prod = (qv - qvs) / (1.0 + dqsdt * hlvm)
    cnt["saturated"] += int(np.count_nonzero(prod > 0.0))
    cnt["subsaturated"] += int(np.count_nonzero(prod < 0.0))
    e1 = dt * (((1.6 + 124.9 * M.pow(rqr, 0.2046)) * M.pow(rqr, 0.525)) / (2.55e6 * pc / (3.8 * qvs) + 5.4e5)) * (np.maximum(qvs - qv, 0.0) / (r * qvs))
    e2 = np.maximum(-prod - qc, 0.0)
    ern = np.minimum(np.minimum(e1, e2), qr)
    cnt["ern_rate"] += int(np.count_nonzero((e1 < e2) & (e1 < qr) & (e1 > 0.0)))
    cnt["ern_deficit"] += int(np.count_nonzero((e2 <= e1) & (e2 < qr) & (e2 > 0.0)))
    cnt["ern_all_rain"] += int(np.count_nonzero((qr <= e1) & (qr <= e2) & (qr > 0.0)))
    dq = np.maximum(prod, -qc)
    cnt["cloud_all_evaporates"] += int(np.count_nonzero(prod < -qc))
    T[...] = T + hlvm * (dq - ern)
    qv[...] = qv - dq + ern
    qc[...] = qc + dq
    qr[...] = qr - ern
    cnt["cloud_with_rain"] += int(np.count_nonzero((qc > 1.0e-6) & (qr > 1.0e-6)))
    cnt["cloud_without_rain"] += int(np.count_nonzero((qc > 1.0e-6) & (qr < 1.0e-7)))
    return vr


COUNTS = ("q2_neg_fixed", "q3_neg_fixed", "qcon_nonpos", "qv_clamped", "qc_clamped", "qr_clamped", "vr_at_min", "vr_above_min", "qr_zero_at_pow",
          "autoconversion", "saturated", "subsaturated", "ern_rate", "ern_deficit", "ern_all_rain", "cloud_all_evaporates", "cloud_with_rain",
          "cloud_without_rain", "ta_below_tmin", "ap1_capped", "rain_reaches_ground")


def n_cycles(pdt, K_cycle):
    """:472-474.  nint rounds halves away from zero"""
    return int(K_cycle) if K_cycle else max(1, int(np.floor(pdt / 30.0 + 0.5)))


def k_warm_rain(bd, km, pr, st, M=None, tab=None):
    """K_warm_rain (:1992-2196) in place on st: ua, va, w, u_dt, v_dt, pt, delp (A x km), q (A x km x nq), delz (is:ie, js:je, km),
    pe (is-1:ie+1, km+1, js-1:je+1), peln (is:ie, km+1, js:je), pk (is:ie, js:je, km+1), ps (A), rain (is:ie, js:je) -> the branch counts.
    pr: pdt, K_cycle, K_sedi_transport, do_K_sedi_w, do_K_sedi_heat, hydrostatic, moist_kappa, sphum, liq_wat, rainwat (1-based), consts.
    drym of every level is left in st["drym"] (is:ie, js:je, km) for the conservation checks."""
    M = M or Math()
    k = pr["consts"]
    mc = module_consts(k)
    tab = tab or qs_table(k, M)      # (the table is the reference's exp and log as well: a perturbed run perturbs it)
    cnt = dict.fromkeys(COUNTS, 0)
    grav, rdgas, c_liq = k["grav"], k["rdgas"], k["c_liq"]
    cv_air, cv_vap = mc["cv_air"], mc["cv_vap"]
    dt = pr["pdt"]
    ncyc = n_cycles(dt, pr["K_cycle"])
    sdt = dt / float(ncyc)
    rgrav = 1.0 / grav
    zvir = k["rvgas"] / rdgas - 1.0
    qv_min, qc_min = 1.0e-7, 1.0e-8
    cv = lambda a: bd.view(a, "A", bd.is_, bd.ie, bd.js, bd.je)      # noqa: E731
    sp, lw, rw = pr["sphum"] - 1, pr["liq_wat"] - 1, pr["rainwat"] - 1
    u, v, w = cv(st["ua"]), cv(st["va"]), (cv(st["w"]) if st.get("w") is not None else None)
    pt, dp, q = cv(st["pt"]), cv(st["delp"]), cv(st["q"])
    peln = np.transpose(st["peln"], (0, 2, 1))
    delz = st.get("delz")
    if pr["hydrostatic"]:
        dz = rdgas * rgrav * pt * (1.0 + zvir * q[..., sp]) * (peln[:, :, 1:] - peln[:, :, :-1])
    else:
        dz = -delz
    dm = dp.copy()
    qa, qb, qc = q[..., sp].copy(), q[..., lw].copy(), q[..., rw].copy()
    q1, q2, q3 = qa * dm, qb * dm, qc * dm
    fix_negative(q2, q3, cnt)
    drym = dm - (q1 + q2 + q3)
    qa, qb, qc = q1 / drym, q2 / drym, q3 / drym
    q1, q2, q3 = np.maximum(qa, qv_min), np.maximum(qb, qc_min), np.maximum(qc, qc_min)
    cnt["qv_clamped"] += int(np.count_nonzero(qa < qv_min))
    cnt["qc_clamped"] += int(np.count_nonzero(qb < qc_min))
    cnt["qr_clamped"] += int(np.count_nonzero(qc < qc_min))
    qa, qb, qc = q1 - qa, q2 - qb, q3 - qc
    t1, u1, v1 = pt.copy(), u.copy(), v.copy()
    w1 = w.copy() if w is not None else None
    rain = np.zeros(dm.shape[:2])
    for _ in range(ncyc):
        qcon = fix_negative(q2, q3, cnt)
        q0 = q1 + qcon
        vr = kessler_imp(t1, q1, q2, q3, drym, sdt, dz, pr["moist_kappa"], k, tab, cnt, M)
        m1 = np.empty_like(dm)
        m1[:, :, 0] = drym[:, :, 0] * (q0[:, :, 0] - (q1[:, :, 0] + q2[:, :, 0] + q3[:, :, 0]))
        for l in range(1, km):
            m1[:, :, l] = m1[:, :, l - 1] + drym[:, :, l] * (q0[:, :, l] - (q1[:, :, l] + q2[:, :, l] + q3[:, :, l]))
        cnt["rain_reaches_ground"] += int(np.count_nonzero(m1[:, :, km - 1] > 0.0))
        rain = rain + np.maximum(0.0, m1[:, :, km - 1]) / grav
        if pr["K_sedi_transport"]:
            if pr["do_K_sedi_w"]:
                for l in range(1, km):
                    w1[:, :, l] = (dm[:, :, l] * w1[:, :, l] - m1[:, :, l - 1] * vr[:, :, l - 1] + m1[:, :, l] * vr[:, :, l]) / \
                                  (dm[:, :, l] + m1[:, :, l - 1] - m1[:, :, l])
            for l in range(1, km):
                fac1 = m1[:, :, l - 1] / (dm[:, :, l] + m1[:, :, l - 1])
                fac2 = 1.0 - fac1
                u1[:, :, l] = fac1 * u1[:, :, l - 1] + fac2 * u1[:, :, l]
                v1[:, :, l] = fac1 * v1[:, :, l - 1] + fac2 * v1[:, :, l]
        if pr["do_K_sedi_heat"]:
            dgz = -0.5 * grav * delz
            cvn = cv_air + q1 * cv_vap + (q2 + q3) * c_liq
            for l in range(1, km):
                cvm = cvn[:, :, l] - c_liq * (m1[:, :, l - 1] - m1[:, :, l]) / drym[:, :, l]
                t1[:, :, l] = (drym[:, :, l] * cvm * t1[:, :, l] + m1[:, :, l - 1] * c_liq * t1[:, :, l - 1] + dgz[:, :, l] * (m1[:, :, l - 1] + m1[:, :, l])) / \
                              (drym[:, :, l] * cvn[:, :, l] + m1[:, :, l] * c_liq)
    cv(st["u_dt"])[...] = cv(st["u_dt"]) + (u1 - u) / dt
    cv(st["v_dt"])[...] = cv(st["v_dt"]) + (v1 - v) / dt
    u[...] = u1
    v[...] = v1
    if w is not None:
        w[...] = w1
    pt[...] = t1
    q1, q2, q3 = (q1 + qa) * drym, (q2 + qb) * drym, (q3 + qc) * drym
    dp[...] = drym + q1 + q2 + q3
    q[..., sp], q[..., lw], q[..., rw] = q1 / dp, q2 / dp, q3 / dp
    pe = st["pe"]
    for l in range(1, km + 1):
        pe[1:-1, l, 1:-1] = pe[1:-1, l - 1, 1:-1] + dp[:, :, l - 1]
        st["peln"][:, l, :] = M.log(pe[1:-1, l, 1:-1])
        st["pk"][:, :, l] = M.exp(k["kappa"] * st["peln"][:, l, :])
    cv(st["ps"])[...] = pe[1:-1, km, 1:-1]
    st["rain"][...] = rain
    st["drym"] = drym
    return cnt
