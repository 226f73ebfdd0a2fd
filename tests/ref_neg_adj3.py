"""neg_adj3 and fillq restated in numpy from the Fortran (model/fv_sg.F90:968-1370), the checker of fv3_neg_adj3.

Like the oracle under oracle/, this restatement is UNPINNED: nothing compiled from the reference stands behind it (neg_adj3 does not
build outside the model), it was written from the source text, line ranges cited below, with the reference's order of operations.  It
is vectorised over (i, j) and sequential in k where the Fortran is, so every cell sees the arithmetic of the Fortran loop nest.

``neg_adj3(...)`` works in place on arrays WITH halos (A kind, Fortran order) over the compute domain of ``bd`` and returns a dict with
one count per branch taken -- the tests assert that their inputs reach every one of them before they compare anything.
"""
from __future__ import annotations

import numpy as np

BRANCHES = (
    "ice_qi_neg", "ice_qs_neg", "ice_to_graupel",                       # :1061-1075
    "g_from_snow", "g_from_ice", "g_from_rain", "g_from_cloud", "g_from_vapor",   # :1079-1111
    "liq_qr_neg", "liq_ql_neg",                                         # :1117-1124
    "rain_from_graupel", "rain_from_ice", "rain_quirk_skip", "rain_from_vapor",   # :1126-1148
    "fillq_g_acting", "fillq_g_early", "fillq_r_acting", "fillq_r_early",          # :1208-1234, :1337-1370
    "qv_top", "qv_int_donor", "qv_int_no_donor", "qv_bottom_donor", "qv_bottom_no_donor",   # :1239-1286
    "qa_interior", "qa_bottom_donor", "qa_bottom_no_donor", "qa_bottom_clipped",           # :1289-1321
)

# the constants a SHiELD build hands the routine (constants_mod GFDL values; gfdl_mp.F90:136-137)
CONSTS = dict(rdgas=287.04, rvgas=461.50, grav=9.80, cp_air=287.04 / (2.0 / 7.0), cp_vapor=4.0 * 461.50, hlv=2.500e6, hlf=3.34e5,
              c_liq=4.218e3, c_ice=2.106e3)


def module_parameters(hydrostatic, c):
    """fv_sg.F90:43-70 and :1004-1014 (the form without ENG_CNV_OLD)"""
    t_ice, hlv0, hlf0 = 273.16, 2.5e6, 3.3358e5
    cv_vap = c["cp_vapor"] - c["rvgas"]
    dc_ice = c["c_liq"] - c["c_ice"]
    li0 = hlf0 - dc_ice * t_ice
    if hydrostatic:
        d0_vap = c["cp_vapor"] - c["c_liq"]
        lv00 = hlv0 - d0_vap * t_ice
    else:
        d0_vap = cv_vap - c["c_liq"]
        lv00 = hlv0 - d0_vap * t_ice - c["rvgas"] * t_ice
    return dict(cv_vap=cv_vap, dc_ice=dc_ice, li0=li0, d0_vap=d0_vap, lv00=lv00, cv_air=c["cp_air"] - c["rdgas"])


def _where(m, a, b):
    return np.where(m, a, b)


def pointwise(hydrostatic, dp, pt, qv, ql, qr, qi, qs, qg, cnt, c):
    """:1020-1204 on compute-domain views (nx, ny, npz), in place.  Each `if` of the Fortran is a mask; a masked update computes the
    Fortran's expression for every cell and keeps it where the branch is taken."""
    mp = module_parameters(hydrostatic, c)
    qv2, ql2, qi2, qs2, qr2, qg2, pt2 = (a.copy() for a in (qv, ql, qi, qs, qr, qg, pt))
    qr_in = qr.copy()
    with np.errstate(all="ignore"):
        if hydrostatic:   # :1038-1039
            lcpk = np.full_like(pt2, c["hlv"] / c["cp_air"])
            icpk = np.full_like(pt2, c["hlf"] / c["cp_air"])
        else:             # :1046-1050
            q_liq = np.maximum(0.0, ql2 + qr2)
            q_sol = np.maximum(0.0, qi2 + qs2)
            cpm = (1.0 - (qv2 + q_liq + q_sol)) * mp["cv_air"] + qv2 * mp["cv_vap"] + q_liq * c["c_liq"] + q_sol * c["c_ice"]
            lcpk = (mp["lv00"] + mp["d0_vap"] * pt2) / cpm
            icpk = (mp["li0"] + mp["dc_ice"] * pt2) / cpm
        # ice phase :1061-1075
        qsum = qi2 + qs2
        pos = qsum > 0.0
        a = pos & (qi2 < 0.0)
        b = pos & ~(qi2 < 0.0) & (qs2 < 0.0)
        e = ~pos
        cnt["ice_qi_neg"] += int(a.sum())
        cnt["ice_qs_neg"] += int(b.sum())
        cnt["ice_to_graupel"] += int((e & (qsum < 0.0)).sum())
        qi_n = _where(a, 0.0, _where(b, qsum, _where(e, 0.0, qi2)))
        qs_n = _where(a, qsum, _where(b, 0.0, _where(e, 0.0, qs2)))
        qg2 = _where(e, qg2 + qsum, qg2)
        qi2, qs2 = qi_n, qs_n
        # graupel from snow then ice :1079-1089
        m = qg2 < 0.0
        dq = np.minimum(qs2, -qg2)
        cnt["g_from_snow"] += int((m & (dq > 0.0)).sum())
        qs2 = _where(m, qs2 - dq, qs2)
        qg2 = _where(m, qg2 + dq, qg2)
        m2 = m & (qg2 < 0.0)
        dq = np.minimum(qi2, -qg2)
        cnt["g_from_ice"] += int((m2 & (dq > 0.0)).sum())
        qi2 = _where(m2, qi2 - dq, qi2)
        qg2 = _where(m2, qg2 + dq, qg2)
        # from rain :1092-1097
        m = (qg2 < 0.0) & (qr2 > 0.0)
        dq = np.minimum(qr2, -qg2)
        cnt["g_from_rain"] += int(m.sum())
        qg2 = _where(m, qg2 + dq, qg2)
        qr2 = _where(m, qr2 - dq, qr2)
        pt2 = _where(m, pt2 + dq * icpk, pt2)
        # from cloud water :1099-1104
        m = (qg2 < 0.0) & (ql2 > 0.0)
        dq = np.minimum(ql2, -qg2)
        cnt["g_from_cloud"] += int(m.sum())
        qg2 = _where(m, qg2 + dq, qg2)
        ql2 = _where(m, ql2 - dq, ql2)
        pt2 = _where(m, pt2 + dq * icpk, pt2)
        # last resort: vapor :1106-1111
        m = (qg2 < 0.0) & (qv2 > 0.0)
        dq = np.minimum(0.999 * qv2, -qg2)
        cnt["g_from_vapor"] += int(m.sum())
        qg2 = _where(m, qg2 + dq, qg2)
        qv2 = _where(m, qv2 - dq, qv2)
        pt2 = _where(m, pt2 + dq * (icpk + lcpk), pt2)
        # liquid phase :1116-1149
        qsum = ql2 + qr2
        pos = qsum > 0.0
        a = pos & (qr2 < 0.0)
        b = pos & ~(qr2 < 0.0) & (ql2 < 0.0)
        e = ~pos
        cnt["liq_qr_neg"] += int(a.sum())
        cnt["liq_ql_neg"] += int(b.sum())
        ql_n = _where(a, qsum, _where(b, 0.0, _where(e, 0.0, ql2)))
        qr_n = _where(a, 0.0, _where(b, qsum, _where(e, qsum, qr2)))
        ql2, qr2 = ql_n, qr_n
        dq = np.minimum(np.maximum(0.0, qg2), -qr2)          # :1129-1132
        cnt["rain_from_graupel"] += int((e & (dq > 0.0)).sum())
        qr2 = _where(e, qr2 + dq, qr2)
        qg2 = _where(e, qg2 - dq, qg2)
        pt2 = _where(e, pt2 - dq * icpk, pt2)
        m = e & (qr_in < 0.0)                                 # :1133: qr(i,j,k), not qr2
        dq = np.minimum(qi2 + qs2, -qr2)
        cnt["rain_from_ice"] += int((m & (dq > 0.0)).sum())
        # the quirk bites where the level came in with qr >= 0, the else branch still left rain negative and ice could have paid
        cnt["rain_quirk_skip"] += int((e & ~(qr_in < 0.0) & (qr2 < 0.0) & (qi2 + qs2 > 0.0)).sum())
        qr2 = _where(m, qr2 + dq, qr2)
        dq1 = np.minimum(dq, qs2)
        qs_n = _where(m, qs2 - dq1, qs2)
        qi2 = _where(m, qi2 + dq1 - dq, qi2)
        qs2 = qs_n
        pt2 = _where(m, pt2 - dq * icpk, pt2)
        m = e & (qr2 < 0.0) & (qv2 > 0.0)                     # :1143-1148
        dq = np.minimum(0.999 * qv2, -qr2)
        cnt["rain_from_vapor"] += int(m.sum())
        qv2 = _where(m, qv2 - dq, qv2)
        qr2 = _where(m, qr2 + dq, qr2)
        pt2 = _where(m, pt2 + dq * lcpk, pt2)
    for dst, src in ((qv, qv2), (ql, ql2), (qi, qi2), (qs, qs2), (qr, qr2), (qg, qg2), (pt, pt2)):   # :1192-1202
        dst[...] = src


def fillq(q, dp, cnt, name):
    """:1337-1370 on (nx, ny, km) views, in place; columns side by side, k in the Fortran's order"""
    km = q.shape[2]
    sum1 = np.zeros(q.shape[:2])
    for k in range(km):                                       # :1345-1350
        sum1 = np.where(q[:, :, k] > 0.0, sum1 + q[:, :, k] * dp[:, :, k], sum1)
    go = ~(sum1 < 1.0e-12)                                    # :1351
    has_neg = (q < 0.0).any(axis=2)
    cnt[f"fillq_{name}_early"] += int((~go & has_neg).sum())
    cnt[f"fillq_{name}_acting"] += int((go & has_neg).sum())
    sum2 = np.zeros_like(sum1)
    for k in range(km - 1, -1, -1):                           # :1353-1360
        v, d = q[:, :, k].copy(), dp[:, :, k]
        m = go & (v < 0.0) & (sum1 > 0.0)
        dq = np.minimum(sum1, -v * d)
        sum1 = np.where(m, sum1 - dq, sum1)
        sum2 = np.where(m, sum2 + dq, sum2)
        q[:, :, k] = np.where(m, v + dq / d, v)
    for k in range(km - 1, -1, -1):                           # :1361-1367
        v, d = q[:, :, k].copy(), dp[:, :, k]
        m = go & (v > 0.0) & (sum2 > 0.0)
        dq = np.minimum(sum2, v * d)
        sum2 = np.where(m, sum2 - dq, sum2)
        q[:, :, k] = np.where(m, v - dq / d, v)


def fix_vapor(qv, dp, cnt):
    """:1239-1286"""
    kb = qv.shape[2]
    m = qv[:, :, 0] < 0.0                                     # top :1244-1247
    cnt["qv_top"] += int(m.sum())
    qv[:, :, 1] = np.where(m, qv[:, :, 1] + qv[:, :, 0] * dp[:, :, 0] / dp[:, :, 1], qv[:, :, 1])
    qv[:, :, 0] = np.where(m, 0.0, qv[:, :, 0])
    for k in range(1, kb - 1):                                # :1255-1267
        m = (qv[:, :, k] < 0.0) & (qv[:, :, k - 1] > 0.0)
        cnt["qv_int_donor"] += int(m.sum())
        dq = np.minimum(-qv[:, :, k] * dp[:, :, k], qv[:, :, k - 1] * dp[:, :, k - 1])
        qv[:, :, k - 1] = np.where(m, qv[:, :, k - 1] - dq / dp[:, :, k - 1], qv[:, :, k - 1])
        qv[:, :, k] = np.where(m, qv[:, :, k] + dq / dp[:, :, k], qv[:, :, k])
        m2 = qv[:, :, k] < 0.0
        cnt["qv_int_no_donor"] += int((m2 & ~m).sum())
        qv[:, :, k + 1] = np.where(m2, qv[:, :, k + 1] + qv[:, :, k] * dp[:, :, k] / dp[:, :, k + 1], qv[:, :, k + 1])
        qv[:, :, k] = np.where(m2, 0.0, qv[:, :, k])
    start = qv[:, :, kb - 1] < 0.0                            # bottom :1274-1284
    found = np.zeros_like(start)
    for k in range(kb - 2, -1, -1):
        m = start & (qv[:, :, kb - 1] < 0.0) & (qv[:, :, k] > 0.0)   # (the early exit: nothing happens once the bottom is >= 0)
        found |= m
        dq = np.minimum(-qv[:, :, kb - 1] * dp[:, :, kb - 1], qv[:, :, k] * dp[:, :, k])
        qv[:, :, k] = np.where(m, qv[:, :, k] - dq / dp[:, :, k], qv[:, :, k])
        qv[:, :, kb - 1] = np.where(m, qv[:, :, kb - 1] + dq / dp[:, :, kb - 1], qv[:, :, kb - 1])
    cnt["qv_bottom_donor"] += int((start & found).sum())
    cnt["qv_bottom_no_donor"] += int((start & ~found).sum())


def fix_qa(qa, dp, cnt):
    """:1289-1321"""
    kb = qa.shape[2]
    for k in range(kb - 1):                                   # :1296-1303
        m = qa[:, :, k] < 0.0
        cnt["qa_interior"] += int(m.sum())
        qa[:, :, k + 1] = np.where(m, qa[:, :, k + 1] + qa[:, :, k] * dp[:, :, k] / dp[:, :, k + 1], qa[:, :, k + 1])
        qa[:, :, k] = np.where(m, 0.0, qa[:, :, k])
    neg = qa[:, :, kb - 1] < 0.0
    m = neg & (qa[:, :, kb - 2] > 0.0)                        # :1311-1315
    cnt["qa_bottom_donor"] += int(m.sum())
    cnt["qa_bottom_no_donor"] += int((neg & ~m).sum())
    dq = np.minimum(-qa[:, :, kb - 1] * dp[:, :, kb - 1], qa[:, :, kb - 2] * dp[:, :, kb - 2])
    qa[:, :, kb - 2] = np.where(m, qa[:, :, kb - 2] - dq / dp[:, :, kb - 2], qa[:, :, kb - 2])
    qa[:, :, kb - 1] = np.where(m, qa[:, :, kb - 1] + dq / dp[:, :, kb - 1], qa[:, :, kb - 1])
    cnt["qa_bottom_clipped"] += int((m & (qa[:, :, kb - 1] < 0.0)).sum())
    qa[:, :, kb - 1] = np.maximum(0.0, qa[:, :, kb - 1])      # :1317


def neg_adj3(bd, hydrostatic, dp, pt, qv, ql, qr, qi, qs, qg, qa=None, consts=None, stop_after_pointwise=False):
    """in place on the compute domain of arrays with halos; returns {branch: count}.  peln and delz are not arguments: they feed p2
    (:1037, :1045), which only the dead saturation block (:1157-1187, sat_adj = .false. at :982) reads."""
    c = {**CONSTS, **(consts or {})}
    cnt = {b: 0 for b in BRANCHES}
    r = (bd.is_, bd.ie, bd.js, bd.je)
    v = lambda a: bd.view(a, "A", *r)
    pointwise(hydrostatic, v(dp), v(pt), v(qv), v(ql), v(qr), v(qi), v(qs), v(qg), cnt, c)
    if stop_after_pointwise:
        return cnt
    fillq(v(qg), v(dp), cnt, "g")
    fillq(v(qr), v(dp), cnt, "r")
    fix_vapor(v(qv), v(dp), cnt)
    if qa is not None:
        fix_qa(v(qa), v(dp), cnt)
    return cnt
