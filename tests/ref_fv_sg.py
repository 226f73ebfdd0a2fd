"""fv_sg_SHiELD (model/fv_sg.F90:76-505) and update_dwinds_phys (model/fv_grid_utils.F90:3291-3475) restated in numpy from the
Fortran, the checkers of fv3_fv_subgrid_z and fv3_update_dwinds_phys at shapes the recorded cases do not have.

Both are held bit for bit to the outputs of the reference's own compiled Fortran (tests/golden/subgrid_sg_*.npz and
tests/golden/subgrid_dwinds.npz, recorded by tests/golden/make_subgrid_golden.py) in tests/test_subgrid_hostemu.py.  Written from the source text, line ranges cited below, with the
reference's order of operations: x**2 as x*x, dim(a, b) as max(a - b, 0), sums left to right.  Vectorised over (i, j) and sequential
in k and in the sweeps where the Fortran is; every `if` of a loop body is a mask.

``fv_sg_shield`` works in place on arrays in the library's layouts (A kind with halos for delp, ta, ua, va, w, u_dt, v_dt and the
tracer array; (nx, ny, km) for pkz, delz; pe (nx+2, km+1, ny+2); peln (nx, km+1, ny)) and returns the counts the tests assert on
before they compare anything.
"""
from __future__ import annotations

import numpy as np

# the constants a SHiELD build hands the routine (constants_mod GFDL values; gfdl_mp.F90:136-137)
CONSTS = dict(rdgas=287.04, rvgas=461.50, grav=9.80, cp_air=287.04 / (2.0 / 7.0), cp_vapor=4.0 * 461.50, c_liq=4.218e3, c_ice=2.106e3)
SPECIES = ("sphum", "liq_wat", "rainwat", "ice_wat", "snowwat", "graupel")
RATIOS = (0.25, 0.5, 0.999)       # :265-268
COUNTS = ("mixed", "not_mixed", "ri_negative", "warm_top", "cold", "mixed_k2", "mixed_k3", "mixed_k4")


def kbot_of(km, k_bot_full, fv_sg_adj_weak):
    return k_bot_full if fv_sg_adj_weak <= 0 else km          # :123-128


def fra_of(km, k_bot_full, fv_sg_adj, fv_sg_adj_weak, dt):
    """:161-169, index k - 1"""
    return [dt / float(fv_sg_adj) if k <= k_bot_full else (dt / float(fv_sg_adj_weak) if fv_sg_adj_weak > 0 else 0.0) for k in range(1, km + 1)]


def _heat_caps(nwat, q, k, sp, c, cv_air, cv_vap):
    """cpm, cvm of level k (:214-249, :408-443); q: list over tracers of lists over levels"""
    cp_air, cp_vapor, c_liq, c_ice = c["cp_air"], c["cp_vapor"], c["c_liq"], c["c_ice"]
    if nwat == 0:
        return cp_air, cv_air
    qv = q[sp["sphum"]][k]
    if nwat in (1, 2):
        return (1.0 - qv) * cp_air + qv * cp_vapor, (1.0 - qv) * cv_air + qv * cv_vap
    if nwat == 3:
        q_liq, q_sol = q[sp["liq_wat"]][k], q[sp["ice_wat"]][k]
        return ((1.0 - (qv + q_liq + q_sol)) * cp_air + qv * cp_vapor + q_liq * c_liq + q_sol * c_ice,
                (1.0 - (qv + q_liq + q_sol)) * cv_air + qv * cv_vap + q_liq * c_liq + q_sol * c_ice)
    if nwat == 4:
        q_liq = q[sp["liq_wat"]][k] + q[sp["rainwat"]][k]
        return ((1.0 - (qv + q_liq)) * cp_air + qv * cp_vapor + q_liq * c_liq,
                (1.0 - (qv + q_liq)) * cv_air + qv * cv_vap + q_liq * c_liq)
    q_liq = q[sp["liq_wat"]][k] + q[sp["rainwat"]][k]
    q_sol = q[sp["ice_wat"]][k] + q[sp["snowwat"]][k] + q[sp["graupel"]][k]
    return ((1.0 - (qv + q_liq + q_sol)) * cp_air + qv * cp_vapor + q_liq * c_liq + q_sol * c_ice,
            (1.0 - (qv + q_liq + q_sol)) * cv_air + qv * cv_vap + q_liq * c_liq + q_sol * c_ice)


def _condensate(nwat, q, k, sp, zero):
    """:278-308, :350-361"""
    if nwat < 2:
        return zero.copy()
    if nwat == 2:
        return q[sp["liq_wat"]][k].copy()
    if nwat == 3:
        return q[sp["liq_wat"]][k] + q[sp["ice_wat"]][k]
    if nwat == 4:
        return q[sp["liq_wat"]][k] + q[sp["rainwat"]][k]
    return q[sp["liq_wat"]][k] + q[sp["ice_wat"]][k] + q[sp["snowwat"]][k] + q[sp["rainwat"]][k] + q[sp["graupel"]][k]


def fv_sg_shield(bd, km, nq, dt, fv_sg_adj, fv_sg_adj_weak, nwat, species, delp, pe, peln, pkz, ta, qa, ua, va, hydrostatic, w, delz,
                 u_dt, v_dt, k_bot_full, ptop, consts=None):
    """species: {name: 1-based index, 0 / missing = absent}.  Returns {count name: [sweep 1, 2, 3]}."""
    c = dict(CONSTS, **(consts or {}))
    rdgas, rvgas, grav, cp_air = c["rdgas"], c["rvgas"], c["grav"], c["cp_air"]
    sp = {n: int((species or {}).get(n, 0)) - 1 for n in SPECIES}
    r = (bd.is_, bd.ie, bd.js, bd.je)
    V = lambda a: bd.view(a, "A", *r)                      # noqa: E731
    ri_max, ri_min, ustar2 = 1.0, 0.25, 1.0e-4             # :57-58, :110
    cv_vap = c["cp_vapor"] - rvgas                         # :45
    cv_air = cp_air - rdgas                                # :114
    rk = cp_air / rdgas + 1.0                              # :115
    g2 = 0.5 * grav
    rdt = 1.0 / dt
    kbot = kbot_of(km, k_bot_full, fv_sg_adj_weak)
    assert 1 <= kbot <= km
    t_min = 160.0 if ptop < 2.0 else 165.0                 # :129-133 (pe(is,1,js) = ptop)
    t_max = 315.0 if k_bot_full < min(km, 24) else 325.0   # :135-139
    xvir, rz = (0.0, 0.0) if nwat == 0 else (rvgas / rdgas - 1.0, rvgas - rdgas)   # :142-147
    fra = fra_of(km, k_bot_full, fv_sg_adj, fv_sg_adj_weak, dt)
    dp = [V(delp)[:, :, k] for k in range(kbot)]
    pl = [peln[:, k, :] for k in range(kbot + 1)]
    pec = [pe[1:-1, k, 1:-1] for k in range(kbot + 1)] if hydrostatic else None
    zero = np.zeros_like(dp[0])
    cnt = {n: [0, 0, 0] for n in COUNTS}
    with np.errstate(all="ignore"):
        # :180-196
        q0 = [[V(qa)[:, :, k, iq].copy() for k in range(kbot)] for iq in range(nq)]
        t0 = [V(ta)[:, :, k].copy() for k in range(kbot)]
        u0 = [V(ua)[:, :, k].copy() for k in range(kbot)]
        v0 = [V(va)[:, :, k].copy() for k in range(kbot)]
        qv = lambda k: q0[sp["sphum"]][k] if nwat != 0 else zero      # noqa: E731  (xvir = rz = 0 multiplies it there)
        pm = [dp[k] / (pl[k + 1] - pl[k]) for k in range(kbot)]
        w0 = [None] * kbot
        hd, te, gz = [None] * kbot, [None] * kbot, [None] * kbot
        gzh = zero.copy()
        if hydrostatic:                                    # :202-211
            for k in range(kbot - 1, -1, -1):
                tvm = t0[k] * (1.0 + xvir * qv(k))
                tv = rdgas * tvm
                gz[k] = gzh + tv * (1.0 - pec[k] / pm[k])
                hd[k] = cp_air * tvm + gz[k] + 0.5 * (u0[k] * u0[k] + v0[k] * v0[k])
                gzh = gzh + tv * (pl[k + 1] - pl[k])
        else:                                              # :213-260
            for k in range(kbot - 1, -1, -1):
                cpm, cvm = _heat_caps(nwat, q0, k, sp, c, cv_air, cv_vap)
                dz = delz[:, :, k]
                w0[k] = V(w)[:, :, k].copy()
                gz[k] = gzh - g2 * dz
                tmp = gz[k] + 0.5 * (u0[k] * u0[k] + v0[k] * v0[k] + w0[k] * w0[k])
                hd[k] = cpm * t0[k] + tmp
                te[k] = cvm * t0[k] + tmp
                gzh = gzh - grav * dz
        for n, ratio in enumerate(RATIOS):                 # :263-453
            gzh = zero.copy()
            qcon = [_condensate(nwat, q0, k, sp, zero) for k in range(kbot)]
            for k in range(kbot - 1, 0, -1):               # 0-based: the pair (k - 1, k); the Fortran's k is k + 1
                k1 = k - 1
                tv1 = t0[k1] * (1.0 + xvir * qv(k1) - qcon[k1])
                tv2 = t0[k] * (1.0 + xvir * qv(k) - qcon[k])
                pt1 = tv1 / pkz[:, :, k1]
                pt2 = tv2 / pkz[:, :, k]
                du, dv = u0[k1] - u0[k], v0[k1] - v0[k]
                ri = (gz[k1] - gz[k]) * (pt1 - pt2) / (0.5 * (pt1 + pt2) * (du * du + dv * dv + ustar2))
                warm = (tv1 > t_max) & (tv1 > tv2)         # :322-327
                cold = ~warm & (tv2 < t_min)
                ri = np.where(warm, 0.0, np.where(cold, np.minimum(ri, 0.1), ri))
                ri_ref = np.minimum(ri_max, ri_min + (ri_max - ri_min) * np.maximum(400.0e2 - pm[k], 0.0) / 200.0e2)   # :332
                if k + 1 == 2:                             # :334-340
                    ri_ref = 4.0 * ri_ref
                elif k + 1 == 3:
                    ri_ref = 2.0 * ri_ref
                elif k + 1 == 4:
                    ri_ref = 1.5 * ri_ref
                mix = ri < ri_ref                          # :342
                cnt["mixed"][n] += int(mix.sum())
                cnt["not_mixed"][n] += int((~mix).sum())
                cnt["ri_negative"][n] += int((ri < 0.0).sum())
                cnt["warm_top"][n] += int(warm.sum())
                cnt["cold"][n] += int(cold.sum())
                if k + 1 in (2, 3, 4):
                    cnt[f"mixed_k{k + 1}"][n] += int(mix.sum())
                x = 1.0 - np.maximum(0.0, ri / ri_ref)
                mc = ratio * dp[k1] * dp[k] / (dp[k1] + dp[k]) * (x * x)          # :343
                W = lambda new, old: np.where(mix, new, old)                      # noqa: E731
                for iq in range(nq):                       # :344-348
                    h0 = mc * (q0[iq][k] - q0[iq][k1])
                    q0[iq][k1] = W(q0[iq][k1] + h0 / dp[k1], q0[iq][k1])
                    q0[iq][k] = W(q0[iq][k] - h0 / dp[k], q0[iq][k])
                qcon[k1] = W(_condensate(nwat, q0, k1, sp, zero), qcon[k1])       # :350-361
                h0 = mc * (u0[k] - u0[k1])                 # :363-369
                u0[k1] = W(u0[k1] + h0 / dp[k1], u0[k1])
                u0[k] = W(u0[k] - h0 / dp[k], u0[k])
                h0 = mc * (v0[k] - v0[k1])
                v0[k1] = W(v0[k1] + h0 / dp[k1], v0[k1])
                v0[k] = W(v0[k] - h0 / dp[k], v0[k])
                h0 = mc * (hd[k] - hd[k1])
                if hydrostatic:                            # :373-375
                    hd[k1] = W(hd[k1] + h0 / dp[k1], hd[k1])
                    hd[k] = W(hd[k] - h0 / dp[k], hd[k])
                else:                                      # :378-384
                    te[k1] = W(te[k1] + h0 / dp[k1], te[k1])
                    te[k] = W(te[k] - h0 / dp[k], te[k])
                    h0 = mc * (w0[k] - w0[k1])
                    w0[k1] = W(w0[k1] + h0 / dp[k1], w0[k1])
                    w0[k] = W(w0[k] - h0 / dp[k], w0[k])
                if hydrostatic:                            # :392-404
                    t = (hd[k] - gzh - 0.5 * (u0[k] * u0[k] + v0[k] * v0[k])) / (rk - pec[k] / pm[k])
                    gzh = gzh + t * (pl[k + 1] - pl[k])
                    t0[k] = t / (rdgas + rz * qv(k))
                    t0[k1] = (hd[k1] - gzh - 0.5 * (u0[k1] * u0[k1] + v0[k1] * v0[k1])) / ((rk - pec[k1] / pm[k1]) * (rdgas + rz * qv(k1)))
                else:                                      # :407-450
                    for kk in (k1, k):
                        cpm, cvm = _heat_caps(nwat, q0, kk, sp, c, cv_air, cv_vap)
                        tv = gz[kk] + 0.5 * (u0[kk] * u0[kk] + v0[kk] * v0[kk] + w0[kk] * w0[kk])
                        t0[kk] = (te[kk] - tv) / cvm
                        hd[kk] = cpm * t0[kk] + tv
        for k in range(kbot):                              # :456-501
            ta_k, ua_k, va_k = V(ta)[:, :, k], V(ua)[:, :, k], V(va)[:, :, k]
            t = ta_k + (t0[k] - ta_k) * fra[k]
            u = ua_k + (u0[k] - ua_k) * fra[k]
            v = va_k + (v0[k] - va_k) * fra[k]
            if not hydrostatic:
                w_k = V(w)[:, :, k]
                w_k[...] = w_k + (w0[k] - w_k) * fra[k]
            for iq in range(nq):
                q_k = V(qa)[:, :, k, iq]
                q_k[...] = q_k + (q0[iq][k] - q_k) * fra[k]
            V(u_dt)[:, :, k] = rdt * (u - ua_k)
            V(v_dt)[:, :, k] = rdt * (v - va_k)
            ta_k[...] = t
            ua_k[...] = u
            va_k[...] = v
    return cnt


def update_dwinds_phys(bd, npx, npy, grid_type, dt, u_dt, v_dt, u, v, geom=None):
    """:3291-3475 in place on u (U x npz), v (V x npz); u_dt, v_dt: A x npz with one ring of halo filled.  geom (grid_type < 3): vlon,
    vlat (A x 3), es1 ((is:ie, js:je+1) x 3), ew2 ((is:ie+1, js:je) x 3), edge_vect_w / _e (jsd:jed), edge_vect_s / _n (isd:ied)."""
    is_, ie, js, je = bd.is_, bd.ie, bd.js, bd.je
    dt5 = 0.5 * dt
    A = lambda a, i0, i1, j0, j1: bd.view(a, "A", i0, i1, j0, j1)     # noqa: E731
    uo = bd.view(u, "U", is_, ie, js, je + 1)
    vo = bd.view(v, "V", is_, ie + 1, js, je)
    if grid_type > 3:                                      # :3338-3349
        uo[...] = uo + dt5 * (A(u_dt, is_, ie, js - 1, je) + A(u_dt, is_, ie, js, je + 1))
        vo[...] = vo + dt5 * (A(v_dt, is_ - 1, ie, js, je) + A(v_dt, is_, ie + 1, js, je))
        return
    g = geom
    im2, jm2 = (npx - 1) // 2, (npy - 1) // 2
    ring = (is_ - 1, ie + 1, js - 1, je + 1)
    ud, vd = A(u_dt, *ring), A(v_dt, *ring)                # (nx+2, ny+2, npz)
    vlon, vlat = A(g["vlon"], *ring), A(g["vlat"], *ring)  # (nx+2, ny+2, 3)
    v3 = [ud * vlon[:, :, m, None] + vd * vlat[:, :, m, None] for m in range(3)]     # :3353-3359
    ue = [x[:, :-1] + x[:, 1:] for x in v3]                # (is-1:ie+1, js:je+1)    :3362-3368
    ve = [x[:-1, :] + x[1:, :] for x in v3]                # (is:ie+1, js-1:je+1)    :3370-3376
    nx, ny = bd.nx, bd.ny
    ii = np.arange(is_, ie + 1)
    jj = np.arange(js, je + 1)
    ng_i, ng_j = is_ - bd.isd, js - bd.jsd
    for cond, i, name in ((is_ == 1, 1, "edge_vect_w"), (ie + 1 == npx, npx, "edge_vect_e")):   # :3379-3416
        if not cond:
            continue
        ev = np.asarray(g[name])[jj - js + ng_j][:, None]
        col = i - is_
        nb = np.where(jj > jm2, jj - 1, jj + 1) - (js - 1)  # index into ve's j axis (js-1 -> 0)
        me = jj - (js - 1)
        for m in range(3):
            vt = ev * ve[m][col, nb] + (1.0 - ev) * ve[m][col, me]
            ve[m][col, me] = vt
    for cond, j, name in ((js == 1, 1, "edge_vect_s"), (je + 1 == npy, npy, "edge_vect_n")):    # :3418-3455
        if not cond:
            continue
        ev = np.asarray(g[name])[ii - is_ + ng_i][:, None]
        row = j - js
        nb = np.where(ii > im2, ii - 1, ii + 1) - (is_ - 1)
        me = ii - (is_ - 1)
        for m in range(3):
            ut = ev * ue[m][nb, row] + (1.0 - ev) * ue[m][me, row]
            ue[m][me, row] = ut
    es1, ew2 = g["es1"], g["ew2"]
    uei = [x[1:-1] for x in ue]                            # i = is:ie
    vej = [x[:, 1:-1] for x in ve]                         # j = js:je
    uo[...] = uo + dt5 * (uei[0] * es1[:, :, 0, None] + uei[1] * es1[:, :, 1, None] + uei[2] * es1[:, :, 2, None])   # :3456-3462
    vo[...] = vo + dt5 * (vej[0] * ew2[:, :, 0, None] + vej[1] * ew2[:, :, 1, None] + vej[2] * ew2[:, :, 2, None])   # :3463-3469
