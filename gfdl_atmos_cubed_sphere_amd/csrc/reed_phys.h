// reed_phys.h -- the Reed-Jablonowski simple physics and the terminator chemistry of the solo driver: the column loop of the
// do_reed_sim_phys branch (driver/solo/fv_phys.F90:551-602) with reed_sim_physics (:2332-2817) inside it, and
// DCMIP2016_terminator_advance (:2819-2894).  Their tendencies go to fv_update_phys (:675-687; phys_update.h here).
//
// ReedSimPhys: one thread per (i, j) column, lanes along i, one launch.  The routine is large-scale condensation (:2608-2632), implicit
// surface fluxes at the bottom level (:2717-2733) and an implicit boundary-layer diffusion of u, v, theta, q (:2743-2815), a
// tridiagonal solve.  Three walks of the column:
//   1. the bottom level alone: za from the entry T and q (:2562-2563), the condensation there, wind, Cd, the surface diffusivities
//      and the four scalars of the surface fluxes (the two denominators, the two numerator terms), which stay in registers;
//   2. UP (k = npz .. 1, :2769-2781): level k forms CC(k), CCm(k) and CA(k-1), CAm(k-1) from the interface above it -- the
//      condensation of level k-1 is run there for t(k-1), which rho reads --, then CE, CEm, CFu, CFv, CFt, CFq of level k, which go to
//      the six work planes wk[0..5] (each (is:ie, js:je, npz), lanes coalesced).  Km, Ke, CA*, CC* and the coefficients of level k+1
//      stay in registers.  The reference's level pver+1 of CE .. CFq is zero (:2756-2767): the registers start as zero and the work
//      planes hold npz levels, not npz+1;
//   3. DOWN (k = 1 .. npz, :2788-2815): the condensation of level k again (the same operations on the same inputs: the same bits),
//      the rain sum in the reference's order (:2616), the surface fluxes at the bottom level, the six coefficients read back, the
//      new u, v, t, q of level k-1 carried in registers, and the four tendencies written.
// reed_cond_only (:2635) ends after the condensation: walk 3 alone, without the solve.  reed_test = 2 (:2506): the reference
// returns with its intent(out) tendencies undefined; here the tendencies keep their bits (fresh: zeros are written) and rain is
// rain2 * 8.64e7 = 0 with COND.
//
// Every expression in the reference's order of floating-point operations (left to right, its parentheses, no contraction).  Where
// the reference evaluates one expression several times on the same operands -- the denominators 1+CA+CC-CA*CE of :2770-2779, the
// exp of :2699-2700, (p0/pmid(k-1))**(rair/cpair) of :2807 and :2810 and of :2776 a level earlier, the right-hand sides of the
// tendency and of the state update -- it is formed once: the same operations on the same operands give the same bits.  log, exp
// are include/fv3_math.h, x**y with a real y is fv3_exp(y * fv3_log(x)), x**2 is x*x, sqrt is the hardware's.
//
// COND, ALT, HYD: do_reed_cond, reed_alt_mxg, hydrostatic (HYD is read only with ALT: zint, :567-580, feeds nothing else).
//
// The wrapper's arithmetic (:555-561, :565-580): q2 = max(0, q); pm = dp / (peln(k+1) - peln(k)); rdelp = 1 / dp; zint upwards
// from phis * rgrav (:565 writes zint(i, k) with the k the loop above leaves, npz+1), hydrostatic with the UNCLAMPED q (:570),
// else minus delz.
//
// tab: two planes on the compute domain formed on the host (fv3_grid_upload_reed): [0] Tsurf (:2573-2577 for test 1, SST_tc for
// test 0), [1] exp((dc_vap*log(Tsurf/tice) + Lv0*(Tsurf-tice)/(Tsurf*tice))/rvgas) of :2719.  No sin, cos or pow of the latitude runs
// on the device.
//
// fresh: the incoming u_dt, v_dt, t_dt, q_dt are taken as zero and not read; every cell of the four on the compute domain is
// written; 0 + x is formed, so the sign of a zero is that of zero-then-call.
//
// TerminatorAdvance: pointwise over the WHOLE A layout x km, halo included (the reference loops ifirst:ilast, jfirst:jlast), on the two
// tracer planes Cl and Cl2; k1 is a plane over the A layout formed on the host (fv3_grid_upload_terminator).
#pragma once

#include "fv3_common.h"

namespace fv3 {

struct ReedScalars {          // formed in the entry point, each a sub-expression the reference's own expressions begin with
  double pdt, rdt;            // dtime, 1./dtime
  double gravit, rair, cpair; // GRAV, RDGAS, CP_AIR (:2516-2518)
  double kap;                 // rair/cpair
  double zvir;                // (rh2o/rair) - 1 with rh2o = 461.5 (:2526)
  double ee0, elv;            // epsilo*e0, epsilo*latvap
  double lvcp, lvrv, rT0;     // latvap/cpair, latvap/rh2o, 1./T0
  double grw, rog;            // gravit*rhow, rair/gravit
  double c04sqC;              // 0.4*sqC
  double rgrav, rdrg, zvir_w; // the wrapper's: 1./grav, rdgas*rgrav, rvgas/rdgas - 1. (:548-549, :570)
};

FV3_HD double reed_pow(double x, double y) { return fv3_exp(y * fv3_log(x)); }

template <bool COND, bool ALT, bool HYD>
struct ReedSimPhys {
  Grid g;
  int fresh, test, cond_only;
  ReedScalars s;
  const double *tab;                                     // 2 x (is:ie, js:je)
  const double *delp, *pt, *ua, *va, *q, *pe, *peln, *phis, *delz;
  double *u_dt, *v_dt, *t_dt, *q_dt, *rain;
  double *wk;                                            // 6 x (is:ie, js:je, npz): CE, CEm, CFu, CFv, CFt, CFq
  static constexpr int CH = 256;                         // columns per workgroup: one per thread

  // one level as the wrapper hands it over and the condensation leaves it (:555-561, :2609-2630).  peln_hi, peln_lo: peln(k+1), peln(k)
  FV3_HD void level(size_t o, double peln_hi, double peln_lo, double &dp, double &pm, double &t, double &qv, double &dtc, double &dqc,
                    double &tmp, bool &sat) const {
    dp = delp[o];
    t = pt[o];
    qv = dmax(0., q[o]);
    pm = dp / (peln_hi - peln_lo);
    dtc = 0.;
    dqc = 0.;
    tmp = 0.;
    sat = false;
    if (COND) {
      const double qsat = s.ee0 / pm * fv3_exp(-(s.lvrv * ((1. / t) - s.rT0)));
      if (qv > qsat) {
        sat = true;
        tmp = s.rdt * (qv - qsat) / (1. + s.lvcp * (s.elv * qsat / (s.rair * (t * t))));
        dtc = 0. + s.lvcp * tmp;
        dqc = 0. - tmp;
      }
      t = t + dtc * s.pdt;
      qv = qv + dqc * s.pdt;
    }
  }

  FV3_HD void operator()(int bx, int, int, int tid, double *) const {
    const double C = 0.0011, Cd0 = 0.0007, Cd1 = 0.000065, Cm = 0.002, v20 = 20.0, p0 = 100000.0;   // :2533-2545
    const double pbltop = 85000., pbltopz = 1000., pblconst = 10000.;
    const size_t n3 = g.nA(), nc = g.nCC();
    const int ncol = g.nx * g.ny, npz = g.npz, np1 = g.npz + 1;
    const size_t spl = (size_t)g.nx, spe = (size_t)g.nx + 2;   // level strides of peln and pe
    const size_t nw = nc * (size_t)npz;
    const double pdt = s.pdt, gravit = s.gravit;
    for (int idx = bx * CH + tid; idx < (bx + 1) * CH && idx < ncol; idx += kNT) {
      const int i = g.is + idx % g.nx, j = g.js + idx / g.nx;
      const size_t a = (size_t)g.iA(i, j), cc = (size_t)g.iCC(i, j);
      // peln(i, k, j) on (is:ie, npz+1, js:je); pe(i, k, j) on (is-1:ie+1, npz+1, js-1:je+1)
      const double *plc = peln + (size_t)(j - g.js) * np1 * g.nx + (i - g.is);
      const double *pec = pe + (size_t)(j - g.js + 1) * np1 * (g.nx + 2) + (i - g.is + 1);
      if (test == 2) {   // :2506
        if (fresh)
          for (int k = 0; k < npz; k++) {
            u_dt[a + (size_t)k * n3] = 0.;
            v_dt[a + (size_t)k * n3] = 0.;
            t_dt[cc + (size_t)k * nc] = 0.;
            q_dt[cc + (size_t)k * nc] = 0.;
          }
        if (COND) rain[cc] = 0. * 8.64e7;   // :582, :599
        continue;
      }
      double *wCE = wk + cc, *wCEm = wCE + nw, *wCFu = wCEm + nw, *wCFv = wCFu + nw, *wCFt = wCFv + nw, *wCFq = wCFt + nw;
      double den_m = 1., den_e = 1., a_t = 0., a_q = 0.;   // the surface fluxes' scalars (:2720-2732)
      double dp, pm, t, qv, dtc, dqc, tmp;
      bool sat;
      if (!cond_only) {
        // ---- 1. the bottom level
        const int kb = npz - 1;
        const size_t ob = a + (size_t)kb * n3;
        const double ps = pec[(size_t)npz * spe];
        const double dlnpint = fv3_log(ps) - fv3_log(pec[(size_t)kb * spe]);                    // :2562
        const double za = s.rog * pt[ob] * (1. + s.zvir * dmax(0., q[ob])) * 0.5 * dlnpint;    // :2563
        double peln_lo = plc[(size_t)kb * spl];
        level(ob, plc[(size_t)npz * spl], peln_lo, dp, pm, t, qv, dtc, dqc, tmp, sat);
        double rp = 1. / dp;
        double u = ua[ob], v = va[ob];
        const double wind = sqrt(u * u + v * v);                                               // :2655
        const double Cd = wind < v20 ? Cd0 + Cd1 * wind : Cm;                                  // :2661-2665, :2684-2690
        const double Ke_s = C * wind * za, Km_s = Cd * wind * za;                              // Ke(pver+1), Km(pver+1) (:2683-2689)
        const double sqCd04 = 0.4 * sqrt(Cd);
        const double qsats = s.ee0 / ps * tab[nc + cc];                                        // :2719
        den_m = 1. + Cd * wind * pdt / za;
        den_e = 1. + C * wind * pdt / za;
        a_t = C * wind * tab[cc] * pdt / za;
        a_q = C * wind * qsats * pdt / za;
        u = u / den_m;
        v = v / den_m;
        t = (t + a_t) / den_e;
        qv = (qv + a_q) / den_e;
        // ---- 2. the sweep up
        double CE1 = 0., CEm1 = 0., CFu1 = 0., CFv1 = 0., CFt1 = 0., CFq1 = 0.;   // level k+1 (:2759-2766)
        double CA = 0., CAm = 0.;                                                   // CA(k), CAm(k) (:2757, :2760)
        double zi = ALT ? phis[a] * s.rgrav : 0.;                                   // zint(k+1) (:565)
        for (int k = npz - 1; k >= 0; k--) {
          const size_t o = a + (size_t)k * n3, oc = cc + (size_t)k * nc;
          if (k < npz - 1) {
            u = ua[o];
            v = va[o];
          }
          double CC = 0., CCm = 0., CAu = 0., CAmu = 0.;   // CC(k), CCm(k) (:2758, :2761), CA(k-1), CAm(k-1)
          double dp_u = 0., pm_u = 0., t_u = 0., q_u = 0., peln_u = 0.;
          if (k > 0) {
            peln_u = plc[(size_t)(k - 1) * spl];
            level(o - n3, peln_lo, peln_u, dp_u, pm_u, t_u, q_u, dtc, dqc, tmp, sat);
            const double pint = pec[(size_t)k * spe];
            double Km, Ke;
            if (ALT) {   // :2668-2678 with zint of :567-580
              if (HYD) zi = zi + s.rdrg * pt[o] * (1. + s.zvir_w * q[o]) * (plc[(size_t)(k + 1) * spl] - peln_lo);
              else zi = zi - delz[oc];
              if (zi > pbltopz) {
                Km = 0.;
                Ke = 0.;
              } else {
                const double f = 1. - zi / pbltopz;
                Km = sqCd04 * wind * zi * (f * f);
                Ke = s.c04sqC * wind * zi * (f * f);
              }
            } else if (pint >= pbltop) {   // :2695-2701
              Km = Km_s;
              Ke = Ke_s;
            } else {
              const double d = pbltop - pint;
              const double e = fv3_exp(-((d * d) / (pblconst * pblconst)));
              Km = Km_s * e;
              Ke = Ke_s * e;
            }
            const double rho = pint / (s.rair * (t + t_u) / 2.0);   // :2745-2753
            const double dpm = pm - pm_u;
            const double rp_u = 1. / dp_u;
            CAmu = rp_u * pdt * gravit * gravit * Km * rho * rho / dpm;
            CCm = rp * pdt * gravit * gravit * Km * rho * rho / dpm;
            CAu = rp_u * pdt * gravit * gravit * Ke * rho * rho / dpm;
            CC = rp * pdt * gravit * gravit * Ke * rho * rho / dpm;
            rp = rp_u;
          }
          const double den = 1. + CA + CC - CA * CE1, denm = 1. + CAm + CCm - CAm * CEm1;   // :2770-2779
          CE1 = CC / den;
          CEm1 = CCm / denm;
          CFu1 = (u + CAm * CFu1) / denm;
          CFv1 = (v + CAm * CFv1) / denm;
          CFt1 = (reed_pow(p0 / pm, s.kap) * t + CA * CFt1) / den;
          CFq1 = (qv + CA * CFq1) / den;
          wCE[(size_t)k * nc] = CE1;
          wCEm[(size_t)k * nc] = CEm1;
          wCFu[(size_t)k * nc] = CFu1;
          wCFv[(size_t)k * nc] = CFv1;
          wCFt[(size_t)k * nc] = CFt1;
          wCFq[(size_t)k * nc] = CFq1;
          CA = CAu;
          CAm = CAmu;
          pm = pm_u;
          t = t_u;
          qv = q_u;
          peln_lo = peln_u;
        }
      }
      // ---- 3. the sweep down: the tendencies
      double prec = 0.;                                   // rain2 (:582)
      double up = 0., vp = 0., tp = 0., qp = 0., pwi = 0.;   // u, v, t, q of level k-1 after the solve, (p0/pmid(k-1))**(rair/cpair)
      double peln_k = plc[0];
      for (int k = 0; k < npz; k++) {
        const size_t o = a + (size_t)k * n3, oc = cc + (size_t)k * nc;
        const double peln_k1 = plc[(size_t)(k + 1) * spl];
        level(o, peln_k1, peln_k, dp, pm, t, qv, dtc, dqc, tmp, sat);
        peln_k = peln_k1;
        if (COND && sat) prec = prec + tmp * dp / s.grw;   // :2616
        double du = 0., dv = 0.;
        if (!cond_only) {
          double u = ua[o], v = va[o];
          if (k == npz - 1) {   // :2720-2732
            du = du + (u / den_m - u) / pdt;
            dv = dv + (v / den_m - v) / pdt;
            u = u / den_m;
            v = v / den_m;
            dtc = dtc + ((t + a_t) / den_e - t) / pdt;
            t = (t + a_t) / den_e;
            dqc = dqc + ((qv + a_q) / den_e - qv) / pdt;
            qv = (qv + a_q) / den_e;
          }
          const double pw = reed_pow(pm / p0, s.kap);
          const double CFu = wCFu[(size_t)k * nc], CFv = wCFv[(size_t)k * nc], CFt = wCFt[(size_t)k * nc], CFq = wCFq[(size_t)k * nc];
          double un, vn, tn, qn;
          if (k == 0) {   // :2789-2796
            un = CFu;
            vn = CFv;
            tn = CFt * pw;
            qn = CFq;
          } else {   // :2803-2813
            const double CE = wCE[(size_t)k * nc], CEm = wCEm[(size_t)k * nc];
            un = CEm * up + CFu;
            vn = CEm * vp + CFv;
            tn = (CE * tp * pwi + CFt) * pw;
            qn = CE * qp + CFq;
          }
          du = du + (un - u) / pdt;
          dv = dv + (vn - v) / pdt;
          dtc = dtc + (tn - t) / pdt;
          dqc = dqc + (qn - qv) / pdt;
          up = un;
          vp = vn;
          tp = tn;
          qp = qn;
          if (k < npz - 1) pwi = reed_pow(p0 / pm, s.kap);
        }
        u_dt[o] = (fresh ? 0. : u_dt[o]) + du;   // :591-594
        v_dt[o] = (fresh ? 0. : v_dt[o]) + dv;
        t_dt[oc] = (fresh ? 0. : t_dt[oc]) + dtc;
        q_dt[oc] = (fresh ? 0. : q_dt[oc]) + dqc;
      }
      if (COND) rain[cc] = prec * 8.64e7;   // :599
    }
  }
};

struct TerminatorAdvance {
  size_t n;                  // cells of the A layout x km
  size_t n2;                 // cells of the A layout: the period of k1
  int fill;                  // term_fill_negative
  double pdt, rdt;
  const double *k1p;         // A
  double *cl, *cl2;          // A x km each
  static constexpr int CH = 4096;

  FV3_HD void operator()(int bx, int, int, int tid, double *) const {
    const double k2 = 1.;
    for (size_t idx = (size_t)bx * CH + tid; idx < (size_t)(bx + 1) * CH && idx < n; idx += kNT) {
      double qCl = cl[idx], qCl2 = cl2[idx];
      if (fill) {   // :2857-2859
        const double dq = dmin(qCl2, 0.) * 2. - dmin(qCl, 0.);
        qCl = qCl + dq;
        qCl2 = qCl2 - dq * 0.5;
      }
      const double r = k1p[idx % n2] / k2 * 0.25;   // :2874-2888
      const double qcly = qCl + 2. * qCl2;
      const double D = sqrt(r * r + 2. * r * qcly);
      const double expdt = fv3_exp(-4. * k2 * D * pdt);
      double el;
      if (fabs(D * k2 * pdt) > 1e-16) el = (1. - expdt) / D * rdt;
      else el = 4. * k2;
      const double cl_f = -el * (qCl - D + r) * (qCl + D + r) / (1. + expdt + pdt * el * (qCl + r));
      cl[idx] = qCl + cl_f * pdt;
      cl2[idx] = qCl2 - cl_f * 0.5 * pdt;
    }
  }
};

}  // namespace fv3
