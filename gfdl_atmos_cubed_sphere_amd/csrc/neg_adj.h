// neg_adj.h -- neg_adj3 (model/fv_sg.F90:968-1335) and its fillq (:1337-1370): the repair of negative water species that
// fv_dynamics runs after the k_split loop whenever nwat == 6 (model/fv_dynamics.F90:722-745).
//
// One thread per (i, j) column, lanes along i, one launch.  The reference makes five passes over the fields (the pointwise repair level
// by level, fillq of qg, fillq of qr, the vapor fix, the qa fix); here the first pass does the pointwise repair AND gathers what decides
// whether a column pass has anything to do (a negative value left in qg / qr / qv / qa, and fillq's sum1 in the reference's own order of
// summation), so a column without negative water costs one read of its inputs and no store.  A value is stored only where it differs
// from what was read: a cell the reference leaves unchanged keeps its bits.  The column passes of the flagged columns go through
// memory again (the thread reads back its own stores, which the hardware keeps in program order).
//
// What is NOT built, because the reference does not run it:
//  - sat_adj is a local constant .false. (:982): the saturation adjustment (:1157-1187) is dead code.
//  - p2 (:1037, :1045) feeds that block only, so peln and delz are never read; the entry point still insists on the one that the
//    caller's mode needs, so that a call that would be wrong with sat_adj on is refused today.
//  - ENG_CNV_OLD: the form without it (:66, :1012).
#pragma once

#include "fv3_common.h"

namespace fv3 {

struct NegAdj3 {
  Grid g;
  int kbot, hydrostatic;
  double rdgas, rvgas, cp_air, cp_vapor, hlv, hlf, c_liq, c_ice;
  const double *delp;
  double *pt, *qv, *ql, *qr, *qi, *qs, *qg, *qa;   // qa may be null
  static constexpr int CH = 256;   // columns per workgroup: one per thread

  // fillq (:1337-1370) of one column whose sum1 (:1345-1350) the caller has; called only where a negative value is left
  FV3_HD void fillq(double *q, const double *dp, size_t a, size_t n3, double sum1) const {
    if (sum1 < 1.E-12) return;   // :1351
    double sum2 = 0.;
    for (int k = kbot - 1; k >= 0; k--) {   // :1353-1360
      const size_t o = a + (size_t)k * n3;
      const double v = q[o];
      if (v < 0.0 && sum1 > 0.) {
        const double d = dp[o], dq = dmin(sum1, -v * d);
        sum1 = sum1 - dq;
        sum2 = sum2 + dq;
        q[o] = v + dq / d;
      }
    }
    for (int k = kbot - 1; k >= 0; k--) {   // :1361-1367
      const size_t o = a + (size_t)k * n3;
      const double v = q[o];
      if (v > 0.0 && sum2 > 0.) {
        const double d = dp[o], dq = dmin(sum2, v * d);
        sum2 = sum2 - dq;
        q[o] = v - dq / d;
      }
    }
  }

  FV3_HD void operator()(int bx, int, int, int tid, double *) const {
    // module parameters of fv_sg.F90:43-70 and the mode's d0_vap, lv00 (:1004-1014), as written there
    const double t_ice = 273.16, hlv0 = 2.5e6, hlf0 = 3.3358e5;
    const double cv_vap = cp_vapor - rvgas, dc_ice = c_liq - c_ice;
    const double Li0 = hlf0 - dc_ice * t_ice;
    const double cv_air = cp_air - rdgas;   // :990
    const double d0_vap = hydrostatic ? cp_vapor - c_liq : cv_vap - c_liq;
    const double lv00 = hydrostatic ? hlv0 - d0_vap * t_ice : hlv0 - d0_vap * t_ice - rvgas * t_ice;
    const size_t n3 = g.nA();
    const int ncol = g.nx * g.ny;
    for (int idx = bx * CH + tid; idx < (bx + 1) * CH && idx < ncol; idx += kNT) {
      const size_t a = (size_t)g.iA(g.is + idx % g.nx, g.js + idx / g.nx);
      bool neg_g = false, neg_r = false, neg_v = false, neg_a = false;
      double sum_g = 0., sum_r = 0.;
      // ---- :1020-1204, level by level; what the column passes need is gathered on the way
      for (int k = 0; k < kbot; k++) {
        const size_t o = a + (size_t)k * n3;
        const double qv0 = qv[o], ql0 = ql[o], qi0 = qi[o], qs0 = qs[o], qr0 = qr[o], qg0 = qg[o], pt0 = pt[o], dp2 = delp[o];
        double qv2 = qv0, ql2 = ql0, qi2 = qi0, qs2 = qs0, qr2 = qr0, qg2 = qg0, pt2 = pt0;
        if (qa) neg_a = neg_a || qa[o] < 0.;
        // a cell whose ice pair and liquid pair are positive sums of non-negative parts and whose graupel is not negative takes
        // none of the branches below
        const bool clean = qi0 + qs0 > 0. && qi0 >= 0. && qs0 >= 0. && qg0 >= 0. && ql0 + qr0 > 0. && ql0 >= 0. && qr0 >= 0.;
        if (!clean) {
          double lcpk, icpk;
          if (hydrostatic) {   // :1038-1039
            lcpk = hlv / cp_air;
            icpk = hlf / cp_air;
          } else {             // :1046-1050
            const double q_liq = dmax(0., ql2 + qr2), q_sol = dmax(0., qi2 + qs2);
            const double cpm = (1. - (qv2 + q_liq + q_sol)) * cv_air + qv2 * cv_vap + q_liq * c_liq + q_sol * c_ice;
            lcpk = (lv00 + d0_vap * pt2) / cpm;
            icpk = (Li0 + dc_ice * pt2) / cpm;
          }
          // ice phase (:1061-1075)
          double qsum = qi2 + qs2;
          if (qsum > 0.) {
            if (qi2 < 0.) {
              qi2 = 0.;
              qs2 = qsum;
            } else if (qs2 < 0.) {
              qs2 = 0.;
              qi2 = qsum;
            }
          } else {   // borrow from graupel
            qi2 = 0.;
            qs2 = 0.;
            qg2 = qg2 + qsum;
          }
          // graupel < 0: from snow, then ice (:1079-1089)
          if (qg2 < 0.) {
            double dq = dmin(qs2, -qg2);
            qs2 = qs2 - dq;
            qg2 = qg2 + dq;
            if (qg2 < 0.) {
              dq = dmin(qi2, -qg2);
              qi2 = qi2 - dq;
              qg2 = qg2 + dq;
            }
          }
          if (qg2 < 0. && qr2 > 0.) {   // from rain: phase change (:1092-1097)
            const double dq = dmin(qr2, -qg2);
            qg2 = qg2 + dq;
            qr2 = qr2 - dq;
            pt2 = pt2 + dq * icpk;
          }
          if (qg2 < 0. && ql2 > 0.) {   // from cloud water (:1099-1104)
            const double dq = dmin(ql2, -qg2);
            qg2 = qg2 + dq;
            ql2 = ql2 - dq;
            pt2 = pt2 + dq * icpk;
          }
          if (qg2 < 0. && qv2 > 0.) {   // last resort: vapor (:1106-1111)
            const double dq = dmin(0.999 * qv2, -qg2);
            qg2 = qg2 + dq;
            qv2 = qv2 - dq;
            pt2 = pt2 + dq * (icpk + lcpk);
          }
          // liquid phase (:1116-1149)
          qsum = ql2 + qr2;
          if (qsum > 0.) {
            if (qr2 < 0.) {
              qr2 = 0.;
              ql2 = qsum;
            } else if (ql2 < 0.) {
              ql2 = 0.;
              qr2 = qsum;
            }
          } else {
            ql2 = 0.;
            qr2 = qsum;   // rain water is still negative
            double dq = dmin(dmax(0.0, qg2), -qr2);   // fill negative rain with qg first
            qr2 = qr2 + dq;
            qg2 = qg2 - dq;
            pt2 = pt2 - dq * icpk;
            if (qr0 < 0.) {   // :1133 tests qr(i,j,k), the value the level came in with, not qr2
              dq = dmin(qi2 + qs2, -qr2);
              qr2 = qr2 + dq;
              const double dq1 = dmin(dq, qs2);
              qs2 = qs2 - dq1;
              qi2 = qi2 + dq1 - dq;
              pt2 = pt2 - dq * icpk;
            }
            if (qr2 < 0. && qv2 > 0.) {   // :1143-1148
              dq = dmin(0.999 * qv2, -qr2);
              qv2 = qv2 - dq;
              qr2 = qr2 + dq;
              pt2 = pt2 + dq * lcpk;
            }
          }
          // :1192-1202, only where the value moved
          if (qv2 != qv0) qv[o] = qv2;
          if (ql2 != ql0) ql[o] = ql2;
          if (qi2 != qi0) qi[o] = qi2;
          if (qs2 != qs0) qs[o] = qs2;
          if (qr2 != qr0) qr[o] = qr2;
          if (qg2 != qg0) qg[o] = qg2;
          if (pt2 != pt0) pt[o] = pt2;
        }
        // fillq's sum1 (:1345-1350) of qg and of qr, in its order; the flags of the column passes
        if (qg2 > 0.) sum_g = sum_g + qg2 * dp2;
        if (qr2 > 0.) sum_r = sum_r + qr2 * dp2;
        neg_g = neg_g || qg2 < 0.;
        neg_r = neg_r || qr2 < 0.;
        neg_v = neg_v || qv2 < 0.;
      }
      // ---- :1208-1234: without a negative value both sweeps of fillq do nothing
      if (neg_g) fillq(qg, delp, a, n3, sum_g);
      if (neg_r) fillq(qr, delp, a, n3, sum_r);
      // ---- :1239-1286: every branch of the vapor fix starts from a negative qv
      if (neg_v) {
        double up = qv[a], cur = qv[a + n3];
        double dpm = delp[a], dpk = delp[a + n3];
        if (up < 0.) {   // top layer: borrow from below (:1244-1247)
          cur = cur + up * dpm / dpk;
          up = 0.;
        }
        for (int k = 1; k < kbot - 1; k++) {   // :1255-1267, a recursion on k / k-1
          const size_t o = a + (size_t)k * n3;
          double nxt = qv[o + n3];
          const double dpp = delp[o + n3];
          if (cur < 0. && up > 0.) {
            const double dq = dmin(-cur * dpk, up * dpm);
            up = up - dq / dpm;
            cur = cur + dq / dpk;
          }
          if (cur < 0.) {
            nxt = nxt + cur * dpk / dpp;
            cur = 0.;
          }
          qv[o - n3] = up;
          up = cur; cur = nxt;
          dpm = dpk; dpk = dpp;
        }
        const size_t ob = a + (size_t)(kbot - 1) * n3;
        qv[ob - n3] = up;
        if (cur < 0.) {   // bottom layer: borrow from above, nearest donor first, until paid (:1274-1284)
          for (int k = kbot - 2; k >= 0; k--) {
            if (cur >= 0.) break;
            const size_t o = a + (size_t)k * n3;
            const double v = qv[o];
            if (v > 0.) {
              const double d = delp[o], dq = dmin(-cur * dpk, v * d);
              qv[o] = v - dq / d;
              cur = cur + dq / dpk;
            }
          }
        }
        qv[ob] = cur;
      }
      // ---- :1289-1321: the downward recursion acts only below a negative qa; the bottom layer ends with max(0, qa)
      if (neg_a) {
        double cur = qa[a], dpk = delp[a], up = 0., dpm = 1.;
        for (int k = 0; k < kbot - 1; k++) {   // :1296-1303
          const size_t o = a + (size_t)k * n3;
          double nxt = qa[o + n3];
          const double dpp = delp[o + n3];
          if (cur < 0.) {
            nxt = nxt + cur * dpk / dpp;
            cur = 0.;
          }
          qa[o] = cur;
          up = cur; cur = nxt;
          dpm = dpk; dpk = dpp;
        }
        const size_t ob = a + (size_t)(kbot - 1) * n3;
        if (cur < 0. && up > 0.) {   // :1311-1315
          const double dq = dmin(-cur * dpk, up * dpm);
          qa[ob - n3] = up - dq / dpm;
          cur = cur + dq / dpk;
        }
        qa[ob] = dmax(0., cur);   // :1317
      }
    }
  }
};

}  // namespace fv3
