// held_suarez.h -- Held_Suarez_Tend and age_of_air (driver/solo/hswf.F90:41-207, :209-245), the idealised forcing the solo driver's
// do_Held_Suarez branch runs (driver/solo/fv_phys.F90:620-627) before fv_update_phys (:675-687; phys_update.h here).
//
// HeldSuarezTend: one thread per (i, j) column, lanes along i, one launch, one walk UP the column (k = npz .. 1, hswf.F90:147): the
// stratosphere and mesosphere branches read pl(k+1) and teq(k+1) of the level below, which the walk carries in two registers; the
// reference's pl(is:ie, npz), teq(is:ie, npz), u1, v1 are not stored.  pl(k) = delp / (peln(k+1) - peln(k)) is formed where it is
// read, peln(k) is carried to the level above as its peln(k+1).  The three branches of :149-197 in the reference's order of
// floating-point operations (left to right, its parentheses, no contraction); log and exp are include/fv3_math.h.  The bottom friction
// (:187-196) belongs to the troposphere branch only, as in the reference.
//
// STRAT, ZUR: the reference's strat and zurita, one instantiation each, so the standard form carries no branch on either.
//
// The latitude never meets a sin, cos or pow on the device: lat holds five planes on the compute domain, formed once on the host
// (fv3_grid_upload_lat) in the reference's own expressions: [0] agrid(i,j,2); [1] COS(agrid); [2] ty*SIN(agrid)*SIN(agrid);
// [3] tz*(ap0k/akap)*COS(agrid)*COS(agrid); [4] COS(agrid)**4.0.  An instantiation loads the planes its branches read.
//
// Loads: ua, va, u_dt, v_dt only where the friction acts (sigl > 0); pkz only in the standard troposphere branch; t_dt, u_dt, v_dt
// not at all with fresh, which takes them as zero and writes every cell of the three on the compute domain -- 0 + x and 0 - x are
// formed, so the sign of a zero is that of zero-then-call.  Stores: t_dt every cell; u_dt, v_dt where the friction acts (fresh: all).
//
// Not defined, as in the reference: a column whose bottom layer has pl <= 100e2 with strat (the reference reads pl(npz+1)).
//
// AgeOfAir: the age tracer q (A x km) zeroed when time < 1e-6, else set to ascale * time where pe(i, k, j) >= 75000.
#pragma once

#include "fv3_common.h"

namespace fv3 {

template <bool STRAT, bool ZUR>
struct HeldSuarezTend {
  Grid g;
  int fresh;
  double pdt, sday, rdt, rkv, rka, drk, rms, rmr, tau, t_ms, rsgb, ap0k, algpk, rd_zur_rad;   // hswf.F90:101-133; drk = rks - rka
  const double *lat;                         // 5 x (is:ie, js:je)
  const double *delp, *peln, *pe, *pkz, *pt, *ua, *va;
  double *u_dt, *v_dt, *t_dt;
  static constexpr int CH = 256;             // columns per workgroup: one per thread

  FV3_HD void operator()(int bx, int, int, int tid, double *) const {
    const double t0 = 200., h0 = 7., sigb = 0.7, akap = 2. / 7.;   // :101-108, :128
    const double rakap = 1. / akap;
    const size_t n3 = g.nA(), nc = g.nCC();
    const int ncol = g.nx * g.ny, npz = g.npz, np1 = g.npz + 1;
    const size_t spl = (size_t)g.nx, spe = (size_t)g.nx + 2;   // level strides of peln and pe
    for (int idx = bx * CH + tid; idx < (bx + 1) * CH && idx < ncol; idx += kNT) {
      const int i = g.is + idx % g.nx, j = g.js + idx / g.nx;
      const size_t a = (size_t)g.iA(i, j), cc = (size_t)g.iCC(i, j);
      // peln(i, k, j) on (is:ie, npz+1, js:je); pe(i, k, j) on (is-1:ie+1, npz+1, js-1:je+1)
      const double *pl = peln + (size_t)(j - g.js) * np1 * g.nx + (i - g.is);
      const double *pec = pe + (size_t)(j - g.js + 1) * np1 * (g.nx + 2) + (i - g.is + 1);
      const double pes = pec[(size_t)npz * spe];
      const double cosl = STRAT ? lat[nc + cc] : 0.;
      double tey = 0., tez = 0., cos4 = 0.;
      if (ZUR) {   // :171-172: the column's alone
        const double tmp = lat[cc] / rd_zur_rad;
        tey = 1.0 - 0.19 * (1. - fv3_exp(-(tmp * tmp)));
      } else {
        tey = ap0k * (315.0 - lat[2 * nc + cc]);   // :180
        tez = lat[3 * nc + cc];
        cos4 = lat[4 * nc + cc];
      }
      double peln_hi = pl[(size_t)npz * spl];
      double pl1 = 0., teq1 = 0.;   // pl(k+1), teq(k+1)
      for (int k = npz - 1; k >= 0; k--) {
        const size_t o = a + (size_t)k * n3, oc = cc + (size_t)k * nc;
        const double peln_lo = pl[(size_t)k * spl];
        const double plk = delp[o] / (peln_hi - peln_lo);   // :144
        const double ptk = pt[o];
        const double td = fresh ? 0. : t_dt[oc];
        double teq;
        bool friction = false;
        if (STRAT && plk <= 1.E2) {   // :149-154, the mesosphere
          const double dz = h0 * fv3_log(pl1 / plk);
          const double dt_tropic = -(2.25 * cosl) * dz;
          teq = teq1 + dt_tropic;
          t_dt[oc] = td + ((ptk + rms * teq) * rmr - ptk) * rdt;
        } else if (STRAT && plk <= 100.E2) {   // :156-165, the stratosphere
          const double dz = h0 * fv3_log(pl1 / plk);
          double relx = t_ms + tau * fv3_log(0.01 * plk);
          relx = pdt / (relx * sday);
          const double dt_tropic = 2.25 * cosl * dz;
          teq = teq1 + dt_tropic;
          t_dt[oc] = td + relx * (teq - ptk) / (1. + relx) * rdt;
        } else {   // :167-196, the troposphere
          double sigl = plk / pes;
          double rkt;
          if (ZUR) {
            double tmp = fv3_exp(akap * fv3_log(sigl));
            const double tzz = 0.1 * (1. - tmp) * rakap;
            tmp = tmp * 315.0;
            teq = dmax(t0, tmp * (tey + tzz));
            rkt = rka;
          } else {
            const double f1 = dmax(0., (sigl - sigb) * rsgb);
            const double pz = pkz[oc];
            const double tmp = tey - tez * (fv3_log(pz) + algpk);
            teq = dmax(t0, tmp * pz);
            rkt = rka + drk * f1 * cos4;
          }
          t_dt[oc] = td + rkt * (teq - ptk) / (1. + rkt) * rdt;
          sigl = (sigl - sigb) * rsgb * rkv;   // :188-196, the bottom friction
          if (sigl > 0.) {
            friction = true;
            const double tmp = sigl / (1. + sigl) * rdt;
            const double ud = fresh ? 0. : u_dt[o], vd = fresh ? 0. : v_dt[o];
            const double u1 = ua[o] + ud, v1 = va[o] + vd;
            u_dt[o] = ud - u1 * tmp;
            v_dt[o] = vd - v1 * tmp;
          }
        }
        if (fresh && !friction) {
          u_dt[o] = 0.;
          v_dt[o] = 0.;
        }
        pl1 = plk;
        teq1 = teq;
        peln_hi = peln_lo;
      }
    }
  }
};

struct AgeOfAir {
  Grid g;
  int km, zero;            // zero: time < tiny (:236)
  double age;              // ascale * time (:239)
  const double *pe;
  double *q;
  static constexpr int CH = 256;

  FV3_HD void operator()(int bx, int, int, int tid, double *) const {
    const double p_source = 75000.;   // :229
    const size_t n3 = g.nA();
    const int ncol = g.nx * g.ny;
    const size_t spe = (size_t)g.nx + 2;
    for (int idx = bx * CH + tid; idx < (bx + 1) * CH && idx < ncol; idx += kNT) {
      const int i = g.is + idx % g.nx, j = g.js + idx / g.nx;
      const size_t a = (size_t)g.iA(i, j);
      const double *pec = pe + (size_t)(j - g.js + 1) * (km + 1) * (g.nx + 2) + (i - g.is + 1);
      for (int k = 0; k < km; k++) {
        if (zero) {
          q[a + (size_t)k * n3] = 0.;
        } else if (pec[(size_t)k * spe] >= p_source) {
          q[a + (size_t)k * n3] = age;
        }
      }
    }
  }
};

}  // namespace fv3
