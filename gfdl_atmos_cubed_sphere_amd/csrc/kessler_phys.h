// kessler_phys.h -- the Kessler warm-rain microphysics of the solo driver: K_warm_rain (driver/solo/fv_phys.F90:1992-2196) with
// kessler_imp (:2202-2291) inside it and qs_wat of driver/solo/qs_tables.F90:67-93, which reads the table fv3_qs_wat_init forms.
//
// KWarmRain: one thread per (i, j) column, lanes along i, one launch.  A cycle of the reference is four loops over k (the fix of
// negative condensates :2089-2103, kessler_imp, the rain flux :2107-2110, the sedimentation transports :2114-2147); their
// dependences allow ONE downward sweep per cycle, level k needing of level k-1 only
//   qr(k-1) AFTER the sedimentation of :2238-2241 and BEFORE the microphysics loop of :2244 / :2267 changes it, r(k-1), vr(k-1),
//   m1(k-1) (a running sum), and the already updated u1(k-1), v1(k-1), t1(k-1) of :2124-2146,
// which are carried in registers; rho(nz) of :2234, the bottom level's drym/(grav*dz), does not change over the cycles and is
// formed once before the first sweep.  There is no private array of length km.
//
// Between cycles the per-level state t1, q1, q2, q3, u1, v1, w1 and the per-level constants drym, dz, qa, qb, qc live in twelve
// work planes of the context, wk[0..11], each (is:ie, js:je, npz), lanes coalesced, under the poison and guard-band contract: the
// first cycle forms them from the inputs (:2031-2085) and writes them, each later cycle reads what the one before wrote, the last
// cycle writes none and goes on to the outputs (:2156-2173) and the pressure fields (:2177-2186) in the same sweep.  With
// K_cycle = 1 the first cycle is the last: no work plane is touched.  u1, v1 are kept only with K_sedi_transport and w1 only with
// do_K_sedi_w: without them u1 = u, v1 = v, w1 = w throughout, and the inputs are read where the reference reads its copies.
//
// pe(k+1) = pe(k) + dp(k) is a running sum down the column and rides on the last sweep; peln(k+1) is overwritten there after the
// hydrostatic dz of level k has read it, and level k+1 reads the OLD value from a register (the reference forms every dz before
// it writes any peln).
//
// Every expression in the reference's order of floating-point operations (left to right, its parentheses, no contraction).  log,
// exp are include/fv3_math.h, x**y with a real y is fv3_exp(y * fv3_log(x)) -- 0 at x = 0, as the reference's: log gives -inf,
// exp of it 0; rain that evaporates completely in one cycle (:2264, ERN = qr) reaches qr**.875 with qr = 0 in the next -- sqrt is
// the hardware's, DIM(a, b) is max(a - b, 0.).
//
// HYD, MK, TR, SW, SH: hydrostatic, moist_kappa, K_sedi_transport, do_K_sedi_w (read with TR only, :2114-2116), do_K_sedi_heat.
#pragma once

#include "fv3_common.h"

namespace fv3 {

constexpr int kQsLen = 2621;   // qs_tables.F90:96

struct KesslerScalars {         // formed in the entry point, each a sub-expression the reference's own expressions begin with
  double dt, sdt;               // dt, dt/real(K_cycle) (:2021)
  double grav, rgrav, rdgas, rvgas, kappa;
  double rdrg, zvir;            // rdgas*rgrav (:2033), rvgas/rdgas - 1. (:470)
  double cv_air, cv_vap, c_liq; // fv_phys.F90:78-79
  double dc_vap, Lv0;           // :83-85
  double hlv_cv;                // hlv / cv_air (:2274)
  double tmin;                  // tice - 160. (qs_tables.F90:79)
  double hg;                    // 0.5*grav (:2137)
  double sdt22;                 // dt*2.2 of :2246 with kessler_imp's dt = sdt
};

FV3_HD double kessler_pow(double x, double y) { return fv3_exp(y * fv3_log(x)); }

template <bool HYD, bool MK, bool TR, bool SW, bool SH>
struct KWarmRain {
  Grid g;
  int ncyc;                                   // K_cycle >= 1
  int i_sphum, i_liq, i_rain;                 // 0-based tracer planes
  KesslerScalars s;
  const double *tw, *dw;                      // table_w, des_w: kQsLen each
  double *ua, *va, *w, *u_dt, *v_dt, *q, *pt, *delp;
  const double *delz;
  double *pe, *peln, *pk, *ps, *rain;
  double *wk;                                 // 12 x (is:ie, js:je, npz); NULL with ncyc = 1
  static constexpr int CH = 256;              // columns per workgroup: one per thread

  // qs_wat (qs_tables.F90:67-93).  ap1 is in [1, 2621]: it = int(ap1) in 1 .. 2621 indexes table_w and des_w; the second index
  // it = int(ap1 - 0.5) is in 0 .. 2620 (ap1 <= 2621 gives it <= 2620), so des_w(it+1) reads at most des_w(2621), the last entry.
  // it = 0 (ta < tmin + 0.05) is the word BEFORE des_w in the reference, not part of the table: it is taken as 0. here and nothing
  // outside the table is read.  Whatever the reference finds there enters as d0 + ap1*(des_w(1) - d0) with des_w(1) ~ 1e-13.
  FV3_HD double qs_wat(double ta, double den, double &dqdt) const {
    double ap1 = 10. * dmax(ta - s.tmin, 0.) + 1.;
    ap1 = dmin(2621., ap1);
    int it = (int)ap1;
    const double es = tw[it - 1] + (ap1 - it) * dw[it - 1];
    const double dem = s.rvgas * ta * den;
    it = (int)(ap1 - 0.5);
    const double d0 = it >= 1 ? dw[it - 1] : 0.;
    dqdt = 10. * (d0 + (ap1 - it) * (dw[it] - d0)) / dem;
    return es / dem;
  }

  FV3_HD void operator()(int bx, int, int, int tid, double *) const {
    const double qv_min = 1.e-7, qc_min = 1.e-8;     // :2008-2009
    const double qr_min = 1.e-8, vr_min = 1.e-3;     // :2222-2223
    const size_t n3 = g.nA(), nc = g.nCC();
    const int ncol = g.nx * g.ny, npz = g.npz, np1 = g.npz + 1;
    const size_t spl = (size_t)g.nx, spe = (size_t)g.nx + 2;   // level strides of peln and pe
    const size_t nw = nc * (size_t)npz;
    const double sdt = s.sdt, grav = s.grav;
    for (int idx = bx * CH + tid; idx < (bx + 1) * CH && idx < ncol; idx += kNT) {
      const int i = g.is + idx % g.nx, j = g.js + idx / g.nx;
      const size_t a = (size_t)g.iA(i, j), cc = (size_t)g.iCC(i, j);
      // peln(i, k, j) on (is:ie, npz+1, js:je); pe(i, k, j) on (is-1:ie+1, npz+1, js-1:je+1)
      double *plc = peln + (size_t)(j - g.js) * np1 * g.nx + (i - g.is);
      double *pec = pe + (size_t)(j - g.js + 1) * np1 * (g.nx + 2) + (i - g.is + 1);
      const double *qa_in = q + (size_t)i_sphum * n3 * npz + a, *qb_in = q + (size_t)i_liq * n3 * npz + a,
                   *qc_in = q + (size_t)i_rain * n3 * npz + a;
      double *wT = wk + cc, *wQ1 = wT + nw, *wQ2 = wQ1 + nw, *wQ3 = wQ2 + nw, *wU = wQ3 + nw, *wV = wU + nw, *wW = wV + nw,
             *wDry = wW + nw, *wDz = wDry + nw, *wQa = wDz + nw, *wQb = wQa + nw, *wQc = wQb + nw;

      // the entry state of one level (:2031-2085): dz, drym, the clamped dry mixing ratios and what the clamps added
      auto entry = [&](int k, double peln_hi, double peln_lo, double &dz, double &drym, double &q1, double &q2, double &q3, double &da,
                       double &db, double &dc) {
        const size_t o = (size_t)k * n3;
        const double qv = qa_in[o];
        if (HYD) dz = s.rdrg * pt[a + o] * (1. + s.zvir * qv) * (peln_hi - peln_lo);
        else dz = -delz[cc + (size_t)k * nc];
        const double dm = delp[a + o];
        q1 = qv * dm;
        q2 = qb_in[o] * dm;
        q3 = qc_in[o] * dm;
        const double qcon = q2 + q3;
        if (qcon > 0.) {
          if (q2 < 0.) {
            q2 = 0.;
            q3 = qcon;
          } else if (q3 < 0.) {
            q3 = 0.;
            q2 = qcon;
          }
        }
        drym = dm - (q1 + q2 + q3);
        da = q1 / drym;
        db = q2 / drym;
        dc = q3 / drym;
        q1 = dmax(da, qv_min);
        q2 = dmax(db, qc_min);
        q3 = dmax(dc, qc_min);
        da = q1 - da;
        db = q2 - db;
        dc = q3 - dc;
      };

      // rho(nz) (:2230, :2234): the bottom level's, from the entry state
      double rho_nz;
      {
        double dz, drym, q1, q2, q3, da, db, dc;
        const int kb = npz - 1;
        entry(kb, HYD ? plc[(size_t)npz * spl] : 0., HYD ? plc[(size_t)kb * spl] : 0., dz, drym, q1, q2, q3, da, db, dc);
        rho_nz = drym / (grav * dz);
      }

      double rsum = 0.;   // rain(i, j) (:2028, :2112)
      for (int n = 0; n < ncyc; n++) {
        const bool first = n == 0, last = n == ncyc - 1;
        double qrs_p = 0., r_p = 0., vr_p = 0., m1_p = 0., u1_p = 0., v1_p = 0., t1_p = 0.;   // level k-1 of this cycle
        double peln_lo = (HYD && first) ? plc[0] : 0.;                                         // the OLD peln(k)
        double pe_run = last ? pec[0] : 0.;                                                    // pe(k) (:2179)
        for (int k = 0; k < npz; k++) {
          const size_t o = a + (size_t)k * n3, oc = cc + (size_t)k * nc;
          double t1, q1, q2, q3, u1 = 0., v1 = 0., w1 = 0., drym, dz, da, db, dc;
          if (first) {
            double peln_hi = 0.;
            if (HYD) peln_hi = plc[(size_t)(k + 1) * spl];
            entry(k, peln_hi, peln_lo, dz, drym, q1, q2, q3, da, db, dc);
            peln_lo = peln_hi;
            t1 = pt[o];
            if (TR) {
              u1 = ua[o];
              v1 = va[o];
              if (SW) w1 = w[o];
            }
          } else {
            t1 = wT[(size_t)k * nc];
            q1 = wQ1[(size_t)k * nc];
            q2 = wQ2[(size_t)k * nc];
            q3 = wQ3[(size_t)k * nc];
            drym = wDry[(size_t)k * nc];
            dz = wDz[(size_t)k * nc];
            da = wQa[(size_t)k * nc];
            db = wQb[(size_t)k * nc];
            dc = wQc[(size_t)k * nc];
            if (TR) {
              u1 = wU[(size_t)k * nc];
              v1 = wV[(size_t)k * nc];
              if (SW) w1 = wW[(size_t)k * nc];
            }
          }
          const double dm = delp[o];   // the moist mass before the call: delp is written by the last cycle only, below
          // :2089-2103
          const double qcon = q2 + q3;
          const double q0 = q1 + qcon;
          if (qcon > 0.) {
            if (q2 < 0.) {
              q2 = 0.;
              q3 = qcon;
            } else if (q3 < 0.) {
              q3 = 0.;
              q2 = qcon;
            }
          }
          // kessler_imp: T = t1, qv = q1, qc = q2, qr = q3, dt = sdt (:2229-2241)
          const double rho = drym / (grav * dz);
          const double pc = 3.8e2 / (rho * s.rdgas * t1);
          const double r = 0.001 * rho;
          double rqr = r * dmax(q3, qr_min);
          double vr = 36.34 * sqrt(rho_nz / rho) * fv3_exp(0.1364 * fv3_log(rqr));
          vr = dmax(vr_min, vr);
          if (k == 0) q3 = dz * q3 / (dz + sdt * vr);
          else q3 = (dz * q3 + qrs_p * r_p * sdt * vr_p / r) / (dz + sdt * vr);
          const double qrs = q3;
          // :2246-2264 / :2269-2287
          const double qrprod = q2 - (q2 - sdt * dmax(.001 * (q2 - .001), 0.)) / (1. + s.sdt22 * kessler_pow(q3, .875));
          q2 = q2 - qrprod;
          q3 = q3 + qrprod;
          rqr = r * dmax(q3, qr_min);
          double dqsdt;
          const double qvs = qs_wat(t1, rho, dqsdt);
          const double hlvm = MK ? (s.Lv0 + s.dc_vap * t1) / (s.cv_air + q1 * s.cv_vap + (q2 + q3) * s.c_liq) : s.hlv_cv;
          const double prod = (q1 - qvs) / (1. + dqsdt * hlvm);
          const double ern = dmin(dmin(sdt * (((1.6 + 124.9 * kessler_pow(rqr, .2046)) * kessler_pow(rqr, .525)) /
                                              (2.55E6 * pc / (3.8 * qvs) + 5.4E5)) *
                                           (dmax(qvs - q1, 0.) / (r * qvs)),
                                       dmax(-prod - q2, 0.)),
                                  q3);
          const double dq = dmax(prod, -q2);
          t1 = t1 + hlvm * (dq - ern);
          q1 = q1 - dq + ern;
          q2 = q2 + dq;
          q3 = q3 - ern;
          // :2107-2110
          double m1 = drym * (q0 - (q1 + q2 + q3));
          if (k > 0) m1 = m1_p + m1;
          if (TR && k > 0) {   // :2114-2132
            if (SW) w1 = (dm * w1 - m1_p * vr_p + m1 * vr) / (dm + m1_p - m1);
            const double fac1 = m1_p / (dm + m1_p);
            const double fac2 = 1. - fac1;
            u1 = fac1 * u1_p + fac2 * u1;
            v1 = fac1 * v1_p + fac2 * v1;
          }
          if (SH && k > 0) {   // :2134-2147
            const double dgz = -s.hg * delz[oc];
            const double cvn = s.cv_air + q1 * s.cv_vap + (q2 + q3) * s.c_liq;
            const double cvm = cvn - s.c_liq * (m1_p - m1) / drym;
            t1 = (drym * cvm * t1 + m1_p * s.c_liq * t1_p + dgz * (m1_p + m1)) / (drym * cvn + m1 * s.c_liq);
          }
          qrs_p = qrs;
          r_p = r;
          vr_p = vr;
          m1_p = m1;
          u1_p = u1;
          v1_p = v1;
          t1_p = t1;
          if (!last) {
            wT[(size_t)k * nc] = t1;
            wQ1[(size_t)k * nc] = q1;
            wQ2[(size_t)k * nc] = q2;
            wQ3[(size_t)k * nc] = q3;
            if (first) {
              wDry[(size_t)k * nc] = drym;
              wDz[(size_t)k * nc] = dz;
              wQa[(size_t)k * nc] = da;
              wQb[(size_t)k * nc] = db;
              wQc[(size_t)k * nc] = dc;
            }
            if (TR) {
              wU[(size_t)k * nc] = u1;
              wV[(size_t)k * nc] = v1;
              if (SW) wW[(size_t)k * nc] = w1;
            }
          } else {   // :2156-2173, :2177-2183
            const double u0 = ua[o], v0 = va[o];
            if (!TR) {
              u1 = u0;
              v1 = v0;
            }
            u_dt[o] = u_dt[o] + (u1 - u0) / s.dt;
            v_dt[o] = v_dt[o] + (v1 - v0) / s.dt;
            if (TR) {
              ua[o] = u1;
              va[o] = v1;
              if (SW) w[o] = w1;
            }
            pt[o] = t1;
            q1 = (q1 + da) * drym;
            q2 = (q2 + db) * drym;
            q3 = (q3 + dc) * drym;
            const double dpn = drym + q1 + q2 + q3;
            delp[o] = dpn;
            q[(size_t)i_sphum * n3 * npz + o] = q1 / dpn;
            q[(size_t)i_liq * n3 * npz + o] = q2 / dpn;
            q[(size_t)i_rain * n3 * npz + o] = q3 / dpn;
            pe_run = pe_run + dpn;
            pec[(size_t)(k + 1) * spe] = pe_run;
            const double pl = fv3_log(pe_run);
            plc[(size_t)(k + 1) * spl] = pl;
            pk[cc + (size_t)(k + 1) * nc] = fv3_exp(s.kappa * pl);
          }
        }
        rsum = rsum + dmax(0., m1_p) / grav;   // :2112
        if (last) ps[a] = pe_run;              // :2185
      }
      rain[cc] = rsum;
    }
  }
};

}  // namespace fv3
