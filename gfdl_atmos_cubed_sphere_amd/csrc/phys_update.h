// phys_update.h -- fv_update_phys (model/fv_update_phys.F90:67-767), what every driver of the reference runs right after the physics
// (atmosphere_state_update of driver/SHiELD/atmosphere.F90 and driver/GFDL/atmosphere.F90, driver/solo/fv_phys.F90): the column
// part.  The wind tendencies go to the D grid through UpdateDwindsPhys (subgrid_z.h) after the caller's halo update.
//
// FvUpdatePhys: one thread per (i, j) column, lanes along i, one launch, one walk down the column.  Every loop of :276-439 is
// pointwise in (i, j), so running them level by level inside a thread is exact; the same walk carries pe down the column for
// :641-663, so delp is read once.  Per level, in the reference's order: the tau_h2o relaxation of q_dt(sphum) (:280-317; qstar and
// p_fac depend on pfull(k) alone and come as two npz arrays formed on the host, p_fac = 0: the level has none), the tracers
// (:322-330), the air mass (:335-338), the mixing ratios (:354-371), the temperature (:375-428), the A-grid winds (:431-437), then
// pe, peln, pk, pkz of the level's lower edge.  The order of the floating-point operations is the reference's (left to right, its
// parentheses, dim(a, b) as max(a - b, 0), no contraction); log and exp are include/fv3_math.h.
//
// The tracer loops run over memory with a stride, so the register set does not depend on nq: the sum of the water tendencies is
// formed first (index order, :337), then each tracer is read, updated, divided and stored once.  The heat capacities read the
// updated species back, from the thread that stored them.  The limiter of the moist constant-volume branch (:412-415) reads the
// pe(k+1) of BEFORE the call and the delp of after the mass adjustment: pe(k+1) is read before the walk overwrites it.
//
// TB, the temperature branch: 0 hydrostatic (moist_cp), 1 nonhydrostatic with phys_hydrostatic (moist_cp, delz at constant
// pressure), 2 nonhydrostatic with nwat = 0 (gama_dt), 3 nonhydrostatic with nwat /= 0 (moist_cv and the tmax limiter).
// NW, the branch set of moist_cp / moist_cv (fv_thermodynamics.F90:250-404, called with t1 present): 2 (the GFS case with its three
// temperature bands), 3, 4, 5, 6, and 0 = `case default` (dry heat capacity: nwat 0, 1, 7, ...).  An instantiation keeps only the
// species indices its branches read.
//
// Not built: nudging (:505-616), adj_mass_vmr /= 0 and Mw_air (:339-346, :360-367), set_physics_BCs and the regional halo fill
// (:224, :682-733), dwind_2d (:665), phys_diag, range_check, fv_debug, ts.
#pragma once

#include "fv3_common.h"

namespace fv3 {

template <int TB, int NW>
struct FvUpdatePhys {
  Grid g;
  int nq, ncnst, nwat;                       // nwat: the namelist's value (the length of the sum, :337)
  int sphum, liq_wat, rainwat, ice_wat, snowwat, graupel, w_diff;   // 0-based tracer indices, -1 = absent
  unsigned long long adj;                    // bit m: tracer m (0-based) is divided by ps_dt (:357: not cld_amt, not w_diff, adjust_mass)
  int has_qdt, relax, winds;                 // present(q_dt); tau_h2o /= 0; the A-grid wind update (off under gfs_phys)
  double dt, ptop, kappa, rdgas, rvgas, grav, cp_air, cp_vapor, c_liq, c_ice;
  const double *qstar, *p_fac;               // npz each (relax only)
  const double *t_dt, *u_dt, *v_dt;
  double *q_dt;                              // (is:ie, js:je, npz, nq), no halo; sphum is written under relax
  double *q, *qdiag, *delp, *pt, *delz, *ua, *va;
  double *ps, *pe, *peln, *pk, *pkz, *u_srf, *v_srf;
  static constexpr int CH = 256;             // columns per workgroup: one per thread

  // moist_cp (AIR = cp_air, VAP = cp_vapor) / moist_cv (cv_air, cv_vap) of one cell, t1 present.  qc: the cell of tracer 0, sq: tracer stride
  FV3_HD double heat_cap(const double *qc, size_t sq, double t1, double c_air, double c_vap) const {
    const double tice = 273.16, t_i0 = 15.;
    if (NW == 2) {   // :265-278, :343-356
      const double q_con = dmax(0., qc[liq_wat * sq]);
      double qs;
      if (t1 > tice) {
        qs = 0.;
      } else if (t1 < tice - t_i0) {
        qs = q_con;
      } else {
        qs = q_con * (tice - t1) / t_i0;
      }
      const double ql = q_con - qs;
      const double qv = dmax(0., qc[sphum * sq]);
      return (1. - (qv + q_con)) * c_air + qv * c_vap + ql * c_liq + qs * c_ice;
    } else if (NW == 3) {
      const double qv = qc[sphum * sq], ql = qc[liq_wat * sq], qs = qc[ice_wat * sq];
      const double q_con = ql + qs;
      return (1. - (qv + q_con)) * c_air + qv * c_vap + ql * c_liq + qs * c_ice;
    } else if (NW == 4) {
      const double qv = qc[sphum * sq];
      const double q_con = qc[liq_wat * sq] + qc[rainwat * sq];
      return (1. - (qv + q_con)) * c_air + qv * c_vap + q_con * c_liq;
    } else if (NW == 5) {
      const double qv = qc[sphum * sq];
      const double ql = qc[liq_wat * sq] + qc[rainwat * sq];
      const double qs = qc[ice_wat * sq] + qc[snowwat * sq];
      const double q_con = ql + qs;
      return (1. - (qv + q_con)) * c_air + qv * c_vap + ql * c_liq + qs * c_ice;
    } else if (NW == 6) {
      const double qv = qc[sphum * sq];
      const double ql = qc[liq_wat * sq] + qc[rainwat * sq];
      const double qs = qc[ice_wat * sq] + qc[snowwat * sq] + qc[graupel * sq];
      const double q_con = ql + qs;
      return (1. - (qv + q_con)) * c_air + qv * c_vap + ql * c_liq + qs * c_ice;
    } else {
      return c_air;
    }
  }

  FV3_HD void operator()(int bx, int, int, int tid, double *) const {
    const double tmax = 330.;                    // :63
    const double cv_air = cp_air - rdgas;        // :165, fv_thermodynamics.F90:40
    const double cv_vap = 3. * rvgas;            // fv_thermodynamics.F90:39
    const double gama_dt = dt * cp_air / cv_air; // :205
    const size_t n3 = g.nA(), nc = g.nCC();
    const int ncol = g.nx * g.ny, npz = g.npz, np1 = g.npz + 1;
    const size_t sq = n3 * npz;                  // tracer stride of q and qdiag
    const size_t sqt = nc * npz;                 // tracer stride of q_dt
    const size_t spl = (size_t)g.nx, spe = (size_t)g.nx + 2;   // level strides of peln and pe
    for (int idx = bx * CH + tid; idx < (bx + 1) * CH && idx < ncol; idx += kNT) {
      const int i = g.is + idx % g.nx, j = g.js + idx / g.nx;
      const size_t a = (size_t)g.iA(i, j), cc = (size_t)g.iCC(i, j);
      // peln(i, k, j) on (is:ie, npz+1, js:je); pe(i, k, j) on (is-1:ie+1, npz+1, js-1:je+1); pk(i, j, k) on (is:ie, js:je, npz+1)
      double *pl = peln + (size_t)(j - g.js) * np1 * g.nx + (i - g.is);
      double *pec = pe + (size_t)(j - g.js + 1) * np1 * (g.nx + 2) + (i - g.is + 1);
      double pe_k = pec[0], peln_k = pl[0];
      double pk_k = TB == 0 ? pk[cc] : 0.;
      double ua_k = 0., va_k = 0.;
      for (int k = 0; k < npz; k++) {
        const size_t o = a + (size_t)k * n3, oc = cc + (size_t)k * nc;
        double dp = delp[o];
        if (has_qdt) {
          double *qd = q_dt + oc;
          double *qc = q + o;
          if (relax) {   // :280-317
            const double pf = p_fac[k];
            if (pf != 0.) qd[sphum * sqt] = qd[sphum * sqt] + (qstar[k] - qc[sphum * sq]) / pf;
          }
          double sum = 0.;   // :337
          for (int m = 0; m < nwat; m++) sum = sum + qd[m * sqt];
          const double ps_dt = 1. + dt * sum;
          dp = dp * ps_dt;   // :338
          delp[o] = dp;
          const bool adjust = nwat != 0;
          for (int m = 0; m < nq; m++) {   // :322-330, :354-361
            if (m == w_diff) continue;
            double x = qc[m * sq] + dt * qd[m * sqt];
            if (adjust && ((adj >> m) & 1ull)) x = x / ps_dt;
            qc[m * sq] = x;
          }
          if (adjust) {   // :362-363
            double *qg = qdiag + o;
            for (int m = nq; m < ncnst; m++)
              if ((adj >> m) & 1ull) qg[(m - nq) * sq] = qg[(m - nq) * sq] / ps_dt;
          }
        }
        // ---- :375-428
        const double t0 = pt[o], td = t_dt[oc];
        if (TB == 0) {
          const double cpm = heat_cap(q + o, sq, t0, cp_air, cp_vapor);
          pt[o] = t0 + td * dt * cp_air / cpm;
        } else if (TB == 1) {
          const double cpm = heat_cap(q + o, sq, t0, cp_air, cp_vapor);
          double dz = delz[oc] / t0;
          const double t1 = t0 + td * dt * cp_air / cpm;
          dz = dz * t1;
          pt[o] = t1;
          delz[oc] = dz;
        } else if (TB == 2) {
          pt[o] = t0 + td * gama_dt;
        } else {
          const double cvm = heat_cap(q + o, sq, t0, cv_air, cv_vap);
          const double tbad = t0 + td * dt * cp_air / cvm;
          const double pe_old = pec[(size_t)(k + 1) * spe];
          delz[oc] = delz[oc] - dp * dmax(tbad - tmax, 0.) * cvm / (grav * (pe_old - ptop));
          pt[o] = dmin(tmax, tbad);
        }
        // ---- :431-437
        if (winds) {
          ua_k = ua[o] + dt * u_dt[o];
          va_k = va[o] + dt * v_dt[o];
          ua[o] = ua_k;
          va[o] = va_k;
        } else if (k == npz - 1) {
          ua_k = ua[o];
          va_k = va[o];
        }
        // ---- :641-663, the lower edge of the level
        const double pe_n = pe_k + dp;
        const double peln_n = fv3_log(pe_n);
        const double pk_n = fv3_exp(kappa * peln_n);
        pec[(size_t)(k + 1) * spe] = pe_n;
        pl[(size_t)(k + 1) * spl] = peln_n;
        pk[cc + (size_t)(k + 1) * nc] = pk_n;
        if (TB == 0) pkz[oc] = (pk_n - pk_k) / (kappa * (peln_n - peln_k));
        pe_k = pe_n;
        peln_k = peln_n;
        pk_k = pk_n;
      }
      ps[a] = pe_k;   // :651-653
      u_srf[cc] = ua_k;
      v_srf[cc] = va_k;
    }
  }
};

}  // namespace fv3
