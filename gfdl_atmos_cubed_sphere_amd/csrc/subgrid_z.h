// subgrid_z.h -- fv_subgrid_z, what every driver of the reference runs once per dt_atmos right after fv_dynamics
// (driver/SHiELD/atmosphere.F90:599-611, driver/GFDL/atmosphere.F90:729-740, driver/solo/fv_phys.F90:315-354):
//  - FvSubgridZ:       fv_sg_SHiELD (model/fv_sg.F90:76-505), the dry convective adjustment / 2dz mixing of the columns;
//  - UpdateDwindsPhys: update_dwinds_phys (model/fv_grid_utils.F90:3291-3475), the A-grid wind tendencies it returns carried to
//                      the D-grid winds.
//
// FvSubgridZ: one thread per (i, j) column, lanes along i, one launch.  The order of the floating-point operations is the
// reference's (x**2 as x*x, dim(a, b) as max(a - b, 0), no contraction), so the results are those of the compiled Fortran bit for
// bit.  The column's working copies (t0, u0, v0, w0, hd, te, gz and q0 of the nq mixed tracers, fv_sg.F90:102-103) live in a work
// array [field][level][column] -- the reference relaxes towards them from the untouched inputs at the end (:456-478), so they
// cannot be kept in the fields themselves.  Each of the three sweeps (:263-453) walks the column bottom-up with a two-layer
// register window of the seven state fields: a layer is read once and written once per sweep.  The tracers are exchanged through
// the work array pair by pair (:344-348), which keeps the register set independent of nq; what feeds the Richardson number and the
// heat capacities (sphum, the nwat condensates) is read back after the exchange, by the thread that stored it.
//
// What the reference computes and never uses is not built: den (:206, :252), and lcp2, icp2, qs, the saturation routines.
// pm (:194) is formed again where it is used (the same division of the same inputs).  qcon(:, k) is the sum of the condensates
// of the layer as they are when it is read: the reference forms it at the head of a sweep (:278-308) and again for the upper layer
// of a pair that mixed (:350-361), which are the only two places where the condensates of a layer change before it is read.
// nwat: 0, 1, 2, 3, 4 have branches of their own; every other value takes the `else` branches (:242-248, :302-307, :358-361,
// :436-442), which read all five condensates -- that is nwat = 6, and the same code for 5 or 7 and above.  The branch set is a
// template parameter: an instantiation keeps only the species indices and heat capacities its branches read.
#pragma once

#include "fv3_common.h"

namespace fv3 {

// NW: the branch set of nwat -- 0, 1, 2, 3, 4 or 6 (= every other value)
template <bool HYDRO, int NW>
struct FvSubgridZ {
  static constexpr int nwat = NW;
  Grid g;
  int kbot, k_bot_full, nq;
  int sphum, liq_wat, rainwat, ice_wat, snowwat, graupel;   // 0-based tracer indices, -1 = absent
  double fra_full, fra_weak;   // fra(k), :161-169: k <= k_bot_full / below
  double rdt, t_max, t_min;
  double rdgas, rvgas, grav, cp_air, cp_vapor, c_liq, c_ice;
  const double *delp, *pe, *peln, *pkz, *delz;
  double *ta, *qa, *ua, *va, *w, *u_dt, *v_dt;
  double *wk;   // (NF + nq) x kbot x (nx * ny)
  static constexpr int CH = 256;             // columns per workgroup: one per thread
  static constexpr int NF = HYDRO ? 5 : 7;   // t0, u0, v0, hd, gz; w0, te when nonhydrostatic
  enum { T0 = 0, U0, V0, HD, GZ, W0, TE };

  static size_t work_doubles(const Grid &g, int kbot, int nq) { return (size_t)(NF + nq) * kbot * g.nx * g.ny; }

  // cpm, cvm of a layer from its working tracers (:214-249, :408-443)
  FV3_HD void heat_caps(const double *q0, size_t sq, double cv_air, double cv_vap, double &cpm, double &cvm) const {
    if (nwat == 0) {
      cpm = cp_air;
      cvm = cv_air;
    } else if (nwat == 1 || nwat == 2) {
      const double qv = q0[sphum * sq];
      cpm = (1. - qv) * cp_air + qv * cp_vapor;
      cvm = (1. - qv) * cv_air + qv * cv_vap;
    } else if (nwat == 3) {
      const double qv = q0[sphum * sq], q_liq = q0[liq_wat * sq], q_sol = q0[ice_wat * sq];
      cpm = (1. - (qv + q_liq + q_sol)) * cp_air + qv * cp_vapor + q_liq * c_liq + q_sol * c_ice;
      cvm = (1. - (qv + q_liq + q_sol)) * cv_air + qv * cv_vap + q_liq * c_liq + q_sol * c_ice;
    } else if (nwat == 4) {
      const double qv = q0[sphum * sq], q_liq = q0[liq_wat * sq] + q0[rainwat * sq];
      cpm = (1. - (qv + q_liq)) * cp_air + qv * cp_vapor + q_liq * c_liq;
      cvm = (1. - (qv + q_liq)) * cv_air + qv * cv_vap + q_liq * c_liq;
    } else {
      const double qv = q0[sphum * sq], q_liq = q0[liq_wat * sq] + q0[rainwat * sq];
      const double q_sol = q0[ice_wat * sq] + q0[snowwat * sq] + q0[graupel * sq];
      cpm = (1. - (qv + q_liq + q_sol)) * cp_air + qv * cp_vapor + q_liq * c_liq + q_sol * c_ice;
      cvm = (1. - (qv + q_liq + q_sol)) * cv_air + qv * cv_vap + q_liq * c_liq + q_sol * c_ice;
    }
  }
  // total condensate of a layer (:278-308, :350-361)
  FV3_HD double condensate(const double *q0, size_t sq) const {
    if (nwat < 2) return 0.;
    if (nwat == 2) return q0[liq_wat * sq];
    if (nwat == 3) return q0[liq_wat * sq] + q0[ice_wat * sq];
    if (nwat == 4) return q0[liq_wat * sq] + q0[rainwat * sq];
    return q0[liq_wat * sq] + q0[ice_wat * sq] + q0[snowwat * sq] + q0[rainwat * sq] + q0[graupel * sq];
  }

  FV3_HD void operator()(int bx, int, int, int tid, double *) const {
    const double ri_max = 1., ri_min = 0.25, ustar2 = 1.E-4;   // :57-58, :110
    const double cv_vap = cp_vapor - rvgas;                     // :45
    const double cv_air = cp_air - rdgas;                       // :114
    const double rk = cp_air / rdgas + 1.;                      // :115
    const double g2 = 0.5 * grav;                               // :118
    const double xvir = nwat == 0 ? 0. : rvgas / rdgas - 1.;    // :70, :142-146
    const double rz = nwat == 0 ? 0. : rvgas - rdgas;           // :147
    const size_t n3 = g.nA(), nc = g.nCC();
    const int ncol = g.nx * g.ny;
    const size_t sk = (size_t)ncol;            // level stride of the work array
    const size_t sf = (size_t)kbot * ncol;     // field stride of the work array (= tracer stride of its q0 part)
    const size_t sqa = n3 * g.npz;             // tracer stride of qa
    const int np1 = g.npz + 1;
    for (int idx = bx * CH + tid; idx < (bx + 1) * CH && idx < ncol; idx += kNT) {
      const int i = g.is + idx % g.nx, j = g.js + idx / g.nx;
      const size_t a = (size_t)g.iA(i, j), cc = (size_t)g.iCC(i, j);
      // peln(i, k, j) on (is:ie, npz+1, js:je); pe(i, k, j) on (is-1:ie+1, npz+1, js-1:je+1)
      const double *pl = peln + (size_t)(j - g.js) * np1 * g.nx + (i - g.is);
      const double *pec = HYDRO ? pe + (size_t)(j - g.js + 1) * np1 * (g.nx + 2) + (i - g.is + 1) : nullptr;
      const size_t spl = (size_t)g.nx, spe = (size_t)g.nx + 2;
      double *wc = wk + idx;                   // this column of field 0, level 0
      double *q0 = wc + NF * sf;               // ... of tracer 0, level 0
      // ---- :180-261: the working copies, and gz / hd / te bottom-up
      double gzh = 0.;
      for (int k = kbot - 1; k >= 0; k--) {
        const size_t o = a + (size_t)k * n3, ow = (size_t)k * sk;
        for (int iq = 0; iq < nq; iq++) q0[iq * sf + ow] = qa[iq * sqa + o];
        const double t0 = ta[o], u0 = ua[o], v0 = va[o];
        double hd, te = 0., gz, w0 = 0.;
        if (HYDRO) {
          const double tvm = nwat == 0 ? t0 : t0 * (1. + xvir * q0[sphum * sf + ow]);
          const double dpl = pl[(k + 1) * spl] - pl[k * spl];
          const double pm = delp[o] / dpl;
          const double tv = rdgas * tvm;
          gz = gzh + tv * (1. - pec[k * spe] / pm);
          hd = cp_air * tvm + gz + 0.5 * (u0 * u0 + v0 * v0);
          gzh = gzh + tv * dpl;
        } else {
          double cpm, cvm;
          heat_caps(q0 + ow, sf, cv_air, cv_vap, cpm, cvm);
          const double dz = delz[cc + (size_t)k * nc];
          w0 = w[o];
          gz = gzh - g2 * dz;
          const double tmp = gz + 0.5 * (u0 * u0 + v0 * v0 + w0 * w0);
          hd = cpm * t0 + tmp;
          te = cvm * t0 + tmp;
          gzh = gzh - grav * dz;
        }
        wc[T0 * sf + ow] = t0;
        wc[U0 * sf + ow] = u0;
        wc[V0 * sf + ow] = v0;
        wc[HD * sf + ow] = hd;
        wc[GZ * sf + ow] = gz;
        if (!HYDRO) {
          wc[W0 * sf + ow] = w0;
          wc[TE * sf + ow] = te;
        }
      }
      // ---- :263-453: three sweeps, ratio = 0.25, 0.5, 0.999
      for (int n = 1; n <= 3; n++) {
        const double ratio = n == 1 ? 0.25 : (n == 2 ? 0.5 : 0.999);
        gzh = 0.;
        // the lower layer of the first pair
        size_t ow = (size_t)(kbot - 1) * sk;
        double t_k = wc[T0 * sf + ow], u_k = wc[U0 * sf + ow], v_k = wc[V0 * sf + ow], hd_k = wc[HD * sf + ow], gz_k = wc[GZ * sf + ow];
        double w_k = 0., te_k = 0.;
        if (!HYDRO) {
          w_k = wc[W0 * sf + ow];
          te_k = wc[TE * sf + ow];
        }
        double dp_k = delp[a + (size_t)(kbot - 1) * n3];
        double qcon_k = condensate(q0 + ow, sf);
        for (int k = kbot - 1; k >= 1; k--) {   // layers k - 1 (upper, the reference's km1) and k, 0-based
          const size_t o1 = a + (size_t)(k - 1) * n3, ow1 = (size_t)(k - 1) * sk;
          ow = (size_t)k * sk;
          double t_1 = wc[T0 * sf + ow1], u_1 = wc[U0 * sf + ow1], v_1 = wc[V0 * sf + ow1], hd_1 = wc[HD * sf + ow1];
          const double gz_1 = wc[GZ * sf + ow1];
          double w_1 = 0., te_1 = 0.;
          if (!HYDRO) {
            w_1 = wc[W0 * sf + ow1];
            te_1 = wc[TE * sf + ow1];
          }
          const double dp_1 = delp[o1];
          double qcon_1 = condensate(q0 + ow1, sf);
          const double qv_1 = nwat == 0 ? 0. : q0[sphum * sf + ow1], qv_k = nwat == 0 ? 0. : q0[sphum * sf + ow];
          // :315-327
          const double tv1 = t_1 * (1. + xvir * qv_1 - qcon_1);
          const double tv2 = t_k * (1. + xvir * qv_k - qcon_k);
          const double pt1 = tv1 / pkz[cc + (size_t)(k - 1) * nc];
          const double pt2 = tv2 / pkz[cc + (size_t)k * nc];
          const double du = u_1 - u_k, dv = v_1 - v_k;
          double ri = (gz_1 - gz_k) * (pt1 - pt2) / (0.5 * (pt1 + pt2) * (du * du + dv * dv + ustar2));
          if (tv1 > t_max && tv1 > tv2) {
            ri = 0.;
          } else if (tv2 < t_min) {
            ri = dmin(ri, 0.1);
          }
          // :332-340
          const double dpl_k = pl[(k + 1) * spl] - pl[k * spl];
          const double pm_k = dp_k / dpl_k;
          double ri_ref = dmin(ri_max, ri_min + (ri_max - ri_min) * dmax(400.e2 - pm_k, 0.) / 200.e2);
          if (k == 1) {
            ri_ref = 4. * ri_ref;
          } else if (k == 2) {
            ri_ref = 2. * ri_ref;
          } else if (k == 3) {
            ri_ref = 1.5 * ri_ref;
          }
          if (ri < ri_ref) {   // :342-386
            const double x = 1. - dmax(0.0, ri / ri_ref);
            const double mc = ratio * dp_1 * dp_k / (dp_1 + dp_k) * (x * x);
            for (int iq = 0; iq < nq; iq++) {
              const double qk = q0[iq * sf + ow], q1 = q0[iq * sf + ow1];
              const double h0 = mc * (qk - q1);
              q0[iq * sf + ow1] = q1 + h0 / dp_1;
              q0[iq * sf + ow] = qk - h0 / dp_k;
            }
            qcon_1 = condensate(q0 + ow1, sf);
            double h0 = mc * (u_k - u_1);
            u_1 = u_1 + h0 / dp_1;
            u_k = u_k - h0 / dp_k;
            h0 = mc * (v_k - v_1);
            v_1 = v_1 + h0 / dp_1;
            v_k = v_k - h0 / dp_k;
            h0 = mc * (hd_k - hd_1);
            if (HYDRO) {
              hd_1 = hd_1 + h0 / dp_1;
              hd_k = hd_k - h0 / dp_k;
            } else {   // :378-380: the enthalpy difference, mixed into the total energy
              te_1 = te_1 + h0 / dp_1;
              te_k = te_k - h0 / dp_k;
              h0 = mc * (w_k - w_1);
              w_1 = w_1 + h0 / dp_1;
              w_k = w_k - h0 / dp_k;
            }
          }
          // :392-451: the temperature back from the energy
          if (HYDRO) {
            const double rzq_k = nwat == 0 ? rdgas : rdgas + rz * q0[sphum * sf + ow];
            const double rzq_1 = nwat == 0 ? rdgas : rdgas + rz * q0[sphum * sf + ow1];
            t_k = (hd_k - gzh - 0.5 * (u_k * u_k + v_k * v_k)) / (rk - pec[k * spe] / pm_k);
            gzh = gzh + t_k * dpl_k;
            t_k = t_k / rzq_k;
            const double pm_1 = dp_1 / (pl[k * spl] - pl[(k - 1) * spl]);
            t_1 = (hd_1 - gzh - 0.5 * (u_1 * u_1 + v_1 * v_1)) / ((rk - pec[(k - 1) * spe] / pm_1) * rzq_1);
          } else {
            double cpm, cvm;
            heat_caps(q0 + ow1, sf, cv_air, cv_vap, cpm, cvm);
            double tv = gz_1 + 0.5 * (u_1 * u_1 + v_1 * v_1 + w_1 * w_1);
            t_1 = (te_1 - tv) / cvm;
            hd_1 = cpm * t_1 + tv;
            heat_caps(q0 + ow, sf, cv_air, cv_vap, cpm, cvm);
            tv = gz_k + 0.5 * (u_k * u_k + v_k * v_k + w_k * w_k);
            t_k = (te_k - tv) / cvm;
            hd_k = cpm * t_k + tv;
          }
          // layer k is done for this sweep; layer k - 1 becomes the lower layer of the next pair
          wc[T0 * sf + ow] = t_k;
          wc[U0 * sf + ow] = u_k;
          wc[V0 * sf + ow] = v_k;
          wc[HD * sf + ow] = hd_k;
          if (!HYDRO) {
            wc[W0 * sf + ow] = w_k;
            wc[TE * sf + ow] = te_k;
          }
          t_k = t_1; u_k = u_1; v_k = v_1; hd_k = hd_1; gz_k = gz_1; w_k = w_1; te_k = te_1;
          dp_k = dp_1; qcon_k = qcon_1;
        }
        wc[T0 * sf] = t_k;
        wc[U0 * sf] = u_k;
        wc[V0 * sf] = v_k;
        wc[HD * sf] = hd_k;
        if (!HYDRO) {
          wc[W0 * sf] = w_k;
          wc[TE * sf] = te_k;
        }
      }
      // ---- :456-501: relaxation towards the mixed column, the tendencies, the fields
      for (int k = 0; k < kbot; k++) {
        const size_t o = a + (size_t)k * n3, ow = (size_t)k * sk;
        const double fra = k < k_bot_full ? fra_full : fra_weak;
        const double ta0 = ta[o], ua0 = ua[o], va0 = va[o];
        const double t0 = ta0 + (wc[T0 * sf + ow] - ta0) * fra;
        const double u0 = ua0 + (wc[U0 * sf + ow] - ua0) * fra;
        const double v0 = va0 + (wc[V0 * sf + ow] - va0) * fra;
        if (!HYDRO) {
          const double w00 = w[o];
          w[o] = w00 + (wc[W0 * sf + ow] - w00) * fra;
        }
        for (int iq = 0; iq < nq; iq++) {
          const double q00 = qa[iq * sqa + o];
          qa[iq * sqa + o] = q00 + (q0[iq * sf + ow] - q00) * fra;
        }
        u_dt[o] = rdt * (u0 - ua0);
        v_dt[o] = rdt * (v0 - va0);
        ta[o] = t0;
        ua[o] = u0;
        va[o] = v0;
      }
    }
  }
};

// update_dwinds_phys (fv_grid_utils.F90:3291-3475): one thread per (i, j) of a level, i = is .. ie+1, j = js .. je+1; the thread
// updates u(i, j) where i <= ie and v(i, j) where j <= je.  SPHERE = false: grid_type > 3 (:3338-3349).  SPHERE = true: the 3-D
// tendency vector (:3353-3359) is formed again by every thread that reads it (at most four cells), summed to the cell edges
// (:3362-3376), blended along the four face edges with edge_vect_* (:3378-3455; the neighbour along the edge is the one towards
// the middle of it, `j > jm2`), and projected on es(:, :, :, 1) / ew(:, :, :, 2) (:3456-3469).  dwind_2d, regional and nested
// domains (bounded_domain) are not built.
struct DwindsGeom {
  const double *vlon, *vlat;   // A x 3
  const double *es1;           // (is:ie, js:je+1) x 3
  const double *ew2;           // (is:ie+1, js:je) x 3
  const double *edge_vect_w, *edge_vect_e;   // indexed by j - jsd
  const double *edge_vect_s, *edge_vect_n;   // indexed by i - isd
};

template <bool SPHERE>
struct UpdateDwindsPhys {
  Grid g;
  DwindsGeom d;
  double dt5;
  const double *u_dt, *v_dt;
  double *u, *v;
  static constexpr int CH = 256;

  FV3_HD void v3(size_t o, size_t a, double r[3]) const {   // :3355-3357
    const size_t n = g.nA();
    const double ut = u_dt[o], vt = v_dt[o];
    r[0] = ut * d.vlon[a] + vt * d.vlat[a];
    r[1] = ut * d.vlon[a + n] + vt * d.vlat[a + n];
    r[2] = ut * d.vlon[a + 2 * n] + vt * d.vlat[a + 2 * n];
  }
  FV3_HD void ue(int i, int j, size_t ok, double r[3]) const {   // :3364-3366
    double p[3], q[3];
    const size_t a0 = (size_t)g.iA(i, j - 1), a1 = (size_t)g.iA(i, j);
    v3(ok + a0, a0, p);
    v3(ok + a1, a1, q);
    for (int m = 0; m < 3; m++) r[m] = p[m] + q[m];
  }
  FV3_HD void ve(int i, int j, size_t ok, double r[3]) const {   // :3372-3374
    double p[3], q[3];
    const size_t a0 = (size_t)g.iA(i - 1, j), a1 = (size_t)g.iA(i, j);
    v3(ok + a0, a0, p);
    v3(ok + a1, a1, q);
    for (int m = 0; m < 3; m++) r[m] = p[m] + q[m];
  }

  FV3_HD void operator()(int bx, int, int bz, int tid, double *) const {
    const int k = bz;
    const int wx = g.nx + 1, npt = wx * (g.ny + 1);
    const size_t ok = (size_t)k * g.nA();
    for (int idx = bx * CH + tid; idx < (bx + 1) * CH && idx < npt; idx += kNT) {
      const int i = g.is + idx % wx, j = g.js + idx / wx;
      if (i <= g.ie) {
        const size_t ou = (size_t)k * g.nU() + g.iU(i, j);
        if (!SPHERE) {
          u[ou] = u[ou] + dt5 * (u_dt[ok + g.iA(i, j - 1)] + u_dt[ok + g.iA(i, j)]);   // :3342
        } else {
          double e[3];
          ue(i, j, ok, e);
          const bool south = j == 1 && g.js == 1, north = j == g.npy && g.je + 1 == g.npy;
          if (south || north) {   // :3418-3455
            const int im2 = (g.npx - 1) / 2;
            const double ev = (south ? d.edge_vect_s : d.edge_vect_n)[i - g.isd];
            double nb[3];
            ue(i > im2 ? i - 1 : i + 1, j, ok, nb);
            for (int m = 0; m < 3; m++) e[m] = ev * nb[m] + (1. - ev) * e[m];
          }
          const size_t oe = (size_t)g.iFY(i, j), ne = g.nFY();
          u[ou] = u[ou] + dt5 * (e[0] * d.es1[oe] + e[1] * d.es1[oe + ne] + e[2] * d.es1[oe + 2 * ne]);   // :3458-3460
        }
      }
      if (j <= g.je) {
        const size_t ov = (size_t)k * g.nV() + g.iV(i, j);
        if (!SPHERE) {
          v[ov] = v[ov] + dt5 * (v_dt[ok + g.iA(i - 1, j)] + v_dt[ok + g.iA(i, j)]);   // :3347
        } else {
          double e[3];
          ve(i, j, ok, e);
          const bool west = i == 1 && g.is == 1, east = i == g.npx && g.ie + 1 == g.npx;
          if (west || east) {   // :3379-3416
            const int jm2 = (g.npy - 1) / 2;
            const double ev = (west ? d.edge_vect_w : d.edge_vect_e)[j - g.jsd];
            double nb[3];
            ve(i, j > jm2 ? j - 1 : j + 1, ok, nb);
            for (int m = 0; m < 3; m++) e[m] = ev * nb[m] + (1. - ev) * e[m];
          }
          const size_t oe = (size_t)g.iFX(i, j), ne = g.nFX();
          v[ov] = v[ov] + dt5 * (e[0] * d.ew2[oe] + e[1] * d.ew2[oe + ne] + e[2] * d.ew2[oe + 2 * ne]);   // :3465-3467
        }
      }
    }
  }
};

}  // namespace fv3
