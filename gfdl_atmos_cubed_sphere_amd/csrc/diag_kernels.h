// diag_kernels.h -- fv_diag (tools/fv_diagnostics.F90) on the resident state.
//  - InterpolateVertical: interpolate_vertical (:4910-4948), a 3-D field at one pressure level
//
// One thread per (i, j) column, i fastest, so every load of the (i, j, k) field and of the (i, k, j) log-pressure is coalesced.  The
// order of the floating-point operations is the reference's (left to right, its parentheses, no contraction).  The reference's
// pm(km) (:4918) is not stored: a layer mean is formed where it is read and carried to the next layer in a register.
#pragma once

#include "fv3_common.h"

namespace fv3 {

struct InterpolateVertical {
  Grid g;
  int km, in_ng;   // in_ng: the halo of a3, 0 = (is:ie, js:je, km), ng = the A layout
  double logp;     // log(plev), taken once on the host (:4922)
  const double *peln, *a3;
  double *a2;
  FV3_HD void operator()(int bx, int, int, int tid, double *) const {
    const int ncol = g.nx * g.ny;
    const size_t nx = (size_t)g.nx;
    const size_t si = nx + 2 * (size_t)in_ng;            // row and level strides of a3
    const size_t sk = si * ((size_t)g.ny + 2 * (size_t)in_ng);
    for (int idx = bx * 256 + tid; idx < (bx + 1) * 256 && idx < ncol; idx += kNT) {
      const int i0 = idx % g.nx, j0 = idx / g.nx;
      const double *pl = peln + (size_t)j0 * (km + 1) * nx + i0;
      const double *ac = a3 + (size_t)(j0 + in_ng) * si + (i0 + in_ng);
      double pa = 0.5 * (pl[0] + pl[nx]);                                                    // pm(1), :4930
      const double pm_bot = 0.5 * (pl[(size_t)(km - 1) * nx] + pl[(size_t)km * nx]);         // pm(km)
      if (logp <= pa) {
        a2[idx] = ac[0];
      } else if (logp >= pm_bot) {
        a2[idx] = ac[(size_t)(km - 1) * sk];
      } else {
        for (int k = 1; k <= km - 1; k++) {
          const double pb = 0.5 * (pl[(size_t)k * nx] + pl[(size_t)(k + 1) * nx]);           // pm(k+1)
          if (logp <= pb && logp >= pa) {
            const double x = ac[(size_t)(k - 1) * sk], y = ac[(size_t)k * sk];
            a2[idx] = x + (y - x) * (logp - pa) / (pb - pa);
            break;
          }
          pa = pb;
        }
      }
    }
  }
};

}  // namespace fv3
