#!/usr/bin/env python3
"""Golden vectors for hord = 1 of the 1-D PPM flux operator (tp_core.F90:394-411), again by EXECUTING the
reference's own docs/examples/tp_core.ipynb, in the manner of make_ppm1d_golden.py (whose cells() / run_case()
do the work).  Runs only where the reference tree is present; the output tests/golden/ppm1d_lin_golden.npz is
committed and is pure data: per case the inputs (q, c), lim_fac, and the face values the notebook computed.

The notebook has an ``ord == 1`` branch that reads a ``lim_fac`` it never defines.  The one edit on top of those
of make_ppm1d_golden.py is therefore a line ``lim_fac = ...`` appended to the user-options cell.

Cases: ord = 1, lim_fac in {1.0, 2.0, 3.0}, the four profiles x 6 steps the low orders get in ppm1d_golden.npz
(the notebook's Gaussian as it is, the two top-hats on the "noise" variant -- the notebook writes ``<=`` where
tp_core.F90 writes ``<`` in the smoothness flag, and the two differ on exactly flat stretches -- and uniform random
data) = 72 vectors of 40 cells.

Nothing else of the notebook pins a scheme this library lacks a reference-held vector for: its fallback branch treats
ord = 2, 3, 4 as ord = 5, and its ``PD`` with ord = 6 is the positive-definite adjustment of hord = -5, which is not
what hord = -6 does in tp_core.F90 (al = max(0, al), then the hord 6 flag).
"""
import json
import os
import sys

import numpy as np

import make_ppm1d_golden as M

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ppm1d_lin_golden.npz")


def main():
    if not os.path.exists(M.NB):
        sys.exit("reference notebook not present (this script only runs in the build container)")
    base = M.cells()
    out, meta, n = {}, [], 0
    for lim_fac in (1.0, 2.0, 3.0):
        src = list(base)
        src[2] = src[2] + f"\nlim_fac = {lim_fac!r}\n"
        for tracer, qmode in ((0, "native"), (1, "noise"), (2, "noise"), (0, "random")):
            rec = M.run_case(src, 1, False, tracer, nsteps=6, seed=2000 + 17 * n, qmode=qmode)
            assert len(rec) == 6
            for step, (q, c, flux) in enumerate(rec):
                key = f"case{n:03d}"
                out[key + "_q"], out[key + "_c"], out[key + "_flux"] = q, c, flux
                meta.append({"key": key, "iord": 1, "lim_fac": lim_fac, "tracer_type": tracer, "qmode": qmode, "step": step})
                n += 1
    out["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {n} vectors")


if __name__ == "__main__":
    main()
