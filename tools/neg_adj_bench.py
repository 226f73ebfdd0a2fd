#!/usr/bin/env python3
"""What neg_adj3 costs: fv3_neg_adj3 on one 384 x 384 x 127 doubly periodic tile, nonhydrostatic, with cld_amt as qa, timed with device
events on (a) a state without any negative water and (b) the same state with negatives planted in about 1 % of the columns (restored
from a device copy before every call: the routine repairs what it is timed on).

Yardsticks, in the same process on the same fields: the five-species fill2D pass of the host (fill2d_mass, the halo update of qt,
fill2d_apply: FvDynamics._fill2d) and fv3_pt_to_theta_v -- both stream the same arrays once.  Reported per case: ms per call and the
algorithmic bytes per second against 8 TB/s.  Algorithmic bytes: the fields the kernel reads over the compute domain -- pt, delp and the
six species, 8, + qa (delz and peln are arguments of the routine, but only its dead saturation block reads them: fv_sg.F90:982,
:1157-1187) -- plus, for (b), 8 bytes for every value that came back different.  Compare only within one run of this script.

usage: neg_adj_bench.py [--nx 384] [--npz 127] [--steps 20] [--warmup 5] [--share 0.01] [--out FILE.json]
       (default FILE: profiles/neg_adj_bench_<build_id>.json)"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=384)
    ap.add_argument("--npz", type=int, default=127)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--share", type=float, default=0.01)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from gfdl_atmos_cubed_sphere_amd import lib as L
    from gfdl_atmos_cubed_sphere_amd.grid import doubly_periodic
    from gfdl_atmos_cubed_sphere_amd.halo import HaloExchanger
    from gfdl_atmos_cubed_sphere_amd.layout import Bounds
    nx, npz = a.nx, a.npz
    bd = Bounds(1, nx, 1, nx)
    g = doubly_periodic(bd, nx + 1, nx + 1, dx_const=26000.0, dy_const=26000.0)
    ctx = L.Context(g, npz, stream=torch.cuda.current_stream().cuda_stream)
    halo = HaloExchanger(ctx, 1, 1, 0, 1)
    rng = np.random.default_rng(7)
    shp = bd.shape("A", npz)
    ng = bd.ng
    pt = np.asfortranarray(rng.uniform(200.0, 300.0, shp))
    delp = np.asfortranarray(rng.uniform(500.0, 1500.0, shp))
    delz = np.asfortranarray(-rng.uniform(100.0, 500.0, (nx, nx, npz)))
    q = np.asfortranarray(rng.uniform(1.0e-6, 1.0e-4, shp + (7,)))
    q[..., 0] = rng.uniform(1.0e-3, 1.0e-2, shp)
    q[..., 6] = rng.uniform(0.05, 1.0, shp)
    # (b): in `share` of the columns a few cells with negative condensates, vapor and cloud fraction
    qb = q.copy(order="F")
    cols = rng.permutation(nx * nx)[:max(1, int(a.share * nx * nx))]
    for c in cols:
        i, j = int(c) % nx + ng, int(c) // nx + ng
        for k in rng.integers(0, npz, 4):
            iq = int(rng.integers(0, 7))
            qb[i, j, k, iq] = -abs(qb[i, j, k, iq]) * (0.5 if iq else 0.05)
    d_pt, d_dp, d_dz = ctx.from_host(pt), ctx.from_host(delp), ctx.from_host(delz)
    d_pt0, d_q, d_q0 = ctx.from_host(pt), ctx.from_host(q), ctx.from_host(q)
    d_qt, d_pkz = ctx.zeros("A", npz), ctx.zeros("CC", npz)
    n3 = int(np.prod(shp))

    def timed(fn, restore=None):
        for _ in range(a.warmup):
            if restore:
                restore()
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.steps):
            if restore:
                restore()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        ms.sort()
        return dict(ms_median=ms[len(ms) // 2], ms_min=ms[0], ms_max=ms[-1])

    def restore():
        d_q.copy_from(d_q0)
        d_pt.copy_from(d_pt0)

    neg = lambda: ctx.neg_adj3(False, None, d_dz, d_dp, d_pt, d_q, qa=7)
    cells = nx * nx * npz
    rows = {}
    # (a) no negatives: nothing is stored (checked)
    r = timed(neg, restore)
    assert np.array_equal(d_q.download(), q) and np.array_equal(d_pt.download(), pt), "neg_adj3 changed a state without negatives"
    r.update(bytes=9 * 8 * cells, stores=0)
    rows["neg_adj3_clean"] = r
    # (b) negatives in `share` of the columns
    d_q0.upload(qb)
    r = timed(neg, restore)
    out_q, out_pt = d_q.download(), d_pt.download()
    stores = int(np.count_nonzero(out_q != qb) + np.count_nonzero(out_pt != pt))
    r.update(bytes=9 * 8 * cells + 8 * stores, stores=stores, columns_planted=int(len(cols)),
             negatives_left=int(np.count_nonzero(out_q[ng:-ng, ng:-ng, :, 1:6] < 0.0)), finite=bool(np.isfinite(out_q).all() and np.isfinite(out_pt).all()))
    rows["neg_adj3_1pct"] = r
    # yardsticks on the same fields: fill2D of the five condensates; T -> theta_v
    d_q0.upload(q)
    restore()

    def fill2d():
        for iq in range(1, 6):
            ctx.fill2d_mass(npz, d_q, d_dp, d_qt, q_offset=iq * n3)
            halo.update([(d_qt, "A")])
            ctx.fill2d_apply(npz, d_qt, d_dp, d_q, q_offset=iq * n3)
    r = timed(fill2d, restore)
    r.update(bytes=5 * (3 + 4) * 8 * cells)      # per species: q, delp read and qt written; qt, q, delp read and q written (area: 2-D)
    rows["fill2d_five_species"] = r
    r = timed(lambda: ctx.pt_to_theta_v(0, 0.6077, L.KAPPA, L.RDGAS, L.GRAV, d_pt, d_dp, d_dz, d_q, d_pkz), restore)
    r.update(bytes=6 * 8 * cells)                # pt, delp, delz, qv read; pt, pkz written
    rows["pt_to_theta_v"] = r
    for r in rows.values():
        r["bytes_per_s"] = r["bytes"] / (r["ms_median"] * 1.0e-3)
        r["of_8TBps"] = r["bytes_per_s"] / PEAK
    res = dict(build_id=L.build_id(), nx=nx, npz=npz, steps=a.steps, share=a.share, device=torch.cuda.get_device_name(0), rows=rows)
    out = a.out or os.path.join(ROOT, "profiles", f"neg_adj_bench_{L.build_id()}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
