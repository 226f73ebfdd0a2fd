"""Check bodies of fv3_interpolate_vertical (interpolate_vertical, tools/fv_diagnostics.F90:4910-4948), shared by
tests/test_diag_hostemu.py (CPU) and tests/test_diag_gpu.py: the library against the numpy restatement tests/ref_fv_diag.py on the
inputs of tests/diag_inputs.py and against the outputs of the reference's compiled Fortran (tests/golden/diag_interpolate_vertical.npz),
refusals, the memory contract, six faces in one launch.

Bound: no exp or log runs on the device (log(plev) is the host's), so the library must give the reference's and the restatement's bits."""
from __future__ import annotations

import ctypes as C

import numpy as np

import diag_inputs as DI
import parity_common as P
import parity_phys as H
import ref_fv_diag as R
from gfdl_atmos_cubed_sphere_amd.lib import Context
from memory_contract import host_out
from parity_phys import compute as cc, same_bits as bits_equal

SHAPES = ((21, 7), (40, 19), (130, 100))      # no multiple of the wavefront; 40 x 19 and 130 x 100 cross a workgroup of 256 columns
KMS = (1, 3, 12, 33, 79)
# 1, 2 hPa: above the first layer mean; 1000 hPa: below the last one on the high ground; the rest inside
LEVELS = tuple(DI.PLEVS[[0, 1, 10, 18, 25, 30]])


class Slab:
    """level n of a (nx, ny, nlev) device array: the entry writes one 2-D field"""

    def __init__(self, a, n):
        self.ptr = a.ptr + 8 * a.shape[0] * a.shape[1] * n
        self.p = C.cast(C.c_void_p(self.ptr), C.POINTER(C.c_double))


def fields(ctx, bd, st, in_ng):
    """[(name, device a3, in_ng, host a3 on the compute domain)]: T in the layout asked for, and a field that only exists on the
    compute domain (the vorticity of fv_diag)"""
    T = ctx.from_host(st["pt"]) if in_ng else ctx.from_host(np.asfortranarray(cc(bd, st["pt"])))
    return [("t", T, in_ng, cc(bd, st["pt"])), ("vort", ctx.from_host(st["vort"]), 0, st["vort"])]


def run_lib(ctx, bd, st, km, in_ng, out_fill=0.0, levels=LEVELS):
    """-> {name: (nx, ny, len(levels))}; the inputs must come back as they went"""
    peln = ctx.from_host(st["peln"])
    got, keep = {}, []
    for name, a3, ng, host in fields(ctx, bd, st, in_ng):
        out = ctx.from_host(host_out((bd.nx, bd.ny, len(levels)), out_fill))
        for n, p in enumerate(levels):
            ctx.interpolate_vertical(km, p, peln, a3, Slab(out, n), in_ng=ng)
        got[name] = out.download()
        keep.append((a3, st["pt"] if (name == "t" and ng) else np.asfortranarray(host)))
    for a3, host in keep:
        assert bits_equal(a3.download(), host), "an input was written"
    assert bits_equal(peln.download(), st["peln"]), "peln was written"
    return got


def run_ref(bd, st, km, levels=LEVELS, cnt=None):
    return {name: np.stack([R.interpolate_vertical(km, p, st["peln"], a3, cnt) for p in levels], axis=2)
            for name, a3 in (("t", cc(bd, st["pt"])), ("vort", st["vort"]))}


def check_against_restatement(lib, shape, km, in_ng, out_fill=0.0):
    """every level of LEVELS, both fields; the branch counts the comparison relies on are asserted first"""
    nx, ny = shape
    bd, st = DI.columns(nx, ny, km, seed=11 + km)
    cnt = {}
    ref = run_ref(bd, st, km, cnt=cnt)
    assert cnt["above_top"] > 0 and cnt["below_bottom"] > 0, cnt
    if km >= 3:
        assert cnt["interior"] > 0, cnt
    ctx = Context(P.make_grid(bd, False), km, lib=lib)
    try:
        got = run_lib(ctx, bd, st, km, in_ng, out_fill)
    finally:
        ctx.close()
    for n in ref:
        assert bits_equal(got[n], ref[n]), f"{n}: not the restatement's bits, max diff {np.max(np.abs(got[n] - ref[n])):.3e}"
    return cnt


# ---- the recorded outputs of the reference's compiled Fortran (tests/golden/make_diag_golden.py) -----------------------------------
GOLDEN_CASES = {"21x7x12": (21, 7, 12, 101), "40x19x33": (40, 19, 33, 102), "21x7x3": (21, 7, 3, 103), "21x7x1": (21, 7, 1, 104),
                "33x9x79": (33, 9, 79, 105)}


def golden():
    return H.golden("diag_", "interpolate_vertical")


def golden_case(name):
    nx, ny, km, seed = GOLDEN_CASES[name]
    bd, st = DI.columns(nx, ny, km, seed)
    g = golden()
    assert str(g[f"{name}|sha"]) == DI.checksum(st), f"{name}: the inputs formed from the seed are not those the golden was recorded with"
    return bd, st, km, {n: g[f"{name}|out|{n}"] for n in ("t", "vort")}


def check_restatement_against_golden(name):
    """no library: the numpy restatement = the compiled reference, bit for bit, and the case takes every branch"""
    bd, st, km, ref = golden_case(name)
    cnt = {}
    got = run_ref(bd, st, km, cnt=cnt)
    assert cnt["above_top"] > 0 and cnt["below_bottom"] > 0 and (km < 3 or cnt["interior"] > 0), cnt
    for n in ref:
        assert bits_equal(got[n], ref[n]), f"{name}: {n} of the restatement is not the reference's"


def check_lib_against_golden(lib, name, in_ng):
    """the library against the recorded outputs with nothing in between"""
    bd, st, km, ref = golden_case(name)
    with H.own_or_borrowed(lib, bd, km) as ctx:
        got = run_lib(ctx, bd, st, km, in_ng, out_fill="pattern")
    for n in ref:
        assert bits_equal(got[n], ref[n]), f"{name}: {n} is not the compiled reference's, max diff {np.max(np.abs(got[n] - ref[n])):.3e}"


def check_on_a_layer_mean(lib):
    """plev exactly on a layer mean of one column takes the `<=` / `>=` sides the reference takes"""
    nx, ny, km = 21, 7, 12
    bd, st = DI.columns(nx, ny, km, seed=5)
    pm = 0.5 * (st["peln"][:, :-1, :] + st["peln"][:, 1:, :])
    levels = tuple(float(np.exp(pm[3, k, 2])) for k in (0, 4, km - 1))
    ref = run_ref(bd, st, km, levels)
    with H.own_or_borrowed(lib, bd, km) as ctx:
        got = run_lib(ctx, bd, st, km, 3, levels=levels)
    for n in ref:
        assert bits_equal(got[n], ref[n]), n


def check_refusals(lib):
    nx, ny, km = 12, 9, 12
    bd, st = DI.columns(nx, ny, km, seed=3)
    with H.own_or_borrowed(lib, bd, km) as ctx:
        peln, a3 = ctx.from_host(st["peln"]), ctx.from_host(st["pt"])
        pat = host_out((nx, ny), "pattern")
        a2 = ctx.from_host(pat)
        check = H.refusals()
        refused = lambda match, *a, **k: check(match, call=lambda: ctx.interpolate_vertical(*a, **k))      # noqa: E731
        refused("null", km, 5.0e4, None, a3, a2, in_ng=3)
        refused("null", km, 5.0e4, peln, None, a2, in_ng=3)
        refused("null", km, 5.0e4, peln, a3, None, in_ng=3)
        refused("km = 0", 0, 5.0e4, peln, a3, a2, in_ng=3)
        refused("plev", km, 0.0, peln, a3, a2, in_ng=3)
        refused("plev", km, -5.0e4, peln, a3, a2, in_ng=3)
        for ng in (1, 2, -3, 4):
            refused("in_ng", km, 5.0e4, peln, a3, a2, in_ng=ng)
        assert bits_equal(a2.download(), pat), "a refused call wrote"


def check_memory_contract(lib, monkeypatch):
    """FV3_MI355X_POISON=1, every device array between guard bands (tests/memory_contract.py): outputs that hold the pattern are
    written whole, no guard band is touched (Context.close raises otherwise), and a call made after another kind of call -- fv_tp_2d
    with its damping work arrays -- gives the bits of a fresh context"""
    import memory_contract as MC
    monkeypatch.setenv("FV3_MI355X_POISON", "1")
    with MC.guarded(monkeypatch):
        for shape, km in (((40, 19), 33), ((21, 7), 3), ((130, 100), 12)):
            for in_ng in (0, 3):
                check_against_restatement(lib, shape, km, in_ng, out_fill="pattern")
        nx, ny, km = 40, 19, 12
        bd, st = DI.columns(nx, ny, km, seed=7)
        g = P.make_grid(bd, True)
        other = MC._tp_case(bd, g, km, 10, 2, 0.06)
        outs = []
        for first in (True, False):
            with H.own_or_borrowed(lib, bd, km, grid=g) as ctx:
                if first:
                    other(ctx)
                outs.append(run_lib(ctx, bd, st, km, 3, out_fill="pattern"))
        for n in outs[0]:
            assert bits_equal(outs[0][n], outs[1][n]), f"{n} after fv_tp_2d in the same context differs from a fresh context's"


def check_six_faces(lib, npx=13, km=12):
    """six C12 faces as one fv3_group: ONE merged launch per call, and the bits of six separate launches"""
    import cubed_common as CC
    from gfdl_atmos_cubed_sphere_amd.cubed_dyn import MultiContext
    cs, gs = CC.sphere(npx)
    n = npx - 1
    sts = [DI.columns(n, n, km, 700 + t)[1] for t in range(6)]
    bd = gs[0].bd
    alone = []
    for t in range(6):
        with H.own_or_borrowed(lib, bd, km, grid=gs[t]) as ctx:
            alone.append(run_lib(ctx, bd, sts[t], km, 3, levels=LEVELS[2:4]))
        ref = run_ref(bd, sts[t], km, LEVELS[2:4])
        for name in ref:
            assert bits_equal(alone[t][name], ref[name]), (t, name)
    mctx = MultiContext([Context(g, km, lib=lib) for g in gs], group=True)
    try:
        assert mctx.group is not None
        peln = mctx.from_host([st["peln"] for st in sts])
        T, vort = mctx.from_host([st["pt"] for st in sts]), mctx.from_host([st["vort"] for st in sts])
        o = {name: [mctx.from_host(np.zeros((n, n), order="F")) for _ in range(2)] for name in ("t", "vort")}

        def calls():
            for k, p in enumerate(LEVELS[2:4]):
                mctx.interpolate_vertical(km, p, peln, T, o["t"][k], in_ng=3)
                mctx.interpolate_vertical(km, p, peln, vort, o["vort"][k], in_ng=0)
        H.merged_once(mctx, "four calls", calls, merged=4)      # only here: one output plane per call, so four calls
        for name in o:
            for k in range(2):
                got = o[name][k].download()
                for t in range(6):
                    assert bits_equal(got[t], alone[t][name][:, :, k]), f"face {t + 1} {name} level {k}"
    finally:
        mctx.close()
