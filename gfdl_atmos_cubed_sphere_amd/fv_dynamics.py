"""Host orchestration of one atmospheric time step -- the build's counterpart of the k_split loop of
``fv_dynamics`` (model/fv_dynamics.F90:460-665): for each remapping cycle the acoustic substeps (``dyn_core``),
the sub-cycled tracer transport (``tracer_2d``) and the vertical remap (``Lagrangian_to_Eulerian``).

``step`` expects the state in the form ``dyn_core`` works on (pt = theta_v, delz < 0); ``step_from_temperature`` is a whole
``fv_dynamics`` call on a Cartesian domain or on the six faces of the sphere: compute_total_energy when consv_te > 0 (:345), T ->
theta_v / theta_m (fv_dynamics.F90:296-399, with moist_cv under use_cond / moist_kappa), the Rayleigh damping when tau > 0
(:362-371: Rayleigh_Super on the cubed sphere and in ideal cases, Rayleigh_Friction otherwise), the k_split loop, the energy
fixer and theta_v -> T in the last remap, the filter of omega (:658-662, nf_omega), neg_adj3 (:722-745, neg_adj), the angular-momentum
fixer (:747-800, consv_am), cubed_to_latlon (:911).  Tracers that are not advected or not remapped (dnats, dnrts, :200-201, :264) and
cld_amt's own remap order (:569-572) follow the reference.  Nudging and the diagnostics are not built.

Behind ``fv_dynamics`` the drivers run ``fv_subgrid_z`` once per dt_atmos (driver/SHiELD/atmosphere.F90:599-611, driver/GFDL/
atmosphere.F90:729-740, driver/solo/fv_phys.F90:315-354): ``fv_subgrid_z`` here is fv_sg_SHiELD and update_dwinds_phys on the device, and
``atmosphere_step`` = ``step_from_temperature`` + ``fv_subgrid_z`` when fv_sg_adj > 0, the drivers' atmosphere_dynamics.  After the
physics the drivers run fv_update_phys (atmosphere_state_update): ``fv_update_phys`` here is the column routine on the device, the halo
update of u_dt, v_dt, update_dwinds_phys and, with gfs_phys, cubed_to_latlon.  Nudging and del2_phys are not built.
"""
from __future__ import annotations

import numpy as np

from .dyn_core import DynCore, DynFlags
from .lib import CP_AIR, NEG_ADJ_CONSTS, Context
from .tracer2d import tracer_2d


CONSV_MIN = 0.001   # fv_mapz.F90:45: below it no correction applies
# prt_negative's names and thresholds at fv_sg.F90:994-1000: T below, the species below
NEGATIVE_THRESHOLDS = (("Temperature", 165.0), ("sphum", -1.0e-8), ("liq_wat", -1.0e-7), ("rainwat", -1.0e-7), ("ice_wat", -1.0e-7),
                       ("snowwat", -1.0e-7), ("graupel", -1.0e-7))


class _TracerView:
    """one tracer (A x npz) of a tracer array on the device, for the entry points that take a field"""

    def __init__(self, q, iq: int):
        self.shape = tuple(q.shape[:3])
        self.ptr = self._as_parameter_ = q.ptr + 8 * int(np.prod(self.shape)) * iq


class FvDynamics:
    def __init__(self, ctx: Context, flags: DynFlags, ak, bk, nq: int = 0, k_split: int = 1, kord_tm: int = -8,
                 kord_mt: int = 8, kord_wz: int = 8, kord_tr: int = 8, q_split: int = 0, nord_tr: int = 0, trdm2: float = 0.0, adiabatic: bool = True,
                 px: int = 1, py: int = 1, rank: int = 0, world: int = 1, dist=None, tau: float = 0.0,
                 rf_cutoff: float = 30.0e2, c2l_ord: int = 4, moist: dict | None = None, fill: bool = False, halo=None,
                 consv_te: float = 0.0, moist_phys: bool = False, radius: float = 6.3712e6, fill2d: tuple = (),
                 remap_te: bool = False, consv_am: dict | None = None, neg_adj: bool = False, check_negative: bool = False,
                 nf_omega: int = 0, dnats: int = 0, dnrts: int = -1, cld_amt: int = 0, neg_adj_consts: dict | None = None,
                 fv_sg_adj: int = 0, fv_sg_adj_weak: int = 0, sg_nq: int | None = None):
        ak, bk = np.asarray(ak, dtype=np.float64), np.asarray(bk, dtype=np.float64)
        dp_ref = (ak[1:] - ak[:-1]) + (bk[1:] - bk[:-1]) * 1.0e5          # dyn_core.F90:241-244
        # flagstruct%tau / %rf_cutoff are ONE pair in the reference: Rayleigh_Friction / _Super here (fv_dynamics.F90:362-376) and Ray_fast /
        # fast_tau_w_sec inside dyn_core (dyn_core.F90:1057-1060) read the same numbers.  The argument and the flags' member are merged
        # (either may carry the value; two different values are an error), so that tau > 0 with rf_fast damps through Ray_fast
        # instead of silently not at all.
        import dataclasses
        if tau != 0.0 and flags.tau != 0.0 and tau != flags.tau:
            raise ValueError(f"FvDynamics: tau = {tau} but flags.tau = {flags.tau} (flagstruct%tau is one number)")
        tau = tau if tau != 0.0 else flags.tau
        rf_default = DynFlags.__dataclass_fields__["rf_cutoff"].default
        if rf_cutoff != rf_default and flags.rf_cutoff != rf_default and rf_cutoff != flags.rf_cutoff:
            raise ValueError(f"FvDynamics: rf_cutoff = {rf_cutoff} but flags.rf_cutoff = {flags.rf_cutoff}")
        rf_cutoff = rf_cutoff if rf_cutoff != rf_default else flags.rf_cutoff
        flags = dataclasses.replace(flags, tau=tau, rf_cutoff=rf_cutoff)
        self.ctx, self.fl, self.nq, self.k_split, self.q_split, self.dist = ctx, flags, nq, k_split, q_split, dist
        self.nord_tr, self.trdm2 = nord_tr, trdm2
        # the tail of fv_dynamics for moist runs.  neg_adj: neg_adj3 after the k_split loop (fv_dynamics.F90:722-745; the reference runs
        # it whenever nwat == 6), check_negative: its prt_negative report (fv_sg.F90:992-1002, :1323-1333), neg_adj_consts: overrides of
        # lib.NEG_ADJ_CONSTS.  nf_omega: passes of del2_cubed on omga after the last remap (:658-662; the reference's default is 1).
        # dnats: the last dnats tracers are not advected (:200-201), dnrts: the last dnrts are not remapped (< 0: = dnats,
        # fv_control.F90:567).  cld_amt: 1-based index of the cloud fraction, 0 = absent: remapped with kord 9 (:571), qa of neg_adj3.
        if dnrts < 0:
            dnrts = dnats
        if not 0 <= dnats <= nq or not 0 <= dnrts <= nq:
            raise ValueError(f"FvDynamics: dnats = {dnats}, dnrts = {dnrts} must lie in 0..nq = {nq}")
        if not 0 <= cld_amt <= nq:
            raise ValueError(f"FvDynamics: cld_amt = {cld_amt} is not a tracer of 1..{nq} (0 = absent)")
        if neg_adj and (moist or {}).get("nwat", 0) != 6:
            raise ValueError("FvDynamics: neg_adj is neg_adj3, the repair of the six water species: it needs moist['nwat'] == 6")
        if dnats and flags.inline_q:
            raise ValueError("FvDynamics: dnats > 0 with inline_q is not built (d_sw's inline tracers take every tracer)")
        if nf_omega < 0:
            raise ValueError(f"FvDynamics: nf_omega = {nf_omega}")
        self.neg_adj, self.check_negative, self.nf_omega = bool(neg_adj), bool(check_negative), int(nf_omega)
        self.dnats, self.dnrts, self.cld_amt = int(dnats), int(dnrts), int(cld_amt)
        self.neg_adj_consts = dict(NEG_ADJ_CONSTS, rdgas=flags.rdgas, grav=flags.grav, cp_air=flags.cp_air, **(neg_adj_consts or {}))
        # the tracer indices (1-based) of the six species: the moist dict's, by default the first six in the reference's usual order
        self.neg_adj_species = tuple(int((moist or {}).get(n, k + 1))
                                     for k, n in enumerate(("sphum", "liq_wat", "rainwat", "ice_wat", "snowwat", "graupel")))
        # fv_subgrid_z: flagstruct%fv_sg_adj / %fv_sg_adj_weak (seconds, integers; <= 0: off), sg_nq = the leading tracers that are mixed
        # (nt_dyn of the SHiELD / GFDL drivers, min(6, nq) of fv_phys.F90:346; default: all).  k_bot_full is flags.n_sponge.
        if not 0 <= (nq if sg_nq is None else sg_nq) <= nq:
            raise ValueError(f"FvDynamics: sg_nq = {sg_nq} must lie in 0..nq = {nq}")
        self.fv_sg_adj, self.fv_sg_adj_weak, self.sg_nq = int(fv_sg_adj), int(fv_sg_adj_weak), int(nq if sg_nq is None else sg_nq)
        self.sg_nwat = int((moist or {}).get("nwat", 0))
        self.sg_species = {n: int((moist or {}).get(n, 0)) for n in ("sphum", "liq_wat", "rainwat", "ice_wat", "snowwat", "graupel")}
        self.rank = rank
        self.negative_report = []          # check_negative: (when, name, minimum) of what fell below its threshold
        # fill2D (fv_dynamics.F90:542-556, FILL2D builds): the 0-based tracer indices of liq_wat, rainwat, ice_wat, snowwat, graupel
        # that get the diffusive filling after tracer_2d when hord_tr < 8 and moist_phys
        self.fill2d = tuple(int(i) for i in fill2d)
        # flagstruct%remap_te (fv_arrays.F90:399): the remap carries total energy in the place of T_v / theta_v
        self.remap_te = bool(remap_te)
        self.tau, self.rf_cutoff, self.c2l_ord = tau, rf_cutoff, c2l_ord
        self.ak, self.bk = ak, bk
        self._rf = None                                                    # (rf, pm, kmax): set on first use, as RF_initialized
        # total-energy conservation (fv_dynamics.F90:345-355, fv_mapz.F90:643-772): fraction of the energy lost in a step that
        # the last remap returns as heat (> consv_min), or a prescribed flux in W/m**2 (< -consv_min)
        self.consv_te, self.moist_phys, self.radius = consv_te, moist_phys, radius
        self.e_flux = 0.0
        # flagstruct%consv_am (fv_dynamics.F90:358-361, :747-800): dict(coslat = cos(agrid(:,:,2)) (A), l2c_u (U), l2c_v (V), zxg (compute
        # domain; idiag%zxg, the mountain-torque term), omega) -- host arrays of the grid (lists of six on the sphere), uploaded on first use
        self.consv_am = consv_am
        self.last_u00 = 0.0
        # moist thermodynamics (flags.use_cond / flags.moist_kappa): nwat and the water-species indices for moist_cv,
        # cv_vap, c_liq, c_ice (lib.Context.set_moist)
        self.moist = None
        if flags.use_cond or flags.moist_kappa:
            self.moist = dict(moist or {}, moist_kappa=int(flags.moist_kappa), use_cond=int(flags.use_cond), sphum=1)
        ph = np.asarray(ak, dtype=np.float64) + np.asarray(bk, dtype=np.float64) * 1.0e5     # fv_dynamics.F90:254-262 (p_ref = 1e5)
        pfull = (ph[1:] - ph[:-1]) / np.log(ph[1:] / ph[:-1])
        ks = int(np.argmax(np.asarray(bk) != 0.0)) - 1 if np.any(np.asarray(bk) != 0.0) else len(pfull)   # the last interface of pure pressure
        self.dc = DynCore(ctx, flags, dp_ref, px, py, rank, world, halo=halo, pfull=pfull, ks=max(ks, 0), akbk=(ak, bk))
        ctx.set_ak_bk(ak, bk)
        npz = ctx.npz
        d = self.dc.d
        d["ps"], d["pkz"] = ctx.zeros("A"), ctx.zeros("CC", npz)
        d["dp1"], d["dp1_nxt"] = ctx.zeros("A", npz), ctx.zeros("A", npz)
        if nq:
            shp = ctx.bd.shape("A", npz) + (nq,)
            d["q"], d["q_nxt"] = ctx.from_host(np.zeros(shp, order="F")), ctx.from_host(np.zeros(shp, order="F"))
        self.remap_par = dict(hydrostatic=int(flags.hydrostatic), adiabatic=int(adiabatic), nq=nq, kord_mt=kord_mt, kord_wz=kord_wz,
                              kord_tm=kord_tm, sphum=1 if nq else 0, akap=flags.akap, ptop=flags.ptop,
                              rdgas=flags.rdgas, grav=flags.grav, cv_air=flags.cp_air - flags.rdgas, r_vir=0.6077,
                              cp=flags.cp_air, t_min=184.0, kord_tr=[kord_tr] * nq, fill=int(fill))
        nr = nq - self.dnrts                                               # :264, :569-572
        if nr != nq or (0 < self.cld_amt <= nr):
            kt = [kord_tr] * nr
            if 0 < self.cld_amt <= nr:
                kt[self.cld_amt - 1] = 9
            self.remap_par.update(nq=nr, kord_tr=kt)

    def set_tracers(self, q: np.ndarray):
        self.dc.d["q"].upload(q)

    def step_from_temperature(self, bdt: float):
        """A whole fv_dynamics call for the adiabatic core: pt holds T (T_v) on entry and on return.
        fv_dynamics.F90:284-399 (T -> theta_v), the k_split loop, and the theta_v -> T conversion that the last remap
        does (fv_mapz.F90:793-821, last_step)."""
        d, ctx, fl = self.dc.d, self.ctx, self.fl
        qv = d["q"] if (self.nq and self.remap_par["sphum"] > 0 and not self.remap_par["adiabatic"]) else None   # first tracer = sphum
        zvir = self.remap_par["r_vir"] if qv else 0.0
        if self.moist:
            ctx.set_moist(self.moist, d.get("q_con"), d.get("cappa"))
        if self.consv_te > CONSV_MIN:                                      # :345-355 (te_2d -> te0_2d of the last remap)
            self.total_energy_before()
        conv = lambda mode: ctx.pt_to_theta_v(mode, zvir, fl.akap, fl.rdgas, fl.grav, d["pt"], d["delp"],
                                              None if fl.hydrostatic else d["delz"], qv, d["pkz"])
        if self.consv_am:                                                  # :358-361: teq, ps2 of the state the step starts from
            self._aam("teq", "ps2")
        if self.tau > 0.0 and not self.fl.rf_fast:                         # :362-376 (RF_fast: Ray_fast inside dyn_core instead) (grid_type = 4: Rayleigh_Friction)
            if not fl.hydrostatic:
                conv(-1)                                                   # pkz from the T, delz before the friction (:323-326)
            self.rayleigh_friction(bdt)
            conv(1)                                                        # :389-397 with that pkz
        else:
            conv(int(fl.hydrostatic))
        self.step(bdt, last_cycle_is_last_step=True)
        if self.neg_adj:                                                   # :722-745
            self._neg_adj3()
        if self.consv_am:                                                  # :747-800
            self._consv_am(bdt)
        self.cubed_to_latlon()                                             # :911

    # -- fv_subgrid_z ---------------------------------------------------------------------------------------------
    def fv_subgrid_z(self, bdt: float):
        """fv_sg_SHiELD and the update of the D-grid winds with the tendencies it returns (driver/SHiELD/atmosphere.F90:587-611,
        fv_update_phys.F90:620-626, :735): on the state step_from_temperature leaves (pt = T, ua / va, pkz, pe, peln)."""
        d, ctx, fl = self.dc.d, self.ctx, self.fl
        if self.fv_sg_adj <= 0:
            raise ValueError("FvDynamics.fv_subgrid_z: fv_sg_adj <= 0 (the drivers do not call fv_sg_SHiELD then)")
        if not self.sg_nq:
            raise ValueError("FvDynamics.fv_subgrid_z: no tracer to mix (fv_sg_SHiELD reads q(:,:,:,sphum))")
        hyd = fl.hydrostatic
        npz = ctx.npz
        if "u_dt" not in d:
            d["u_dt"], d["v_dt"] = ctx.zeros("A", npz), ctx.zeros("A", npz)
        d["u_dt"].zero()                                                   # atmosphere.F90:587-588
        d["v_dt"].zero()
        ctx.fv_subgrid_z(hyd, self.sg_nq, self.sg_nwat, self.sg_species, fl.n_sponge, self.fv_sg_adj, self.fv_sg_adj_weak, bdt, fl.ptop,
                         d["delp"], d["pe"] if hyd else None, d["peln"], d["pkz"], d["pt"], d["q"], d["ua"], d["va"],
                         None if hyd else d["w"], None if hyd else d["delz"], d["u_dt"], d["v_dt"], consts=self.neg_adj_consts)
        self.dc.halo.update([(d["u_dt"], "A"), (d["v_dt"], "A")])          # fv_update_phys.F90:620-626: two scalars
        ctx.update_dwinds_phys(bdt, d["u_dt"], d["v_dt"], d["u"], d["v"])  # :735

    def atmosphere_step(self, bdt: float):
        """the drivers' atmosphere_dynamics: fv_dynamics, then fv_subgrid_z when fv_sg_adj > 0"""
        self.step_from_temperature(bdt)
        if self.fv_sg_adj > 0:
            self.fv_subgrid_z(bdt)

    # -- fv_update_phys -------------------------------------------------------------------------------------------
    def fv_update_phys(self, dt: float, t_dt, q_dt=None, u_dt=None, v_dt=None, phys_hydrostatic: bool = True, gfs_phys: bool = False,
                       tau_h2o: float = 0.0, adjust_mass=None, w_diff: int = 0):
        """fv_update_phys (model/fv_update_phys.F90:67-767; atmosphere_state_update of the drivers) on the resident state: the column
        routine, the halo update of u_dt, v_dt as two scalars (:620-626), update_dwinds_phys (:735) and, with gfs_phys,
        cubed_to_latlon (:738-742).  t_dt (is:ie, js:je, npz), q_dt (is:ie, js:je, npz, nq) or None, u_dt, v_dt (A x npz) or None
        (zero wind tendencies): device arrays, or host arrays that are uploaded.  The species are those of the moist dict and cld_amt
        of the constructor; ps, pe, peln, pk (pkz when hydrostatic) are rebuilt, the bottom winds go to d["u_srf"], d["v_srf"]."""
        d, ctx, fl = self.dc.d, self.ctx, self.fl
        hyd = fl.hydrostatic
        npz = ctx.npz
        dev = lambda a: ctx.from_host(a) if isinstance(a, (np.ndarray, list, tuple)) else a      # noqa: E731
        if "u_srf" not in d:
            d["u_srf"], d["v_srf"] = ctx.zeros("CC"), ctx.zeros("CC")
        for n, a in (("u_dt", u_dt), ("v_dt", v_dt)):
            if a is not None:
                d[n] = dev(a)
            elif n not in d:
                d[n] = ctx.zeros("A", npz)
            else:
                d[n].zero()
        species = dict(self.sg_species, cld_amt=self.cld_amt, w_diff=int(w_diff))
        ctx.fv_update_phys(dt, fl.ptop, hyd, self.nq, self.nq, self.sg_nwat, species, d["u_dt"], d["v_dt"], dev(t_dt),
                           None if q_dt is None else dev(q_dt), d["delp"], d["pt"], d.get("q"), None, d["ua"], d["va"],
                           None if hyd else d["w"], None if hyd else d["delz"], d["ps"], d["pe"], d["peln"], d["pk"], d["pkz"] if hyd else None,
                           d["u_srf"], d["v_srf"], phys_hydrostatic=phys_hydrostatic, gfs_phys=gfs_phys, adjust_mass=adjust_mass,
                           tau_h2o=tau_h2o, ak=self.ak, bk=self.bk, consts=dict(self.neg_adj_consts, kappa=fl.akap))
        self.dc.halo.update([(d["u_dt"], "A"), (d["v_dt"], "A")])          # :620-626, :673: two scalars
        ctx.update_dwinds_phys(dt, d["u_dt"], d["v_dt"], d["u"], d["v"])   # :735
        if gfs_phys:                                                       # :738-742
            self.cubed_to_latlon()

    # -- Held-Suarez forcing --------------------------------------------------------------------------------------
    def held_suarez(self, dt: float, strat: bool = True, zurita: bool = False, rd_zur: float = 1.0 / 25.0, age_tracer: int = 0,
                    time_total: float = 0.0):
        """the do_Held_Suarez path of fv_phys (driver/solo/fv_phys.F90:292-313, :620-627, :675-687) on the resident state, a tile or
        the six faces alike: Held_Suarez_Tend with fresh set writes d["t_dt"], d["u_dt"], d["v_dt"] (the reference zeroes them
        first), fv_update_phys applies them (moist_phys false, no nudging; the reference's q_dt is zero there, which leaves the
        tracers and the air mass with their bits, so none is passed), and age_of_air sets the tracer age_tracer (1-based, 0 = none;
        the reference's -DDO_AGE build takes the last one) from time_total.  No field leaves the device."""
        d, ctx = self.dc.d, self.ctx
        npz = ctx.npz
        if not 0 <= age_tracer <= self.nq:
            raise ValueError(f"FvDynamics.held_suarez: age_tracer = {age_tracer} is not a tracer of 1..{self.nq} (0 = none)")
        if "t_dt" not in d:
            d["t_dt"] = ctx.empty("CC", npz)
        for n in ("u_dt", "v_dt"):
            if n not in d:
                d[n] = ctx.zeros("A", npz)                                 # (the halo: fv_update_phys' exchange fills it)
        ctx.held_suarez_tend(dt, d["delp"], d["peln"], d["pe"], d["pkz"], d["pt"], d["ua"], d["va"], d["u_dt"], d["v_dt"], d["t_dt"],
                             strat=strat, zurita=zurita, rd_zur=rd_zur, fresh=True, radius=self.radius)
        self.fv_update_phys(dt, d["t_dt"], None, d["u_dt"], d["v_dt"])
        if age_tracer:                                                     # hswf.F90:202-205
            q = d["q"]
            if hasattr(q, "a"):                                            # six faces: one tracer view per face
                for t, c in enumerate(ctx.ctxs):
                    c.age_of_air(npz, time_total, d["pe"][t], _TracerView(q[t], age_tracer - 1))
            else:
                ctx.age_of_air(npz, time_total, d["pe"], _TracerView(q, age_tracer - 1))

    def forced_step(self, bdt: float, **hs):
        """atmosphere_step followed by held_suarez: one step of a Held-Suarez climate (the solo driver's atmosphere_dynamics and
        fv_phys with do_Held_Suarez).  A hydrostatic run starts with d["pkz"] set as p_var sets it: step_from_temperature divides by it."""
        self.atmosphere_step(bdt)
        self.held_suarez(bdt, **hs)

    # -- Reed-Jablonowski simple physics ----------------------------------------------------------------------------
    def reed_sim_phys(self, dt: float, reed_test: int = 0, do_reed_cond: bool = True, reed_cond_only: bool = False,
                      reed_alt_mxg: bool = False, terminator=None, term_fill_negative: bool = False, consts: dict | None = None):
        """the do_reed_sim_phys path of fv_phys (driver/solo/fv_phys.F90:292-313, :546-602, :654-658, :675-687) on the resident state, a
        tile or the six faces alike, in the reference's order: reed_sim_physics with fresh set writes d["u_dt"], d["v_dt"], d["t_dt"]
        and the sphum plane of d["q_dt"] (the reference zeroes the four first) and, with do_reed_cond, d["rain"];
        DCMIP2016_terminator_advance when terminator = (Cl, Cl2), 1-based tracer indices, is given; fv_update_phys applies the
        tendencies with the resident q_dt (moist_phys true).  The other planes of q_dt are zeroed once, where it is allocated.  No
        field leaves the device."""
        d, ctx, fl = self.dc.d, self.ctx, self.fl
        npz = ctx.npz
        if not self.nq:
            raise ValueError("FvDynamics.reed_sim_phys: no tracer (reed_sim_physics reads q(:,:,:,sphum))")
        sphum = self.sg_species.get("sphum", 0) or 1
        if terminator is not None:
            cl, cl2 = (int(t) for t in terminator)
            if not (1 <= cl <= self.nq and 1 <= cl2 <= self.nq and cl != cl2):
                raise ValueError(f"FvDynamics.reed_sim_phys: terminator = {terminator} are not two tracers of 1..{self.nq}")
        if "t_dt" not in d:
            d["t_dt"] = ctx.empty("CC", npz)
        for n in ("u_dt", "v_dt"):
            if n not in d:
                d[n] = ctx.zeros("A", npz)                                 # (the halo: fv_update_phys' exchange fills it)
        if "q_dt" not in d:
            d["q_dt"] = ctx.from_host(np.zeros((ctx.bd.nx, ctx.bd.ny, npz, self.nq), order="F"))
        if "rain" not in d:
            d["rain"] = ctx.zeros("CC")
        faces = list(enumerate(ctx.ctxs)) if hasattr(ctx, "ctxs") else [(None, ctx)]
        at = lambda a, t: a if t is None else a[t]      # noqa: E731
        for t, c in faces:
            c.reed_sim_phys(dt, at(d["delp"], t), at(d["pt"], t), at(d["ua"], t), at(d["va"], t), _TracerView(at(d["q"], t), sphum - 1),
                            at(d["pe"], t), at(d["peln"], t), at(d["phis"], t), None if fl.hydrostatic else at(d["delz"], t), at(d["u_dt"], t),
                            at(d["v_dt"], t), at(d["t_dt"], t), _TracerView(at(d["q_dt"], t), sphum - 1), at(d["rain"], t),
                            hydrostatic=fl.hydrostatic, reed_test=reed_test, do_reed_cond=do_reed_cond, reed_cond_only=reed_cond_only,
                            reed_alt_mxg=reed_alt_mxg, fresh=True, consts=dict(dict(self.neg_adj_consts, radius=self.radius), **(consts or {})))
        if terminator is not None:                                         # :654-658
            for t, c in faces:
                c.terminator_advance(npz, dt, _TracerView(at(d["q"], t), cl - 1), _TracerView(at(d["q"], t), cl2 - 1),
                                     term_fill_negative=term_fill_negative)
        self.fv_update_phys(dt, d["t_dt"], d["q_dt"], d["u_dt"], d["v_dt"])

    def moist_forced_step(self, bdt: float, **reed):
        """atmosphere_step followed by reed_sim_phys: one step of a moist idealised run (the solo driver's atmosphere_dynamics and fv_phys
        with do_reed_sim_phys)"""
        self.atmosphere_step(bdt)
        self.reed_sim_phys(bdt, **reed)

    # -- Kessler warm-rain microphysics -----------------------------------------------------------------------------
    def k_warm_rain(self, dt: float, K_cycle: int = 0, K_sedi_transport: bool = False, do_K_sedi_w: bool = False, do_K_sedi_heat: bool = False,
                    consts: dict | None = None):
        """the do_K_warm_rain path of fv_phys (driver/solo/fv_phys.F90:292-313, :466-499, :675-687) on the resident state, a tile or the
        six faces alike: d["u_dt"], d["v_dt"] are zeroed as the reference zeroes them, K_warm_rain updates pt, delp, the tracers
        sphum, liq_wat, rainwat of the moist dict, ua, va, w in place, rebuilds pe, peln, pk, ps and writes d["rain"] [kg/dA].  With
        K_sedi_transport fv_update_phys follows with the resident u_dt, v_dt and zero t_dt, q_dt (:499: no_tendency false);
        otherwise nothing follows.  moist_kappa is the flags'.  Not applied: the do_terminator rescaling of :476-515.  No
        field leaves the device."""
        d, ctx, fl = self.dc.d, self.ctx, self.fl
        npz = ctx.npz
        sp = {n: int(self.sg_species.get(n, 0) or 0) for n in ("sphum", "liq_wat", "rainwat")}
        if not all(1 <= v <= self.nq for v in sp.values()):
            raise ValueError(f"FvDynamics.k_warm_rain: the moist dict names {sp}; K_warm_rain reads sphum, liq_wat and rainwat of 1..{self.nq}")
        for n in ("u_dt", "v_dt"):                                          # :292-313
            if n not in d:
                d[n] = ctx.zeros("A", npz)
            else:
                d[n].zero()
        if "rain" not in d:
            d["rain"] = ctx.zeros("CC")
        hyd = fl.hydrostatic
        k = dict(dict(self.neg_adj_consts, kappa=fl.akap), **(consts or {}))
        ctx.k_warm_rain(dt, d["ua"], d["va"], None if hyd else d["w"], d["u_dt"], d["v_dt"], d["q"], d["pt"], d["delp"],
                        None if hyd else d["delz"], d["pe"], d["peln"], d["pk"], d["ps"], d["rain"], self.nq, sphum=sp["sphum"],
                        liq_wat=sp["liq_wat"], rainwat=sp["rainwat"], K_cycle=K_cycle, K_sedi_transport=K_sedi_transport,
                        do_K_sedi_w=do_K_sedi_w, do_K_sedi_heat=do_K_sedi_heat, hydrostatic=hyd, moist_kappa=bool(fl.moist_kappa), consts=k)
        if K_sedi_transport:                                               # :499, :675-687
            if "t_dt" not in d:
                d["t_dt"] = ctx.zeros("CC", npz)
            else:
                d["t_dt"].zero()
            if "q_dt" not in d:
                d["q_dt"] = ctx.from_host(np.zeros((ctx.bd.nx, ctx.bd.ny, npz, self.nq), order="F"))
            else:
                d["q_dt"].zero()
            self.fv_update_phys(dt, d["t_dt"], d["q_dt"], d["u_dt"], d["v_dt"])

    def supercell_step(self, bdt: float, **kessler):
        """atmosphere_step followed by k_warm_rain: one step of the supercell case with its microphysics (the solo driver's
        atmosphere_dynamics and fv_phys with do_K_warm_rain)"""
        self.atmosphere_step(bdt)
        self.k_warm_rain(bdt, **kessler)

    # -- neg_adj3 -------------------------------------------------------------------------------------------------
    def _prt_negative(self, when: str):
        """prt_negative (fv_sg.F90:1372-1392) of T and the six species: the global minimum, reported when below its threshold"""
        d, ctx = self.dc.d, self.ctx
        multi = hasattr(ctx, "ctxs")
        for n, (name, thr) in enumerate(NEGATIVE_THRESHOLDS):
            if n == 0:
                f = d["pt"]
            elif multi:
                from .cubed_dyn import FaceSet
                f = FaceSet([_TracerView(a, self.neg_adj_species[n - 1] - 1) for a in d["q"].a])
            else:
                f = _TracerView(d["q"], self.neg_adj_species[n - 1] - 1)
            out = ctx.prt_maxmin(f, 1.0)
            qmin = min(o[1] for o in out) if multi else out[1]
            if self.dist is not None:                                      # mp_reduce_min over the ranks of the host's process group
                import torch
                t = torch.tensor([qmin], dtype=torch.float64)
                if self.dist.get_backend() == "nccl":
                    t = t.cuda()
                self.dist.all_reduce(t, op=self.dist.ReduceOp.MIN)
                qmin = float(t.cpu()[0])
            if qmin < thr:
                self.negative_report.append((when, name, qmin))
                if self.rank == 0:
                    print(f" {name} min (negative) = {qmin!r}")

    def _neg_adj3(self):
        d, ctx, hyd = self.dc.d, self.ctx, self.fl.hydrostatic
        if self.check_negative:
            self._prt_negative("before")
        ctx.neg_adj3(hyd, d["peln"] if hyd else None, None if hyd else d["delz"], d["delp"], d["pt"], d["q"],
                     species=self.neg_adj_species, qa=self.cld_amt, consts=self.neg_adj_consts)
        if self.check_negative:
            self._prt_negative("after")

    def _carry_unadvected(self, dst, src):
        """the last dnats tracers from one buffer of the tracer ping-pong pair to the other: tracer_2d leaves them where they were"""
        nadv = self.nq - self.dnats
        for a, b in zip(getattr(dst, "a", [dst]), getattr(src, "a", [src])):
            n3 = int(np.prod(a.shape[:3]))
            a.ctx.call("fv3_memcpy_d2d", a.ptr + 8 * n3 * nadv, b.ptr + 8 * n3 * nadv, 8 * n3 * self.dnats)

    # -- consv_am -------------------------------------------------------------------------------------------------
    def _aam(self, aam_name: str, ps_name: str):
        """compute_aam (fv_dynamics.F90:1266-1314): cubed_to_latlon(ord 2), then aam, m_fac, ps of every column"""
        d, ctx, fl, ca = self.dc.d, self.ctx, self.fl, self.consv_am
        if "coslat" not in d:
            d["coslat"], d["l2c_u"], d["l2c_v"] = ctx.from_host(ca["coslat"]), ctx.from_host(ca["l2c_u"]), ctx.from_host(ca["l2c_v"])
            d["m_fac"] = ctx.zeros("CC")
        for n, kind in ((aam_name, "CC"), (ps_name, "A")):
            if n not in d:
                d[n] = ctx.zeros(kind)
        ctx.c2l(2, d["u"], d["v"], d["ua"], d["va"])                       # :1287 (mode 1, c2l_ord 2: no halo update)
        ctx.compute_aam(self.radius, ca.get("omega", 7.292e-5), 1.0 / fl.grav, fl.ptop, d["coslat"], d["ua"], d["delp"], d[aam_name],
                        d["m_fac"], d[ps_name])

    def _consv_am(self, bdt: float):
        from .global_sum import g_sum
        d, ctx = self.dc.d, self.ctx
        self._aam("aam2", "ps")
        aslist = lambda x: x if isinstance(x, list) else [x]
        areas = self._areas()
        b = ctx.bd
        cc = lambda a: np.asarray(a)[b.ng:b.ng + b.nx, b.ng:b.ng + b.ny]
        te, teq, ps2, ps = (aslist(d[n].download()) for n in ("aam2", "teq", "ps2", "ps"))
        zxg = aslist(self.consv_am["zxg"])
        dt2 = 0.5 * bdt
        te_2d = [t - q + dt2 * (cc(p2) + cc(p1)) * np.asarray(z) for t, q, p2, p1, z in zip(te, teq, ps2, ps, zxg)]     # :761-767
        amdt = g_sum(te_2d, areas, self.dist)                              # :771
        u00 = -self.radius * amdt / g_sum(aslist(d["m_fac"].download()), areas, self.dist)    # :772
        self.last_u00 = u00
        ctx.consv_am_apply(u00, d["l2c_u"], d["l2c_v"], d["u"], d["v"])    # :784-798

    # -- consv_te -------------------------------------------------------------------------------------------------
    def total_energy_before(self):
        """compute_total_energy at fv_dynamics.F90:345 (pt = T, before the conversion to theta_v): te0_2d of every column"""
        d, ctx, hyd = self.dc.d, self.ctx, self.fl.hydrostatic
        if "te0_2d" not in d:
            for n in ("te0_2d", "te_2d", "zsum1", "zsum0"):
                d[n] = ctx.zeros("CC")
        if self.moist:
            ctx.set_moist(self.moist, d.get("q_con"), d.get("cappa"))
        ctx.compute_total_energy(self.remap_par, self.moist_phys, d["u"], d["v"], None if hyd else d["w"],
                                 None if hyd else d["delz"], d["pt"], d["delp"], d.get("q"), None, d["pe"] if hyd else None,
                                 d["peln"] if hyd else None, d["phis"], d["te0_2d"])
        self._te0_valid = True          # consumed (and cleared) by the energy fixer of this call's last remap

    def _areas(self):
        """area (compute domain) of every context: the weights of g_sum (area_64, fv_mapz.F90:736)"""
        ctxs = getattr(self.ctx, "ctxs", [self.ctx])
        out = []
        for c in ctxs:
            b = c.bd
            out.append(np.asarray(c.grid.m["area"])[b.ng:b.ng + b.nx, b.ng:b.ng + b.ny])
        return out

    def _energy_fixer(self, par: dict, pdt: float):
        """fv_mapz.F90:643-772 after the remap of the last step, then step 9a with dtmp (:793-821)"""
        from .global_sum import g_sum
        d, ctx, hyd = self.dc.d, self.ctx, self.fl.hydrostatic
        only_sums = self.consv_te < 0.0
        if not only_sums and not getattr(self, "_te0_valid", False):
            # te_2d = te0_2d - E(remapped column): without the energy of THIS call's initial state (fv_dynamics.F90:345-355, which
            # step_from_temperature does and a bare step() does not) dtmp would be -E / zsum, applied to pt.  A te0_2d left from an
            # earlier call is as wrong.
            raise RuntimeError("consv_te > 0: total_energy_before() was not called for this step (te0_2d unset or stale); "
                               "use step_from_temperature(), or call total_energy_before() on the temperature state first")
        self._te0_valid = False
        for n in ("te0_2d", "te_2d", "zsum1", "zsum0"):
            if n not in d:
                d[n] = ctx.zeros("CC")
        ctx.energy_fixer_sums(par, only_sums, d["u"], d["v"], None if hyd else d["w"], None if hyd else d["delz"], d["pt"],
                              d["delp"], d.get("q"), d["pe"] if hyd else None, d["peln"] if hyd else None, d["phis"], d["pkz"],
                              d["pk"] if hyd else None, d["te0_2d"], d["te_2d"], d["zsum1"], d["zsum0"] if hyd else None)
        aslist = lambda x: x if isinstance(x, list) else [x]
        areas = self._areas()
        zs = g_sum(aslist(d["zsum0" if hyd else "zsum1"].download()), areas, self.dist)
        if only_sums:                                                      # :745-771: a prescribed flux
            self.e_flux = self.consv_te
            dtmp = self.e_flux * (self.fl.grav * pdt * 4.0 * np.pi * self.radius ** 2) / zs
        else:
            dtmp = self.consv_te * g_sum(aslist(d["te_2d"].download()), areas, self.dist)
            self.e_flux = dtmp / (self.fl.grav * pdt * 4.0 * np.pi * self.radius ** 2)
            dtmp = dtmp / zs
        self.dtmp = dtmp
        ctx.remap_finish(par, dtmp, d["pt"], d["pkz"], d.get("q"))

    def rayleigh_profile(self, dt: float):
        """rf(k), kmax of Rayleigh_Friction (fv_dynamics.F90:1169-1182) with pfull of fv_dynamics.F90:254-262 (p_ref = 1e5)"""
        ak, bk, ptop, akap = self.ak, self.bk, self.fl.ptop, self.fl.akap
        ph = ak + bk * 1.0e5
        pfull = (ph[1:] - ph[:-1]) / np.log(ph[1:] / ph[:-1])
        rf = np.zeros(len(pfull))
        kmax = 0
        for k, pm in enumerate(pfull):
            if pm < self.rf_cutoff:
                rf[k] = dt / (self.tau * 86400.0) * np.sin(0.5 * np.pi * np.log(self.rf_cutoff / pm) / np.log(self.rf_cutoff / ptop)) ** 2
                kmax = k + 1
            else:
                break
        return rf, pfull, kmax

    def rayleigh_friction(self, bdt: float, conserve: bool = True):
        """fv_dynamics.F90:362-371: Rayleigh_Super (:953-1124) on the cubed sphere (grid_type < 4) and in ideal cases, Rayleigh_Friction
        (:1126-1264, two kernels around the halo update of u2f) on the Cartesian domains"""
        d, ctx, fl = self.dc.d, self.ctx, self.fl
        if self._rf is None:
            self._rf = self.rayleigh_profile(abs(bdt))
        rf, pm, kmax = self._rf
        if kmax == 0:
            return
        hyd = fl.hydrostatic
        if ctx.grid.grid_type < 4 or fl.is_ideal_case:
            ideal = fl.is_ideal_case
            if ideal and "u00" not in d:                                       # :997-1014: the winds of the first call are kept
                d["u00"], d["v00"] = ctx.zeros("U", ctx.npz), ctx.zeros("V", ctx.npz)
                d["u00"].copy_from(d["u"])
                d["v00"].copy_from(d["v"])
            ctx.c2l(2, d["u"], d["v"], d["ua"], d["va"])                       # :1040-1042
            ctx.rayleigh_super(kmax, not ideal, hyd, fl.cp_air, fl.rdgas, fl.ptop, pm[:kmax], rf[:kmax], d["ua"], d["va"],
                               d["pt"], d["u"], d["v"], None if hyd else d["w"], d.get("u00") if ideal else None,
                               d.get("v00") if ideal else None)
            return
        if "u2f" not in d:
            d["u2f"] = ctx.zeros("A", ctx.npz)
        ctx.rayleigh_u2f(kmax, hyd, d["u"], d["v"], None if hyd else d["w"], d["ua"], d["va"], d["u2f"])
        self.dc.halo.update([(d["u2f"], "A")])                             # :1207-1209
        ctx.rayleigh_apply(kmax, conserve, hyd, fl.cp_air, fl.rdgas, fl.ptop, pm[:kmax], rf[:kmax], d["u2f"], d["pt"],
                           None if hyd else d["delz"], d["u"], d["v"], None if hyd else d["w"])

    def cubed_to_latlon(self):
        """A-grid winds for the physics (fv_dynamics.F90:911; c2l_ord4 updates the halo of u, v first, :2372-2376)"""
        d = self.dc.d
        if self.c2l_ord == 4:
            self.dc.halo.update([(d["u"], "U"), (d["v"], "V")])
        self.ctx.c2l(self.c2l_ord, d["u"], d["v"], d["ua"], d["va"])

    def _fill2d(self):
        """fill2D (fv_fill.F90:183-258) of the water species named at construction: qt = q delp area, its halo (width 1), the fluxes
        between cells of opposite sign and the update of q"""
        d, ctx = self.dc.d, self.ctx
        npz = ctx.npz
        if "qt" not in d:
            d["qt"] = ctx.zeros("A", npz)
        n3 = int(np.prod(d["delp"].shape))
        for iq in self.fill2d:
            ctx.fill2d_mass(npz, d["q"], d["delp"], d["qt"], q_offset=iq * n3)
            self.dc.halo.update([(d["qt"], "A")])                               # :236
            ctx.fill2d_apply(npz, d["qt"], d["delp"], d["q"], q_offset=iq * n3)

    def step(self, bdt: float, last_cycle_is_last_step: bool = False):
        """One dt_atmos: k_split x (n_split acoustic substeps, tracer transport, vertical remap)."""
        d, ctx = self.dc.d, self.ctx
        mdt = bdt / float(self.k_split)
        if "diss_est" in d:                                                    # do_diss_est: dyn_core zeroes it on init_step = (n_map == 1), :497
            d["diss_est"].zero()
        for n_map in range(1, self.k_split + 1):
            last_step = last_cycle_is_last_step and n_map == self.k_split
            d["dp1"].copy_from(d["delp"])                                      # fv_dynamics.F90:475-481
            if self.fl.use_cond:
                self.dc.halo.update([(d["q_con"], "A")])                       # :464 / :487 (pack 11)
            if self.fl.moist_kappa:
                self.dc.halo.update([(d["cappa"], "A")])                       # :465 / :488 (pack 12)
            self.dc.run(mdt, end_step=(n_map == self.k_split))                 # :493, last_step = (n_map == k_split)
            if self.nq and not self.fl.inline_q:                               # :509-533 (inline_q: the tracers rode inside d_sw)
                q, dp1, _ = tracer_2d(ctx, self.dc.halo, d["q"], d["q_nxt"], d["dp1"], d["dp1_nxt"], d["mfx"], d["mfy"],
                                      d["cx"], d["cy"], d["crx"], d["cry"], self.nq - self.dnats, self.fl.hord_tr, self.q_split,
                                      self.nord_tr, self.trdm2, dist=self.dist)          # nq = nq_tot - dnats, :200
                if q is not d["q"]:
                    if self.dnats:
                        self._carry_unadvected(d["q_nxt"], d["q"])
                    d["q"], d["q_nxt"] = d["q_nxt"], d["q"]
                if dp1 is not d["dp1"]:
                    d["dp1"], d["dp1_nxt"] = d["dp1_nxt"], d["dp1"]
                if self.fill2d and self.fl.hord_tr < 8 and self.moist_phys:     # :542-556
                    self._fill2d()
            fixer = last_step and abs(self.consv_te) > CONSV_MIN                # fv_mapz.F90:645-647, :745
            par = dict(self.remap_par, last_step=2 if fixer else int(last_step))
            hyd = self.fl.hydrostatic
            if self.moist:                                                     # q_con is a ping-pong pair: current buffer
                ctx.set_moist(self.moist, d.get("q_con"), d.get("cappa"))
            if self.remap_te:                                                  # te = dp1, as fv_dynamics.F90:612 hands it over
                ctx.set_remap_te(True, d["phis"], d["dp1"])
            ctx.lagrangian_to_eulerian(par, d["ps"], d["pe"], d["delp"], d["pkz"], d["pk"], d["u"], d["v"],
                                       None if hyd else d["w"], None if hyd else d["delz"], d["pt"], d.get("q"),
                                       d["peln"], d["omga"], None if hyd else d["ws"])   # :607
            if fixer:
                self._energy_fixer(par, bdt)
            if last_step and self.nf_omega > 0:                                # :658-662
                self.dc.halo.update([(d["omga"], "A")])                        # del2_cubed's mpp_update_domains, dyn_core.F90:2399
                ctx.del2_cubed(d["omga"], 0.18 * ctx.grid.da_min, self.nf_omega)
