! bind(C) driver of the reference's fv_update_phys (model/fv_update_phys.F90:67), called through ctypes by
! tests/golden/make_update_phys_golden.py: one rank, doubly periodic (grid_type 4, square_domain as the reference sets it for
! equal extents), no nest (child_grids of one element, :224), phys_diag and nudge_diag unallocated, nudge off.
subroutine up_run(is, ie, js, je, ng, npz, nq, ncnst, nwat, idx, adjust, hydrostatic, phys_hydrostatic, has_qdt, dt, ptop, tau_h2o, ak, bk, &
                  u, v, w, delp, pt, q, qdiag, ua, va, ps, pe, peln, pk, pkz, phis, u_srf, v_srf, ts, delz, u_dt, v_dt, t_dt, q_dt) &
    bind(C, name="up_run")
  use iso_c_binding
  use fv_arrays_mod, only: fv_grid_type, fv_flags_type, fv_nest_type, fv_grid_bounds_type, phys_diag_type, nudge_diag_type
  use mpp_domains_mod, only: domain2d
  use time_manager_mod, only: time_type
  use tracer_manager_mod, only: up_index, up_adjust
  use fv_mp_mod, only: up_ng
  use fv_update_phys_mod, only: fv_update_phys
  implicit none
  integer(c_int), value :: is, ie, js, je, ng, npz, nq, ncnst, nwat, hydrostatic, phys_hydrostatic, has_qdt
  integer(c_int), intent(in) :: idx(8), adjust(ncnst)
  real(c_double), value :: dt, ptop, tau_h2o
  real(c_double), intent(in) :: ak(npz+1), bk(npz+1)
  real(c_double) :: u(is-ng:ie+ng, js-ng:je+ng+1, npz), v(is-ng:ie+ng+1, js-ng:je+ng, npz), w(is-ng:ie+ng, js-ng:je+ng, npz)
  real(c_double) :: delp(is-ng:ie+ng, js-ng:je+ng, npz), pt(is-ng:ie+ng, js-ng:je+ng, npz), q(is-ng:ie+ng, js-ng:je+ng, npz, nq)
  real(c_double) :: qdiag(is-ng:ie+ng, js-ng:je+ng, npz, nq+1:ncnst), ua(is-ng:ie+ng, js-ng:je+ng, npz), va(is-ng:ie+ng, js-ng:je+ng, npz)
  real(c_double) :: ps(is-ng:ie+ng, js-ng:je+ng), pe(is-1:ie+1, npz+1, js-1:je+1), peln(is:ie, npz+1, js:je), pk(is:ie, js:je, npz+1)
  real(c_double) :: pkz(is:ie, js:je, npz), phis(is-ng:ie+ng, js-ng:je+ng), u_srf(is:ie, js:je), v_srf(is:ie, js:je), ts(is:ie, js:je)
  real(c_double) :: delz(is:ie, js:je, npz), u_dt(is-ng:ie+ng, js-ng:je+ng, npz), v_dt(is-ng:ie+ng, js-ng:je+ng, npz)
  real(c_double) :: t_dt(is:ie, js:je, npz), q_dt(is:ie, js:je, npz, nq)
  type(fv_grid_type), target :: gs
  type(fv_flags_type) :: fl
  type(fv_nest_type) :: nest
  type(fv_grid_bounds_type) :: bd
  type(domain2d) :: dom
  type(time_type) :: time
  type(phys_diag_type) :: phys_diag
  type(nudge_diag_type) :: nudge_diag
  integer, target :: gt
  logical, target :: regional
  integer :: npx, npy, m
  npx = ie - is + 2
  npy = je - js + 2
  gt = 4
  gs%grid_type => gt
  gs%bounded_domain = .false.
  regional = .false.
  gs%regional => regional
  ! update_dwinds_phys points at these before it looks at grid_type (fv_grid_utils.F90:3318-3326); grid_type 4 reads none of them
  allocate(gs%vlon(1, 1, 3), gs%vlat(1, 1, 3), gs%es(3, 1, 1, 2), gs%ew(3, 1, 1, 2))
  allocate(gs%edge_vect_w(1), gs%edge_vect_e(1), gs%edge_vect_s(1), gs%edge_vect_n(1))
  gs%square_domain = npx == npy
  fl%nwat = nwat
  fl%ncnst = ncnst
  fl%tau_h2o = tau_h2o
  fl%hydrostatic = hydrostatic /= 0
  fl%phys_hydrostatic = phys_hydrostatic /= 0
  fl%adj_mass_vmr = 0
  fl%fv_debug = .false.
  fl%range_warn = .false.
  fl%dwind_2d = .false.
  allocate(nest%child_grids(1))
  nest%child_grids = .false.
  bd%is = is; bd%ie = ie; bd%js = js; bd%je = je
  bd%isc = is; bd%iec = ie; bd%jsc = js; bd%jec = je
  bd%isd = is - ng; bd%ied = ie + ng; bd%jsd = js - ng; bd%jed = je + ng
  bd%ng = ng
  up_ng = ng
  up_index = idx
  up_adjust = .true.
  do m = 1, ncnst
    up_adjust(m) = adjust(m) /= 0
  enddo
  if (has_qdt /= 0) then
    call fv_update_phys(dt, is, ie, js, je, is-ng, ie+ng, js-ng, je+ng, ng, nq, u, v, w, delp, pt, q, qdiag, ua, va, ps, pe, peln, pk, pkz, &
                        ak, bk, phis, u_srf, v_srf, ts, delz, hydrostatic /= 0, u_dt, v_dt, t_dt, nwat /= 0, time, .false., gs, &
                        npx=npx, npy=npy, npz=npz, flagstruct=fl, neststruct=nest, bd=bd, domain=dom, ptop=ptop, phys_diag=phys_diag, &
                        nudge_diag=nudge_diag, q_dt=q_dt)
  else
    call fv_update_phys(dt, is, ie, js, je, is-ng, ie+ng, js-ng, je+ng, ng, nq, u, v, w, delp, pt, q, qdiag, ua, va, ps, pe, peln, pk, pkz, &
                        ak, bk, phis, u_srf, v_srf, ts, delz, hydrostatic /= 0, u_dt, v_dt, t_dt, nwat /= 0, time, .false., gs, &
                        npx=npx, npy=npy, npz=npz, flagstruct=fl, neststruct=nest, bd=bd, domain=dom, ptop=ptop, phys_diag=phys_diag, &
                        nudge_diag=nudge_diag)
  endif
end subroutine
