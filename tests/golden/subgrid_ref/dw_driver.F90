! bind(C) driver of the reference's update_dwinds_phys (model/fv_grid_utils.F90:3291), called through ctypes by
! tests/golden/make_subgrid_golden.py.  The gridstruct members the routine reads are handed in the reference's own shapes.
subroutine dw_run(is, ie, js, je, ng, npx, npy, npz, grid_type, dt, u_dt, v_dt, u, v, vlon, vlat, es, ew, ev_w, ev_e, ev_s, ev_n) &
    bind(C, name="dw_run")
  use iso_c_binding
  use fv_arrays_mod, only: fv_grid_type
  use mpp_domains_mod, only: domain2d
  use fv_grid_utils_mod, only: update_dwinds_phys
  implicit none
  integer(c_int), value :: is, ie, js, je, ng, npx, npy, npz, grid_type
  real(c_double), value :: dt
  real(c_double) :: u_dt(is-ng:ie+ng, js-ng:je+ng, npz), v_dt(is-ng:ie+ng, js-ng:je+ng, npz)
  real(c_double) :: u(is-ng:ie+ng, js-ng:je+ng+1, npz), v(is-ng:ie+ng+1, js-ng:je+ng, npz)
  real(c_double), intent(in) :: vlon(is-ng:ie+ng, js-ng:je+ng, 3), vlat(is-ng:ie+ng, js-ng:je+ng, 3)
  real(c_double), intent(in) :: es(3, is-ng:ie+ng, js-ng:je+ng+1, 2), ew(3, is-ng:ie+ng+1, js-ng:je+ng, 2)
  real(c_double), intent(in) :: ev_w(js-ng:je+ng), ev_e(js-ng:je+ng), ev_s(is-ng:ie+ng), ev_n(is-ng:ie+ng)
  type(fv_grid_type), target :: gs
  type(domain2d) :: dom
  integer, target :: gt
  gt = grid_type
  gs%grid_type => gt
  gs%bounded_domain = .false.
  allocate(gs%vlon(is-ng:ie+ng, js-ng:je+ng, 3), gs%vlat(is-ng:ie+ng, js-ng:je+ng, 3))
  allocate(gs%es(3, is-ng:ie+ng, js-ng:je+ng+1, 2), gs%ew(3, is-ng:ie+ng+1, js-ng:je+ng, 2))
  allocate(gs%edge_vect_w(js-ng:je+ng), gs%edge_vect_e(js-ng:je+ng), gs%edge_vect_s(is-ng:ie+ng), gs%edge_vect_n(is-ng:ie+ng))
  gs%vlon = vlon; gs%vlat = vlat; gs%es = es; gs%ew = ew
  gs%edge_vect_w = ev_w; gs%edge_vect_e = ev_e; gs%edge_vect_s = ev_s; gs%edge_vect_n = ev_n
  call update_dwinds_phys(is, ie, js, je, is-ng, ie+ng, js-ng, je+ng, dt, u_dt, v_dt, u, v, gs, npx, npy, npz, dom)
end subroutine
