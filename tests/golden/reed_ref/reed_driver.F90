! bind(C) drivers of what tests/golden/make_reed_golden.py cuts from the reference's driver/solo/fv_phys.F90 into the module
! reed_cut_mod of its temporary directory: reed_wrap (the column loop of do_reed_sim_phys with reed_sim_physics inside it),
! DCMIP2016_terminator_advance, and the host-formed planes (Tsurf, the SST factor of qsats, the terminator's k1) from this compiler's
! SIN, COS, EXP, LOG and **.  Called through ctypes.
subroutine reed_run(is, ie, js, je, ng, npz, pdt, hydrostatic, reed_test, do_reed_cond, reed_cond_only, reed_alt_mxg, agrid, delp, pt, ua, va, &
                    q, pe, peln, phis, delz, u_dt, v_dt, t_dt, q_dt, rain) bind(C, name="reed_run")
  use iso_c_binding
  use reed_cut_mod, only: reed_wrap
  implicit none
  integer(c_int), value :: is, ie, js, je, ng, npz, hydrostatic, reed_test, do_reed_cond, reed_cond_only, reed_alt_mxg
  real(c_double), value :: pdt
  real(c_double) :: agrid(is-ng:ie+ng, js-ng:je+ng, 2), delp(is-ng:ie+ng, js-ng:je+ng, npz), pt(is-ng:ie+ng, js-ng:je+ng, npz)
  real(c_double) :: ua(is-ng:ie+ng, js-ng:je+ng, npz), va(is-ng:ie+ng, js-ng:je+ng, npz), q(is-ng:ie+ng, js-ng:je+ng, npz, 1)
  real(c_double) :: pe(is-1:ie+1, npz+1, js-1:je+1), peln(is:ie, npz+1, js:je), phis(is-ng:ie+ng, js-ng:je+ng), delz(is:ie, js:je, npz)
  real(c_double) :: u_dt(is-ng:ie+ng, js-ng:je+ng, npz), v_dt(is-ng:ie+ng, js-ng:je+ng, npz), t_dt(is:ie, js:je, npz)
  real(c_double) :: q_dt(is:ie, js:je, npz, 1), rain(is:ie, js:je)
  call reed_wrap(is, ie, js, je, ng, npz, 1, 1, pdt, hydrostatic /= 0, reed_test, do_reed_cond /= 0, reed_cond_only /= 0, reed_alt_mxg /= 0, &
                 agrid, delp, pt, ua, va, q, pe, peln, phis, delz, u_dt, v_dt, t_dt, q_dt, rain)
end subroutine

! the chained case: q and q_dt with nq tracers, sphum the first
subroutine reed_run_nq(is, ie, js, je, ng, npz, nq, pdt, hydrostatic, reed_test, do_reed_cond, reed_cond_only, reed_alt_mxg, agrid, delp, pt, &
                       ua, va, q, pe, peln, phis, delz, u_dt, v_dt, t_dt, q_dt, rain) bind(C, name="reed_run_nq")
  use iso_c_binding
  use reed_cut_mod, only: reed_wrap
  implicit none
  integer(c_int), value :: is, ie, js, je, ng, npz, nq, hydrostatic, reed_test, do_reed_cond, reed_cond_only, reed_alt_mxg
  real(c_double), value :: pdt
  real(c_double) :: agrid(is-ng:ie+ng, js-ng:je+ng, 2), delp(is-ng:ie+ng, js-ng:je+ng, npz), pt(is-ng:ie+ng, js-ng:je+ng, npz)
  real(c_double) :: ua(is-ng:ie+ng, js-ng:je+ng, npz), va(is-ng:ie+ng, js-ng:je+ng, npz), q(is-ng:ie+ng, js-ng:je+ng, npz, nq)
  real(c_double) :: pe(is-1:ie+1, npz+1, js-1:je+1), peln(is:ie, npz+1, js:je), phis(is-ng:ie+ng, js-ng:je+ng), delz(is:ie, js:je, npz)
  real(c_double) :: u_dt(is-ng:ie+ng, js-ng:je+ng, npz), v_dt(is-ng:ie+ng, js-ng:je+ng, npz), t_dt(is:ie, js:je, npz)
  real(c_double) :: q_dt(is:ie, js:je, npz, nq), rain(is:ie, js:je)
  call reed_wrap(is, ie, js, je, ng, npz, nq, 1, pdt, hydrostatic /= 0, reed_test, do_reed_cond /= 0, reed_cond_only /= 0, reed_alt_mxg /= 0, &
                 agrid, delp, pt, ua, va, q, pe, peln, phis, delz, u_dt, v_dt, t_dt, q_dt, rain)
end subroutine

subroutine term_run(is, ie, js, je, ng, km, pdt, fill, agrid, q) bind(C, name="term_run")
  use iso_c_binding
  use reed_standins_mod, only: term_fill_negative
  use reed_cut_mod, only: DCMIP2016_terminator_advance
  implicit none
  integer(c_int), value :: is, ie, js, je, ng, km, fill
  real(c_double), value :: pdt
  real(c_double) :: agrid(is-ng:ie+ng, js-ng:je+ng, 2), q(is-ng:ie+ng, js-ng:je+ng, km, 2)
  real(c_double), allocatable :: delp(:, :, :)
  allocate(delp(is-ng:ie+ng, js-ng:je+ng, km))
  delp = 0.
  term_fill_negative = fill /= 0
  call DCMIP2016_terminator_advance(is, ie, js, je, is-ng, ie+ng, js-ng, je+ng, km, q, delp, 2, agrid(is-ng, js-ng, 1), agrid(is-ng, js-ng, 2), pdt)
  term_fill_negative = .false.
  if (any(delp /= 0.)) error stop 'reed_driver: the terminator wrote delp'
end subroutine

subroutine reed_planes_run(n, lat, test, tsurf, sstf) bind(C, name="reed_planes_run")
  use iso_c_binding
  use reed_cut_mod, only: reed_planes
  implicit none
  integer(c_int), value :: n, test
  real(c_double), intent(in) :: lat(n)
  real(c_double), intent(out) :: tsurf(n), sstf(n)
  call reed_planes(n, lat, test, tsurf, sstf)
end subroutine

subroutine term_k1_run(n, lon, lat, k1) bind(C, name="term_k1_run")
  use iso_c_binding
  use reed_cut_mod, only: term_k1
  implicit none
  integer(c_int), value :: n
  real(c_double), intent(in) :: lon(n), lat(n)
  real(c_double), intent(out) :: k1(n)
  call term_k1(n, lon, lat, k1)
end subroutine
