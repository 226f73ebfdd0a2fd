! bind(C) drivers of the reference's qs_tables_mod (driver/solo/qs_tables.F90, compiled unmodified) and of what
! tests/golden/make_kessler_golden.py cuts from driver/solo/fv_phys.F90 into the module kessler_cut_mod of its temporary directory:
! K_warm_rain with kessler_imp.  Called through ctypes.
subroutine qs_table_run(n, tw, dw) bind(C, name="qs_table_run")
  use iso_c_binding
  use qs_tables_mod, only: qs_wat_init, table_w, des_w
  implicit none
  integer(c_int), value :: n
  real(c_double), intent(out) :: tw(n), dw(n)
  call qs_wat_init
  if (size(table_w) /= n .or. size(des_w) /= n) error stop 'kessler_driver: the table is not of the length asked for'
  tw = table_w
  dw = des_w
end subroutine

! K_cycle_in = 0: fv_phys.F90:472-474, restated here because the lines are interleaved with the lookup of the tracer names
subroutine kessler_run(is, ie, js, je, ng, km, nq, dt, K_cycle_in, transport, sedi_w, sedi_heat, hydrostatic, moist_kappa, i_sphum, i_liq, i_rain, &
                       u, v, w, u_dt, v_dt, q, pt, dp, delz, pe, peln, pk, ps, rain) bind(C, name="kessler_run")
  use iso_c_binding
  use constants_mod, only: rvgas, rdgas
  use qs_tables_mod, only: qs_wat_init
  use kessler_standins_mod
  use kessler_cut_mod, only: K_warm_rain
  implicit none
  integer(c_int), value :: is, ie, js, je, ng, km, nq, K_cycle_in, transport, sedi_w, sedi_heat, hydrostatic, moist_kappa, i_sphum, i_liq, i_rain
  real(c_double), value :: dt
  real(c_double) :: u(is-ng:ie+ng, js-ng:je+ng, km), v(is-ng:ie+ng, js-ng:je+ng, km), w(is-ng:ie+ng, js-ng:je+ng, km)
  real(c_double) :: u_dt(is-ng:ie+ng, js-ng:je+ng, km), v_dt(is-ng:ie+ng, js-ng:je+ng, km), q(is-ng:ie+ng, js-ng:je+ng, km, nq)
  real(c_double) :: pt(is-ng:ie+ng, js-ng:je+ng, km), dp(is-ng:ie+ng, js-ng:je+ng, km), delz(is:ie, js:je, km)
  real(c_double) :: pe(is-1:ie+1, km+1, js-1:je+1), peln(is:ie, km+1, js:je), pk(is:ie, js:je, km+1), ps(is-ng:ie+ng, js-ng:je+ng)
  real(c_double) :: rain(is:ie, js:je)
  type(time_type) :: Time
  real(c_double) :: zvir
  call qs_wat_init
  K_sedi_transport = transport /= 0
  do_K_sedi_w = sedi_w /= 0
  do_K_sedi_heat = sedi_heat /= 0
  sphum = i_sphum
  liq_wat = i_liq
  rainwat = i_rain
  K_cycle = K_cycle_in
  if (K_cycle .eq. 0) K_cycle = max(1, nint(dt/30.))
  zvir = rvgas/rdgas - 1.
  call K_warm_rain(dt, is, ie, js, je, ng, km, nq, zvir, u, v, w, u_dt, v_dt, q, pt, dp, delz, pe, peln, pk, ps, rain, Time, &
                   hydrostatic /= 0, moist_kappa /= 0)
end subroutine
