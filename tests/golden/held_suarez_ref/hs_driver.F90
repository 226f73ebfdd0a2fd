! bind(C) drivers of the reference's Held_Suarez_Tend and age_of_air (driver/solo/hswf.F90:41, :209), called through ctypes by
! tests/golden/make_held_suarez_golden.py.  radius: fv_arrays_mod's module variable, set as the small-earth scaling sets it.  The
! arguments the routine never reads (u, v, q, q_dt, delz, phis, ak, bk) are zeros of their declared shapes.
subroutine hs_run(is, ie, js, je, ng, npz, pdt, strat, zurita, rd_zur, radius_in, agrid, pt, pe, delp, peln, pkz, ua, va, u_dt, v_dt, t_dt) &
    bind(C, name="hs_run")
  use iso_c_binding
  use fv_arrays_mod, only: radius
  use time_manager_mod, only: time_type
  use hswf_mod, only: Held_Suarez_Tend
  implicit none
  integer(c_int), value :: is, ie, js, je, ng, npz, strat, zurita
  real(c_double), value :: pdt, rd_zur, radius_in
  real(c_double) :: agrid(is-ng:ie+ng, js-ng:je+ng, 2), pt(is-ng:ie+ng, js-ng:je+ng, npz), pe(is-1:ie+1, npz+1, js-1:je+1)
  real(c_double) :: delp(is-ng:ie+ng, js-ng:je+ng, npz), peln(is:ie, npz+1, js:je), pkz(is:ie, js:je, npz)
  real(c_double) :: ua(is-ng:ie+ng, js-ng:je+ng, npz), va(is-ng:ie+ng, js-ng:je+ng, npz)
  real(c_double) :: u_dt(is-ng:ie+ng, js-ng:je+ng, npz), v_dt(is-ng:ie+ng, js-ng:je+ng, npz), t_dt(is:ie, js:je, npz)
  real(c_double), allocatable :: u(:, :, :), v(:, :, :), q(:, :, :, :), q_dt(:, :, :, :), delz(:, :, :), phis(:, :), ak(:), bk(:)
  type(time_type) :: time
  real(c_double) :: keep
  allocate(u(is-ng:ie+ng, js-ng:je+1+ng, npz), v(is-ng:ie+1+ng, js-ng:je+ng, npz), q(is-ng:ie+ng, js-ng:je+ng, npz, 1))
  allocate(q_dt(is:ie, js:je, npz, 1), delz(is:ie, js:je, npz), phis(is-ng:ie+ng, js-ng:je+ng), ak(npz+1), bk(npz+1))
  u = 0.; v = 0.; q = 0.; q_dt = 0.; delz = 0.; phis = 0.; ak = 0.; bk = 0.
  keep = radius
  radius = radius_in
  call Held_Suarez_Tend(ie-is+2, je-js+2, npz, is, ie, js, je, ng, 1, u, v, pt, q, pe, delp, peln, pkz, pdt, ua, va, u_dt, v_dt, t_dt, q_dt, &
                        agrid, delz, phis, .true., ak, bk, 0, strat /= 0, zurita /= 0, rd_zur, .false., time, 0.0_c_double)
  radius = keep
  if (any(u /= 0.) .or. any(v /= 0.) .or. any(q /= 0.) .or. any(q_dt /= 0.) .or. any(delz /= 0.) .or. any(phis /= 0.)) &
    error stop 'hs_driver: Held_Suarez_Tend wrote an argument the library leaves out'
end subroutine

subroutine hs_age(is, ie, js, je, km, ng, time, pe, q) bind(C, name="hs_age")
  use iso_c_binding
  use hswf_mod, only: age_of_air
  implicit none
  integer(c_int), value :: is, ie, js, je, km, ng
  real(c_double), value :: time
  real(c_double) :: pe(is-1:ie+1, km+1, js-1:je+1), q(is-ng:ie+ng, js-ng:je+ng, km)
  call age_of_air(is, ie, js, je, km, ng, time, pe, q)
end subroutine

! the four latitude planes of fv3_grid_upload_lat in the expressions of hswf.F90:152, :180-184, from this compiler's SIN, COS, **:
! what --measure holds the host-formed table to
subroutine hs_lat_planes(n, lat, planes) bind(C, name="hs_lat_planes")
  use iso_c_binding
  implicit none
  integer(c_int), value :: n
  real(c_double), intent(in) :: lat(n)
  real(c_double), intent(out) :: planes(n, 4)
  real :: ty, tz, akap, p0, ap0k
  integer :: i
  ty = 60.0
  tz = 10.0
  akap = 2./7.
  p0 = 100000.
  ap0k = 1./p0**akap
  do i = 1, n
    planes(i, 1) = COS(lat(i))
    planes(i, 2) = ty*SIN(lat(i))*SIN(lat(i))
    planes(i, 3) = tz*( ap0k/akap )*COS(lat(i))*COS(lat(i))
    planes(i, 4) = COS(lat(i))**4.0
  enddo
end subroutine
