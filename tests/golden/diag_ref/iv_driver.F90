! bind(C) driver of the reference's interpolate_vertical for tests/golden/make_diag_golden.py.  iv_ref_mod is formed by the generator in
! its temporary directory: the routine's own lines of tools/fv_diagnostics.F90 between `contains` and `end module`, nothing else.
subroutine iv_run(is, ie, js, je, km, plev, peln, a3, a2) bind(C, name="iv_run")
  use iso_c_binding, only: c_int, c_double
  use iv_ref_mod, only: interpolate_vertical
  implicit none
  integer(c_int), value :: is, ie, js, je, km
  real(c_double), value :: plev
  real(c_double), intent(in) :: peln(is:ie, km+1, js:je), a3(is:ie, js:je, km)
  real(c_double), intent(out) :: a2(is:ie, js:je)
  call interpolate_vertical(is, ie, js, je, km, plev, peln, a3, a2)
end subroutine iv_run
