! Stand-ins for what driver/solo/qs_tables.F90 (compiled unmodified) and the cuts of driver/solo/fv_phys.F90 that
! tests/golden/make_kessler_golden.py compiles (K_warm_rain, kessler_imp) take from constants_mod, gfdl_mp_mod, time_manager_mod,
! diag_manager_mod, fv_diagnostics_mod and from fv_phys_mod's own module variables: the constants with the reference's values (GFDL
! constants, gfdl_mp.F90:137), the Kessler namelist switches, the three tracer indices and the diagnostic id that is never
! registered.
module constants_mod
  implicit none
  public
  real, parameter :: grav = 9.80, rdgas = 287.04, rvgas = 461.50, kappa = 2.0/7.0
  real, parameter :: cp_air = rdgas/kappa, cp_vapor = 4.0*rvgas, hlv = 2.500e6
end module constants_mod

module gfdl_mp_mod
  implicit none
  public
  real, parameter :: c_liq = 4.218e3
end module gfdl_mp_mod

module kessler_standins_mod
  implicit none
  public
  type time_type
    integer :: unused = 0
  end type
  logical :: K_sedi_transport = .false., do_K_sedi_w = .false., do_K_sedi_heat = .false.
  integer :: K_cycle = 0
  integer :: sphum = 1, liq_wat = 2, rainwat = 3
  integer :: id_vr_k = 0
contains
  logical function send_data(id, field, time)
    integer, intent(in) :: id
    real, intent(in) :: field(:, :, :)
    type(time_type), intent(in) :: time
    send_data = .false.
    error stop 'kessler_standins: send_data is not available (id_vr_k is never registered)'
  end function
  subroutine prt_maxmin(qname, q, is, ie, js, je, n_g, km, fac)
    character(len=*), intent(in) :: qname
    real, intent(in) :: q(*)
    integer, intent(in) :: is, ie, js, je, n_g, km
    real, intent(in) :: fac
    error stop 'kessler_standins: prt_maxmin is not available'
  end subroutine
end module kessler_standins_mod
