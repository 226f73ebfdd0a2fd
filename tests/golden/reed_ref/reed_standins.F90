! Stand-ins for what the cuts of driver/solo/fv_phys.F90 that tests/golden/make_reed_golden.py compiles (reed_sim_physics, its column
! loop, DCMIP2016_terminator_advance) take from constants_mod, gfdl_mp_mod, field_manager_mod, tracer_manager_mod and from fv_phys_mod's
! own namelist: the constants with the reference's values (GFDL constants, gfdl_mp.F90:137), the two tracer names the terminator
! looks up, and its namelist switch.
module reed_standins_mod
  implicit none
  public
  integer, parameter :: r8_kind = selected_real_kind(15)
  real(r8_kind), parameter :: pi_8 = 3.14159265358979323846_r8_kind
  real(r8_kind), parameter :: radius = 6.3712e6_r8_kind
  real(r8_kind), parameter :: omega = 7.2921e-5_r8_kind
  real, parameter :: pi = pi_8
  real, parameter :: grav = 9.80, rdgas = 287.04, rvgas = 461.50, kappa = 2.0/7.0
  real, parameter :: cp_air = rdgas/kappa, cp_vapor = 4.0*rvgas, hlv = 2.500e6
  real, parameter :: c_liq = 4.218e3
  integer, parameter :: MODEL_ATMOS = 1
  logical :: term_fill_negative = .false.
contains
  integer function get_tracer_index(model, name)
    integer, intent(in) :: model
    character(len=*), intent(in) :: name
    get_tracer_index = -1
    if (name == 'Cl') get_tracer_index = 1
    if (name == 'Cl2') get_tracer_index = 2
    if (get_tracer_index < 0) error stop 'reed_standins: unknown tracer'
  end function
end module reed_standins_mod
