! Stand-ins for what driver/solo/hswf.F90 uses beyond tests/golden/update_phys_ref/up_standins.F90, compiled AFTER that file so that
! these module files are the ones the later sources see (tests/golden/make_held_suarez_golden.py): constants_mod with pi and RADIAN
! beside what up_standins.F90 has (the same values), time_manager_mod with get_date / get_time beside time_type, and
! diag_manager_mod's send_data.  Held_Suarez_Tend and age_of_air call none of the procedures: they stop with a message.
module constants_mod
  use platform_mod, only: r8_kind
  implicit none
  public
  real(r8_kind), parameter :: pi_8 = 3.14159265358979323846_r8_kind
  real(r8_kind), parameter :: radius = 6.3712e6_r8_kind
  real(r8_kind), parameter :: omega = 7.2921e-5_r8_kind
  real, parameter :: pi = pi_8, RADIAN = 180.0/pi
  real, parameter :: grav = 9.80, rdgas = 287.04, rvgas = 461.50, kappa = 2.0/7.0
  real, parameter :: cp_air = rdgas/kappa, cp_vapor = 4.0*rvgas, TFREEZE = 273.16, wtmair = 2.896440e1, wtmh2o = wtmair*(rdgas/rvgas)
end module constants_mod

module time_manager_mod
  implicit none
  public
  type time_type
    integer :: unused = 0
  end type
contains
  subroutine get_date(time, year, month, day, hour, minute, second)
    type(time_type), intent(in) :: time
    integer, intent(out) :: year, month, day, hour, minute, second
    year = 0; month = 0; day = 0; hour = 0; minute = 0; second = 0
    error stop 'hs_standins: get_date is not available'
  end subroutine
  subroutine get_time(time, seconds, days)
    type(time_type), intent(in) :: time
    integer, intent(out) :: seconds
    integer, intent(out), optional :: days
    seconds = 0
    if (present(days)) days = 0
    error stop 'hs_standins: get_time is not available'
  end subroutine
end module time_manager_mod

module diag_manager_mod
  implicit none
  public
  interface send_data
    module procedure send_data_2d, send_data_3d
  end interface
contains
  logical function send_data_2d(id, field, time)
    use time_manager_mod, only: time_type
    integer, intent(in) :: id
    real, intent(in) :: field(:, :)
    type(time_type), intent(in), optional :: time
    send_data_2d = .false.
    error stop 'hs_standins: send_data is not available'
  end function
  logical function send_data_3d(id, field, time)
    use time_manager_mod, only: time_type
    integer, intent(in) :: id
    real, intent(in) :: field(:, :, :)
    type(time_type), intent(in), optional :: time
    send_data_3d = .false.
    error stop 'hs_standins: send_data is not available'
  end function
end module diag_manager_mod
