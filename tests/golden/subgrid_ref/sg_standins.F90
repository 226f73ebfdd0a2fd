! Stand-ins for the modules model/fv_sg.F90 uses, so that the reference file compiles unmodified from where it lies
! (tests/golden/make_subgrid_golden.py).  fv_sg_SHiELD takes constants and tracer indices from them and nothing else: the
! saturation routines are never reached from it and stop if they are.
module constants_mod
  implicit none
  public
  real, parameter :: grav = 9.80
  real, parameter :: rdgas = 287.04
  real, parameter :: rvgas = 461.50
  real, parameter :: kappa = 2.0 / 7.0
  real, parameter :: cp_air = rdgas / kappa
  real, parameter :: cp_vapor = 4.0 * rvgas
  real, parameter :: hlv = 2.500e6
  real, parameter :: hlf = 3.34e5
end module constants_mod

module field_manager_mod
  implicit none
  public
  integer, parameter :: MODEL_ATMOS = 1
end module field_manager_mod

module tracer_manager_mod
  implicit none
  public
  ! sphum, liq_wat, rainwat, ice_wat, snowwat, graupel, cld_amt: set by the driver before a call
  integer, save :: sg_index(7) = 0
contains
  integer function get_tracer_index(model, name)
    integer, intent(in) :: model
    character(len=*), intent(in) :: name
    select case (trim(name))
    case ('sphum');   get_tracer_index = sg_index(1)
    case ('liq_wat'); get_tracer_index = sg_index(2)
    case ('rainwat'); get_tracer_index = sg_index(3)
    case ('ice_wat'); get_tracer_index = sg_index(4)
    case ('snowwat'); get_tracer_index = sg_index(5)
    case ('graupel'); get_tracer_index = sg_index(6)
    case ('cld_amt'); get_tracer_index = sg_index(7)
    case default;     get_tracer_index = -1
    end select
  end function
end module tracer_manager_mod

module gfdl_mp_mod
  implicit none
  public
  real, parameter :: c_ice = 2.106e3   ! model/gfdl_mp.F90:136
  real, parameter :: c_liq = 4.218e3   ! model/gfdl_mp.F90:137
  interface wqs
    module procedure wqs3, wqs4
  end interface
contains
  real function wqs3(ta, den, dqdt)
    real, intent(in) :: ta, den
    real, intent(out) :: dqdt
    stop 'sg_standins: wqs is not part of fv_sg_SHiELD'
  end function
  real function wqs4(ta, pa, qv, dqdt)
    real, intent(in) :: ta, pa, qv
    real, intent(out) :: dqdt
    stop 'sg_standins: wqs is not part of fv_sg_SHiELD'
  end function
  subroutine mqs3d(im, km, ks, ta, pa, qv, qs, dqdt)
    integer, intent(in) :: im, km, ks
    real, intent(in) :: ta(im, ks:km), pa(im, ks:km), qv(im, ks:km)
    real, intent(out) :: qs(im, ks:km)
    real, intent(out), optional :: dqdt(im, ks:km)
    stop 'sg_standins: mqs3d is not part of fv_sg_SHiELD'
  end subroutine
end module gfdl_mp_mod

module fv_mp_mod
  implicit none
  public
contains
  logical function is_master()
    is_master = .true.
  end function
  subroutine mp_reduce_min(x)
    real, intent(inout) :: x
  end subroutine
end module fv_mp_mod

module mpp_mod
  implicit none
  public
contains
  integer function mpp_pe()
    mpp_pe = 0
  end function
end module mpp_mod
