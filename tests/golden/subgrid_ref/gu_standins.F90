! Stand-ins for the modules model/fv_arrays.F90 and model/fv_grid_utils.F90 use, so that both reference files compile unmodified from
! where they lie (tests/golden/make_subgrid_golden.py).  update_dwinds_phys reaches none of the routines below: whatever cannot be
! honest without the real library stops with a message.
module platform_mod
  implicit none
  public
  integer, parameter :: r8_kind = selected_real_kind(15, 307)
  integer, parameter :: r4_kind = selected_real_kind(6, 37)
end module platform_mod

module constants_mod
  use platform_mod, only: r8_kind
  implicit none
  public
  real(r8_kind), parameter :: pi_8 = 3.14159265358979323846_r8_kind
  real(r8_kind), parameter :: radius = 6.3712e6_r8_kind
  real(r8_kind), parameter :: omega = 7.2921e-5_r8_kind
  real(r8_kind), parameter :: grav = 9.80_r8_kind
end module constants_mod

module mpp_mod
  implicit none
  public
  integer, parameter :: NOTE = 0, WARNING = 1, FATAL = 2
  interface mpp_broadcast
    module procedure mpp_broadcast_stop
  end interface
contains
  integer function mpp_pe()
    mpp_pe = 0
  end function
  subroutine mpp_error(level, message)
    integer, intent(in) :: level
    character(len=*), intent(in) :: message
    write(*, '(a)') 'gu_standins mpp_error: ' // trim(message)
    if (level == FATAL) error stop 'gu_standins: mpp_error(FATAL)'
  end subroutine
  subroutine mpp_broadcast_stop(x, n, from_pe)
    real, intent(inout) :: x(*)
    integer, intent(in) :: n, from_pe
    error stop 'gu_standins: mpp_broadcast is not available'
  end subroutine
end module mpp_mod

module mpp_parameter_mod
  implicit none
  public
  integer, parameter :: AGRID = 1, CGRID_NE = 2, CORNER = 3, SCALAR_PAIR = 4
end module mpp_parameter_mod

module mpp_domains_mod
  implicit none
  public
  integer, parameter :: DGRID_NE = 5, BITWISE_EXACT_SUM = 1, BITWISE_EFP_SUM = 2
  type domain2d
    integer :: unused = 0
  end type domain2d
  interface mpp_update_domains
    module procedure upd_2d, upd_3d, upd_2dv, upd_3dv
  end interface
contains
  subroutine upd_2d(field, domain, whalo, ehalo, shalo, nhalo, complete)
    real, intent(inout) :: field(:, :)
    type(domain2d), intent(inout) :: domain
    integer, intent(in), optional :: whalo, ehalo, shalo, nhalo
    logical, intent(in), optional :: complete
    error stop 'gu_standins: mpp_update_domains is not available (no halo exchange)'
  end subroutine
  subroutine upd_3d(field, domain, whalo, ehalo, shalo, nhalo, complete)
    real, intent(inout) :: field(:, :, :)
    type(domain2d), intent(inout) :: domain
    integer, intent(in), optional :: whalo, ehalo, shalo, nhalo
    logical, intent(in), optional :: complete
    error stop 'gu_standins: mpp_update_domains is not available (no halo exchange)'
  end subroutine
  subroutine upd_2dv(fx, fy, domain, flags, gridtype, complete)
    real, intent(inout) :: fx(:, :), fy(:, :)
    type(domain2d), intent(inout) :: domain
    integer, intent(in), optional :: flags, gridtype
    logical, intent(in), optional :: complete
    error stop 'gu_standins: mpp_update_domains is not available (no halo exchange)'
  end subroutine
  subroutine upd_3dv(fx, fy, domain, flags, gridtype, complete)
    real, intent(inout) :: fx(:, :, :), fy(:, :, :)
    type(domain2d), intent(inout) :: domain
    integer, intent(in), optional :: flags, gridtype
    logical, intent(in), optional :: complete
    error stop 'gu_standins: mpp_update_domains is not available (no halo exchange)'
  end subroutine
  real function mpp_global_sum(domain, field, flags)
    type(domain2d), intent(in) :: domain
    real, intent(in) :: field(:, :)
    integer, intent(in), optional :: flags
    mpp_global_sum = 0.
    error stop 'gu_standins: mpp_global_sum is not available'
  end function
end module mpp_domains_mod

module fms2_io_mod
  implicit none
  public
  type FmsNetcdfFile_t
    integer :: unused = 0
  end type
  type FmsNetcdfDomainFile_t
    integer :: unused = 0
  end type
end module fms2_io_mod

module time_manager_mod
  implicit none
  public
  type time_type
    integer :: unused = 0
  end type
end module time_manager_mod

module horiz_interp_type_mod
  implicit none
  public
  type horiz_interp_type
    integer :: unused = 0
  end type
end module horiz_interp_type_mod

module external_sst_mod
  implicit none
  public
  integer :: i_sst = -1, j_sst = -1
  real, allocatable, dimension(:, :) :: sst_ncep, sst_anom
end module external_sst_mod

module fv_eta_mod
  implicit none
  public
contains
  subroutine set_eta(km, ks, ptop, ak, bk, npz_type, fv_eta_file)
    integer, intent(in) :: km
    integer, intent(out) :: ks
    real, intent(out) :: ptop, ak(km+1), bk(km+1)
    character(*), intent(in) :: npz_type, fv_eta_file
    error stop 'gu_standins: set_eta is not available'
  end subroutine
end module fv_eta_mod

module fv_timing_mod
  implicit none
  public
contains
  subroutine timing_on(name)
    character(len=*), intent(in) :: name
  end subroutine
  subroutine timing_off(name)
    character(len=*), intent(in) :: name
  end subroutine
end module fv_timing_mod

module fv_mp_mod
  implicit none
  public
  integer, parameter :: XDir = 1, YDir = 2
  interface fill_corners
    module procedure fill_corners_scalar_stop, fill_corners_vector_stop
  end interface
contains
  logical function is_master()
    is_master = .true.
  end function
  subroutine mp_reduce_sum(x)
    real, intent(inout) :: x
  end subroutine
  subroutine mp_reduce_min(x)
    real, intent(inout) :: x
  end subroutine
  subroutine mp_reduce_max(x)
    real, intent(inout) :: x
  end subroutine
  subroutine fill_corners_scalar_stop(q, npx, npy, FILL, AGRID, BGRID)
    real, intent(inout) :: q(:, :)
    integer, intent(in) :: npx, npy, FILL
    logical, intent(in), optional :: AGRID, BGRID
    error stop 'gu_standins: fill_corners is not available'
  end subroutine
  subroutine fill_corners_vector_stop(x, y, npx, npy, VECTOR, AGRID, BGRID, CGRID, DGRID)
    real, intent(inout) :: x(:, :), y(:, :)
    integer, intent(in) :: npx, npy
    logical, intent(in), optional :: VECTOR, AGRID, BGRID, CGRID, DGRID
    error stop 'gu_standins: fill_corners is not available'
  end subroutine
end module fv_mp_mod
