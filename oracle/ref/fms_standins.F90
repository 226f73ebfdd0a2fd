!> Stand-ins for the modules of the FMS library (and two of the reference's own tools/ modules) that the reference's
!> hot-path sources `use`.  TEST INFRASTRUCTURE ONLY: with these, oracle/Makefile compiles the reference's model/fv_arrays,
!> tp_core, a2b_edge, sw_core, nh_utils, nh_core, fv_fill and fv_operators .F90 where they lie, unmodified, into
!> oracle/_ref/libfv3ref.so (git-ignored), which tests/ref_lib.py loads.
!>
!> Everything here is this project's own text.  Derived types are empty: the pinned routines never touch them.  A routine
!> that cannot be honest without the real library (halo exchange, corner fill across faces, great-circle distances of the
!> grid generator) stops with a message; it never returns silently.  A pinned case therefore never reaches one.
!>
!> constants_mod carries the values the project itself uses (gfdl_atmos_cubed_sphere_amd/lib.py: GRAV, RDGAS, KAPPA,
!> CP_AIR = RDGAS / KAPPA; cubed_sphere.py: RADIUS, OMEGA).  They are INPUTS of the comparison -- the oracle and the kernels
!> receive the same numbers as arguments -- not something the comparison pins.

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
  real(r8_kind), parameter :: grav   = 9.80_r8_kind
  real(r8_kind), parameter :: rdgas  = 287.04_r8_kind
  real(r8_kind), parameter :: kappa  = 2.0_r8_kind / 7.0_r8_kind
  real(r8_kind), parameter :: cp_air = rdgas / kappa
  real(r8_kind), parameter :: pi_8   = 3.14159265358979323846_r8_kind
  real(r8_kind), parameter :: radius = 6.3712e6_r8_kind
  real(r8_kind), parameter :: omega  = 7.2921e-5_r8_kind
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
  end function mpp_pe
  subroutine mpp_error(level, message)
    integer, intent(in) :: level
    character(len=*), intent(in) :: message
    write(*, '(a)') 'fms_standins mpp_error: ' // trim(message)
    if (level == FATAL) error stop 'fms_standins: mpp_error(FATAL)'
  end subroutine mpp_error
  subroutine mpp_broadcast_stop(x, n, from_pe)
    real, intent(inout) :: x(*)
    integer, intent(in) :: n, from_pe
    error stop 'fms_standins: mpp_broadcast is not available (no message passing in the reference library)'
  end subroutine mpp_broadcast_stop
end module mpp_mod

module mpp_domains_mod
  implicit none
  public
  type domain2d
    integer :: unused = 0
  end type domain2d
  interface mpp_update_domains
    module procedure mpp_update_domains_2d_stop
    module procedure mpp_update_domains_3d_stop
  end interface
contains
  subroutine mpp_update_domains_2d_stop(field, domain, whalo, ehalo, shalo, nhalo)
    real, intent(inout) :: field(:, :)
    type(domain2d), intent(inout) :: domain
    integer, intent(in), optional :: whalo, ehalo, shalo, nhalo
    error stop 'fms_standins: mpp_update_domains is not available (no halo exchange in the reference library)'
  end subroutine mpp_update_domains_2d_stop
  subroutine mpp_update_domains_3d_stop(field, domain, whalo, ehalo, shalo, nhalo)
    real, intent(inout) :: field(:, :, :)
    type(domain2d), intent(inout) :: domain
    integer, intent(in), optional :: whalo, ehalo, shalo, nhalo
    error stop 'fms_standins: mpp_update_domains is not available (no halo exchange in the reference library)'
  end subroutine mpp_update_domains_3d_stop
end module mpp_domains_mod

module fms2_io_mod
  implicit none
  public
  type FmsNetcdfFile_t
    integer :: unused = 0
  end type FmsNetcdfFile_t
  type FmsNetcdfDomainFile_t
    integer :: unused = 0
  end type FmsNetcdfDomainFile_t
end module fms2_io_mod

module time_manager_mod
  implicit none
  public
  type time_type
    integer :: unused = 0
  end type time_type
end module time_manager_mod

module horiz_interp_type_mod
  implicit none
  public
  type horiz_interp_type
    integer :: unused = 0
  end type horiz_interp_type
end module horiz_interp_type_mod

!> tools/fv_grid_utils.F90 of the reference needs the whole grid generator; the hot path takes one constant and one function.
module fv_grid_utils_mod
  use platform_mod, only: r8_kind
  implicit none
  public
  real, parameter :: big_number = 1.e8
contains
  real(r8_kind) function great_circle_dist(q1, q2, radius)
    real(r8_kind), intent(in) :: q1(2), q2(2)
    real(r8_kind), intent(in), optional :: radius
    great_circle_dist = 0.
    error stop 'fms_standins: great_circle_dist is not available (a2b_ord4 at a cube corner is not pinned)'
  end function great_circle_dist
end module fv_grid_utils_mod

!> tools/fv_mp_mod.F90 of the reference is the message-passing layer; d_sw names its corner fill for nord > 0 at a cube corner.
module fv_mp_mod
  implicit none
  public
  integer, parameter :: XDir = 1, YDir = 2
  interface fill_corners
    module procedure fill_corners_scalar_stop
    module procedure fill_corners_vector_stop
  end interface
contains
  subroutine fill_corners_scalar_stop(q, npx, npy, FILL, AGRID, BGRID)
    real, intent(inout) :: q(:, :)
    integer, intent(in) :: npx, npy, FILL
    logical, intent(in), optional :: AGRID, BGRID
    error stop 'fms_standins: fill_corners is not available (d_sw with nord > 0 at a cube corner is not pinned)'
  end subroutine fill_corners_scalar_stop
  subroutine fill_corners_vector_stop(x, y, npx, npy, VECTOR, AGRID, BGRID, CGRID, DGRID)
    real, intent(inout) :: x(:, :), y(:, :)
    integer, intent(in) :: npx, npy
    logical, intent(in), optional :: VECTOR, AGRID, BGRID, CGRID, DGRID
    error stop 'fms_standins: fill_corners is not available (d_sw with nord > 0 at a cube corner is not pinned)'
  end subroutine fill_corners_vector_stop
end module fv_mp_mod
