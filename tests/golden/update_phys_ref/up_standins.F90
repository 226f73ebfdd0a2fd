! Stand-ins for the modules that tools/fv_eta.F90, model/fv_arrays.F90, model/fv_grid_utils.F90, model/fv_thermodynamics.F90 and
! model/fv_update_phys.F90 use, so that the five reference files compile unmodified from where they lie
! (tests/golden/make_update_phys_golden.py; subgrid_ref/up_standins.F90 is where the first half comes from).  fv_update_phys is run on
! a one-rank doubly periodic domain (grid_type 4), where a periodic fill IS start_group_halo_update; the tracer manager answers from
! what the driver hands it.  Whatever cannot be honest without the real library stops with a message.
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
  real, parameter :: grav = 9.80, rdgas = 287.04, rvgas = 461.50, kappa = 2.0/7.0
  real, parameter :: cp_air = rdgas/kappa, cp_vapor = 4.0*rvgas, TFREEZE = 273.16, wtmair = 2.896440e1, wtmh2o = wtmair*(rdgas/rvgas)
end module constants_mod

module mpp_mod
  implicit none
  public
  integer, parameter :: NOTE = 0, WARNING = 1, FATAL = 2
  character(len=8) :: input_nml_file(1) = ''
  interface mpp_broadcast
    module procedure mpp_broadcast_stop
  end interface
contains
  integer function mpp_pe()
    mpp_pe = 0
  end function
  integer function mpp_root_pe()
    mpp_root_pe = 0
  end function
  subroutine mpp_error(level, message)
    integer, intent(in) :: level
    character(len=*), intent(in) :: message
    write(*, '(a)') 'up_standins mpp_error: ' // trim(message)
    if (level == FATAL) error stop 'up_standins: mpp_error(FATAL)'
  end subroutine
  subroutine mpp_broadcast_stop(x, n, from_pe)
    real, intent(inout) :: x(*)
    integer, intent(in) :: n, from_pe
    error stop 'up_standins: mpp_broadcast is not available'
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
    error stop 'up_standins: mpp_update_domains is not available (no halo exchange)'
  end subroutine
  subroutine upd_3d(field, domain, whalo, ehalo, shalo, nhalo, complete)
    real, intent(inout) :: field(:, :, :)
    type(domain2d), intent(inout) :: domain
    integer, intent(in), optional :: whalo, ehalo, shalo, nhalo
    logical, intent(in), optional :: complete
    error stop 'up_standins: mpp_update_domains is not available (no halo exchange)'
  end subroutine
  subroutine upd_2dv(fx, fy, domain, flags, gridtype, complete)
    real, intent(inout) :: fx(:, :), fy(:, :)
    type(domain2d), intent(inout) :: domain
    integer, intent(in), optional :: flags, gridtype
    logical, intent(in), optional :: complete
    error stop 'up_standins: mpp_update_domains is not available (no halo exchange)'
  end subroutine
  subroutine upd_3dv(fx, fy, domain, flags, gridtype, complete)
    real, intent(inout) :: fx(:, :, :), fy(:, :, :)
    type(domain2d), intent(inout) :: domain
    integer, intent(in), optional :: flags, gridtype
    logical, intent(in), optional :: complete
    error stop 'up_standins: mpp_update_domains is not available (no halo exchange)'
  end subroutine
  real function mpp_global_sum(domain, field, flags)
    type(domain2d), intent(in) :: domain
    real, intent(in) :: field(:, :)
    integer, intent(in), optional :: flags
    mpp_global_sum = 0.
    error stop 'up_standins: mpp_global_sum is not available'
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
contains
  subroutine ascii_read(f, c)
    character(len=*), intent(in) :: f
    character(len=:), allocatable, intent(inout) :: c(:)
    error stop 'up_standins: ascii_read is not available'
  end subroutine
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
  type group_halo_update_type
    integer :: unused = 0
  end type
  integer, save :: up_ng = 0   ! the halo width of the A-grid arrays, set by the driver
  interface fill_corners
    module procedure fill_corners_scalar_stop, fill_corners_vector_stop
  end interface
contains
  subroutine start_group_halo_update(group, f, domain, whalo, ehalo, shalo, nhalo, complete)
    use mpp_domains_mod, only: domain2d
    type(group_halo_update_type), intent(inout) :: group
    real, intent(inout) :: f(:, :, :)
    type(domain2d), intent(inout) :: domain
    integer, intent(in), optional :: whalo, ehalo, shalo, nhalo
    logical, intent(in), optional :: complete
    ! one rank, doubly periodic: every halo cell within the asked width from the opposite side of the compute domain
    integer :: i, j, k, nx, ny, w, si, sj
    if (up_ng <= 0) error stop 'up_standins: start_group_halo_update without up_ng'
    nx = size(f, 1) - 2*up_ng
    ny = size(f, 2) - 2*up_ng
    w = up_ng
    if (present(whalo)) then
      if (.not. (present(ehalo) .and. present(shalo) .and. present(nhalo))) error stop 'up_standins: a halo width is missing'
      if (ehalo /= whalo .or. shalo /= whalo .or. nhalo /= whalo) error stop 'up_standins: unequal halo widths'
      w = whalo
    endif
    if (w > up_ng .or. w > nx .or. w > ny) error stop 'up_standins: halo wider than the array has or the domain fills'
    do k = 1, size(f, 3)
      do j = up_ng + 1 - w, up_ng + ny + w
        do i = up_ng + 1 - w, up_ng + nx + w
          if (i > up_ng .and. i <= up_ng + nx .and. j > up_ng .and. j <= up_ng + ny) cycle
          si = up_ng + 1 + modulo(i - up_ng - 1, nx)
          sj = up_ng + 1 + modulo(j - up_ng - 1, ny)
          f(i, j, k) = f(si, sj, k)
        enddo
      enddo
    enddo
  end subroutine
  subroutine complete_group_halo_update(group, domain)
    use mpp_domains_mod, only: domain2d
    type(group_halo_update_type), intent(inout) :: group
    type(domain2d), intent(inout) :: domain
  end subroutine
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
    error stop 'up_standins: fill_corners is not available'
  end subroutine
  subroutine fill_corners_vector_stop(x, y, npx, npy, VECTOR, AGRID, BGRID, CGRID, DGRID)
    real, intent(inout) :: x(:, :), y(:, :)
    integer, intent(in) :: npx, npy
    logical, intent(in), optional :: VECTOR, AGRID, BGRID, CGRID, DGRID
    error stop 'up_standins: fill_corners is not available'
  end subroutine
end module fv_mp_mod

module fms_mod
  implicit none
  public
  integer, parameter :: FATAL = 2
contains
  integer function check_nml_error(ios, name)
    integer, intent(in) :: ios
    character(len=*), intent(in) :: name
    check_nml_error = 0
  end function
  subroutine error_mesg(a, b, level)
    character(len=*), intent(in) :: a, b
    integer, intent(in) :: level
    write(*, '(a)') 'up_standins error_mesg: ' // trim(a) // ': ' // trim(b)
    error stop 'up_standins: error_mesg'
  end subroutine
end module fms_mod

module field_manager_mod
  implicit none
  public
  integer, parameter :: MODEL_ATMOS = 1
end module

module tracer_manager_mod
  implicit none
  public
  ! set by the driver: the 1-based indices of sphum, liq_wat, ice_wat, rainwat, snowwat, graupel, cld_amt, w_diff (absent: -1, what
  ! the real get_tracer_index returns, NO_TRACER) and the adjust_mass flag of every tracer
  character(len=8), parameter :: up_names(8) = (/'sphum   ', 'liq_wat ', 'ice_wat ', 'rainwat ', 'snowwat ', 'graupel ', 'cld_amt ', 'w_diff  '/)
  integer, save :: up_index(8) = -1
  logical, save :: up_adjust(64) = .true.
contains
  integer function get_tracer_index(model, name)
    integer, intent(in) :: model
    character(len=*), intent(in) :: name
    integer :: n
    get_tracer_index = -1
    do n = 1, 8
      if (trim(name) == trim(up_names(n))) then
        get_tracer_index = up_index(n)
        return
      endif
    enddo
    error stop 'up_standins: get_tracer_index of a name the driver does not know'
  end function
  logical function adjust_mass(model, n)
    integer, intent(in) :: model, n
    if (n < 1 .or. n > 64) error stop 'up_standins: adjust_mass of a tracer outside 1..64'
    adjust_mass = up_adjust(n)
  end function
  subroutine get_tracer_names(model, n, name, longname, units)
    integer, intent(in) :: model, n
    character(len=*), intent(out) :: name
    character(len=*), intent(out), optional :: longname, units
    error stop 'up_standins: get_tracer_names is not available (adj_mass_vmr > 0 is not recorded)'
  end subroutine
  logical function get_tracer_name(model, n, name)
    integer, intent(in) :: model, n
    character(len=*), intent(out) :: name
    get_tracer_name = .false.
    error stop 'up_standins: get_tracer_name is not available (fv_thermodynamics_init is not run)'
  end function
end module
module gfdl_mp_mod
  implicit none
  public
  real, parameter :: c_ice = 2.106e3, c_liq = 4.218e3
end module
module sat_vapor_pres_mod
  implicit none
  public
  integer, parameter :: tcmin = -160, tcmax = 100
end module
