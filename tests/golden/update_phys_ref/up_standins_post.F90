! Stand-ins for the modules model/fv_update_phys.F90 uses that themselves need fv_arrays_mod: compiled after the reference's
! fv_arrays.F90.  The recorded calls reach none of them but prt_maxmin's absence (fv_debug is off): they stop with a message.
module boundary_mod
  implicit none
  public
contains
  subroutine nested_grid_BC()
    error stop 'up_standins: nested_grid_BC is not available'
  end subroutine
  subroutine extrapolation_BC()
    error stop 'up_standins: extrapolation_BC is not available'
  end subroutine
end module
module fv_diagnostics_mod
  implicit none
  public
contains
  subroutine prt_maxmin(qname, q, is, ie, js, je, n_g, km, fac)
    character(len=*), intent(in) :: qname
    real, intent(in) :: q(*)
    integer, intent(in) :: is, ie, js, je, n_g, km
    real, intent(in) :: fac
    error stop 'up_standins: prt_maxmin is not available'
  end subroutine
  subroutine range_check(qname, q, is, ie, js, je, n_g, km, pos, q_low, q_hi, bad_range, Time)
    use time_manager_mod, only: time_type
    character(len=*), intent(in) :: qname
    real, intent(in) :: q(*), pos(*)
    integer, intent(in) :: is, ie, js, je, n_g, km
    real, intent(in) :: q_low, q_hi
    logical, intent(out), optional :: bad_range
    type(time_type), intent(in), optional :: Time
    error stop 'up_standins: range_check is not available'
  end subroutine
  elemental real function Mw_air(q)
    real, intent(in) :: q
    Mw_air = 0.
    error stop 'up_standins: Mw_air is not available (adj_mass_vmr = 2 is not recorded)'
  end function
end module
module fv_nwp_nudge_mod
  implicit none
  public
contains
  subroutine fv_nwp_nudge(Time, dt, npx, npy, npz, ps_dt, u_dt, v_dt, t_dt, q_dt, zvir, ak, bk, ts, ps, delp, ua, va, pt, nwat, q, phis, gridstruct, bd, domain)
    use time_manager_mod, only: time_type
    use fv_arrays_mod, only: fv_grid_type, fv_grid_bounds_type
    use mpp_domains_mod, only: domain2d
    type(time_type), intent(in) :: Time
    real, intent(in) :: dt, zvir
    integer, intent(in) :: npx, npy, npz, nwat
    real :: ps_dt(*), u_dt(*), v_dt(*), t_dt(*), q_dt(*), ak(*), bk(*), ts(*), ps(*), delp(*), ua(*), va(*), pt(*), q(*), phis(*)
    type(fv_grid_type) :: gridstruct
    type(fv_grid_bounds_type) :: bd
    type(domain2d) :: domain
    error stop 'up_standins: fv_nwp_nudge is not available'
  end subroutine
end module
module fv_nesting_mod
  implicit none
  public
contains
  subroutine set_physics_BCs(ps, u_dt, v_dt, flagstruct, gridstruct, neststruct, npx, npy, npz, ng, ak, bk, bd)
    use fv_arrays_mod, only: fv_grid_type, fv_grid_bounds_type, fv_flags_type, fv_nest_type
    real :: ps(*), u_dt(*), v_dt(*), ak(*), bk(*)
    type(fv_flags_type) :: flagstruct
    type(fv_grid_type) :: gridstruct
    type(fv_nest_type) :: neststruct
    integer :: npx, npy, npz, ng
    type(fv_grid_bounds_type) :: bd
    error stop 'up_standins: set_physics_BCs is not available'
  end subroutine
end module
