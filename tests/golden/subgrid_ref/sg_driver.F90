! bind(C) driver of the reference's fv_sg_SHiELD (model/fv_sg.F90:76), called through ctypes by tests/golden/make_subgrid_golden.py
subroutine sg_run(is, ie, js, je, ng, km, nq, nqa, dt, fv_sg_adj, fv_sg_adj_weak, nwat, idx, hydrostatic, k_bot_full, &
                  delp, pe, peln, pkz, ta, qa, ua, va, w, delz, u_dt, v_dt) bind(C, name="sg_run")
  use iso_c_binding
  use fv_sg_mod, only: fv_sg_SHiELD
  use tracer_manager_mod, only: sg_index
  implicit none
  integer(c_int), value :: is, ie, js, je, ng, km, nq, nqa, fv_sg_adj, fv_sg_adj_weak, nwat, hydrostatic, k_bot_full
  real(c_double), value :: dt
  integer(c_int), intent(in) :: idx(7)
  real(c_double) :: delp(is-ng:ie+ng, js-ng:je+ng, km), ta(is-ng:ie+ng, js-ng:je+ng, km), ua(is-ng:ie+ng, js-ng:je+ng, km)
  real(c_double) :: va(is-ng:ie+ng, js-ng:je+ng, km), w(is-ng:ie+ng, js-ng:je+ng, km), qa(is-ng:ie+ng, js-ng:je+ng, km, nqa)
  real(c_double) :: u_dt(is-ng:ie+ng, js-ng:je+ng, km), v_dt(is-ng:ie+ng, js-ng:je+ng, km)
  real(c_double) :: pe(is-1:ie+1, km+1, js-1:je+1), peln(is:ie, km+1, js:je), pkz(is:ie, js:je, km), delz(is:ie, js:je, km)
  sg_index = idx
  ! qa is handed with its first nq tracers: the routine's dummy is qa(isd:ied, jsd:jed, km, nq)
  call fv_sg_SHiELD(is-ng, ie+ng, js-ng, je+ng, is, ie, js, je, km, nq, dt, fv_sg_adj, fv_sg_adj_weak, nwat, delp, pe, peln, pkz, &
                    ta, qa(:, :, :, 1:nq), ua, va, hydrostatic /= 0, w, delz, u_dt, v_dt, k_bot_full)
end subroutine
