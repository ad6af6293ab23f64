! srt_bindc.f90 -- Fortran-callable shim over the C ABI of libsrt_hip.so (include/srt.h).
!
! A Fortran program (e.g. a trimmed raytracer_driver) replaces its serial loop
!     do ... ; call raytracer_run(pos,time,vprel,...,pos0,dir0,w,dt0,...) ; write records ; end do
! (fortran/raytracer_driver.f95:1144-1232) by ONE call of srt_trace_batch over the whole ray file and one
! call of srt_write_ray_file.  Arrays are passed in Fortran's natural layout: pos0(3,nrays) is exactly the
! C layout pos0[nrays][3]; rows(SRT_ROW, slots, nrays) is rows[nrays][slots][SRT_ROW].
module srt_bindc
  use iso_c_binding
  implicit none
  integer, parameter :: SRT_ROW = 20, SRT_MAXSPEC = 4
  ! device layouts of the interp model (include/srt.h)
  integer(c_int), parameter :: SRT_INTERP_EXPANDED = 0, SRT_INTERP_NODES = 1, SRT_INTERP_AUTO = 2

  type, bind(C) :: srt_params
     real(c_double) :: dt0, dtmax, tmax, maxerr, minalt, del
     integer(c_int32_t) :: maxsteps, root, fixedstep, outputper, first_attempt_policy, refill_threshold, ray_order
  end type srt_params
  ! srt_damping_params of include/srt.h (the MATLAB post-processor matlab/damping/, SURVEY 8f-3)
  type, bind(C) :: srt_damping_params
     integer(c_int32_t) :: dist, mode, nres
     integer(c_int32_t) :: m(8)
     real(c_double) :: Ne_h, kT, tol
  end type srt_damping_params
  ! srt_surface of include/srt.h: kind 0 sphere, 1 dipole L-shell, 2 magnetic latitude (radians), 3 plane
  integer(c_int), parameter :: SRT_MAXSURF = 16
  type, bind(C) :: srt_surface
     integer(c_int32_t) :: kind, reserved
     real(c_double) :: p(4)
  end type srt_surface
  ! srt_bin_axis / srt_bin_params of include/srt.h: kind 0 .. 7 = x y z r rho L sinlat mlt; edges = c_loc of n + 1 doubles
  type, bind(C) :: srt_bin_axis
     integer(c_int32_t) :: kind, n
     type(c_ptr) :: edges
  end type srt_bin_axis
  type, bind(C) :: srt_bin_params
     integer(c_int32_t) :: naxes, nsub
     real(c_double) :: quantum
     type(srt_bin_axis) :: axis(3)
  end type srt_bin_params
  ! srt_observer of include/srt.h: a point in SM metres and its detection radius in metres
  integer(c_int), parameter :: SRT_MAXOBS = 65536
  type, bind(C) :: srt_observer
     real(c_double) :: x(3), radius
  end type srt_observer
  ! srt_segment: what one srt_trace_run_next hands out (valid until the next call on the run).  c_f_pointer turns the members
  ! into arrays: ray(nrays), offsets(nrays+1), rows(20, offsets(nrays+1)), nrows(nrays), stopcond(nrays)
  type, bind(C) :: srt_segment
     integer(c_int32_t) :: segment, reserved
     integer(c_int64_t) :: nrays
     type(c_ptr) :: ray, offsets, rows, nrows, stopcond
     integer(c_int64_t) :: accepted_steps
  end type srt_segment

  interface
     integer(c_int) function srt_init(device) bind(C, name="srt_init")
       import :: c_int
       integer(c_int), value :: device
     end function srt_init
     function srt_last_error() bind(C, name="srt_last_error")
       import :: c_ptr
       type(c_ptr) :: srt_last_error
     end function srt_last_error
     integer(c_int) function srt_model_create_ngo(configfile, yearday, msec, model) bind(C, name="srt_model_create_ngo")
       import :: c_int, c_char, c_ptr
       character(kind=c_char), dimension(*) :: configfile
       integer(c_int), value :: yearday, msec
       type(c_ptr) :: model
     end function srt_model_create_ngo
     integer(c_int) function srt_model_create_interp_file(gridfile, yearday, msec, model) &
          bind(C, name="srt_model_create_interp_file")
       import :: c_int, c_char, c_ptr
       character(kind=c_char), dimension(*) :: gridfile
       integer(c_int), value :: yearday, msec
       type(c_ptr) :: model
     end function srt_model_create_interp_file
     ! modelnum = 3 in a chosen device layout (SRT_INTERP_EXPANDED / _NODES / _AUTO above; include/srt.h): from a grid file,
     ! from host arrays F(nspec,nx,ny,nz) (derivs = c_null_ptr or the address of seven c_ptr to arrays of F's shape), from
     ! another handle; the layout a handle has (-1: not an interp model); and the two pure host functions on the sizes
     integer(c_int) function srt_model_create_interp_file_layout(gridfile, yearday, msec, layout, model) &
          bind(C, name="srt_model_create_interp_file_layout")
       import :: c_int, c_char, c_ptr
       character(kind=c_char), dimension(*) :: gridfile
       integer(c_int), value :: yearday, msec, layout
       type(c_ptr) :: model
     end function srt_model_create_interp_file_layout
     integer(c_int) function srt_model_create_interp_layout(nspec, nx, ny, nz, bounds, qs, ms, F, derivs, yearday, msec, &
          layout, model) bind(C, name="srt_model_create_interp_layout")
       import :: c_int, c_ptr, c_double
       integer(c_int), value :: nspec, nx, ny, nz, yearday, msec, layout
       real(c_double), intent(in) :: bounds(6), qs(*), ms(*), F(*)
       type(c_ptr), value :: derivs
       type(c_ptr) :: model
     end function srt_model_create_interp_layout
     integer(c_int) function srt_model_create_interp_from_model_layout(src, compder, nx, ny, nz, bounds, yearday, msec, &
          layout, model) bind(C, name="srt_model_create_interp_from_model_layout")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: src
       integer(c_int), value :: compder, nx, ny, nz, yearday, msec, layout
       real(c_double), intent(in) :: bounds(6)
       type(c_ptr) :: model
     end function srt_model_create_interp_from_model_layout
     integer(c_int) function srt_model_interp_layout(model) bind(C, name="srt_model_interp_layout")
       import :: c_int, c_ptr
       type(c_ptr), value :: model
     end function srt_model_interp_layout
     integer(c_int) function srt_interp_layout_bytes(nspec, nx, ny, nz, layout, table, peak) &
          bind(C, name="srt_interp_layout_bytes")
       import :: c_int, c_int64_t
       integer(c_int), value :: nspec, nx, ny, nz, layout
       integer(c_int64_t) :: table, peak
     end function srt_interp_layout_bytes
     integer(c_int) function srt_interp_layout_choose(nspec, nx, ny, nz, free_bytes) bind(C, name="srt_interp_layout_choose")
       import :: c_int, c_int64_t
       integer(c_int), value :: nspec, nx, ny, nz
       integer(c_int64_t), value :: free_bytes
     end function srt_interp_layout_choose
     ! modelnum = 5 (ngo_3d_dens_model_adapter.f95): the Ngo model with the plasmapause of each point at a8(MLT, kp) - ddk;
     ! fixed_MLT = 1 holds every point at MLT hours (the reference's driver never sets it)
     integer(c_int) function srt_model_create_ngo3d(configfile, kp, fixed_MLT, MLT, yearday, msec, model) &
          bind(C, name="srt_model_create_ngo3d")
       import :: c_int, c_char, c_ptr, c_double
       character(kind=c_char), intent(in) :: configfile(*)
       real(c_double), value :: kp, MLT
       integer(c_int), value :: fixed_MLT, yearday, msec
       type(c_ptr) :: model
     end function srt_model_create_ngo3d
     ! modelnum = 6 (simple_3d_model_adapter.f95): fixed_MLT = 1 holds every point at MLT hours
     integer(c_int) function srt_model_create_simple3d(kp, fixed_MLT, MLT, yearday, msec, model) &
          bind(C, name="srt_model_create_simple3d")
       import :: c_int, c_ptr, c_double
       real(c_double), value :: kp, MLT
       integer(c_int), value :: fixed_MLT, yearday, msec
       type(c_ptr) :: model
     end function srt_model_create_simple3d
     ! modelnum = 7 (AT64ThCh_adapter.f95): one field-line trace through T04_s + IGRF per evaluated point; gcpm_kp is an integer,
     ! parmod the ten --tsyganenko_* values (always needed); igrf_coeff_file: c_null_char = the table shipped with the library
     integer(c_int) function srt_model_create_at64thch(gcpm_kp, parmod, igrf_coeff_file, yearday, msec, model) &
          bind(C, name="srt_model_create_at64thch")
       import :: c_int, c_char, c_ptr, c_double
       integer(c_int), value :: gcpm_kp, yearday, msec
       real(c_double), intent(in) :: parmod(10)
       character(kind=c_char), intent(in) :: igrf_coeff_file(*)
       type(c_ptr) :: model
     end function srt_model_create_at64thch
     ! geopack's TRACE_08, batched: x(3,n) SM metres -> out(6,n) = XF YF ZF (GSM, R_E), |IGRF| there, ending, number of points
     integer(c_int) function srt_field_line_foot(model, n, x, out) bind(C, name="srt_field_line_foot")
       import :: c_int, c_int64_t, c_ptr, c_double
       type(c_ptr), value :: model
       integer(c_int64_t), value :: n
       real(c_double), intent(in) :: x(3,*)
       real(c_double) :: out(6,*)
     end function srt_field_line_foot
     integer(c_int) function srt_model_create_scattered_file(ptsfile, yearday, msec, window_scale, order, exact, &
          local_window_scale, model) bind(C, name="srt_model_create_scattered_file")
       import :: c_int, c_char, c_ptr, c_double
       character(kind=c_char), dimension(*) :: ptsfile
       integer(c_int), value :: yearday, msec, order, exact
       real(c_double), value :: window_scale, local_window_scale
       type(c_ptr) :: model
     end function srt_model_create_scattered_file
     subroutine srt_model_destroy(model) bind(C, name="srt_model_destroy")
       import :: c_ptr
       type(c_ptr), value :: model
     end subroutine srt_model_destroy
     ! --use_igrf / --use_tsyganenko of the driver (interp_dens_model_adapter.f95:214-267 and twins); coeff_file may be
     ! c_null_char-terminated empty string's address replaced by c_null_ptr semantics: pass c_null_char for the default
     integer(c_int) function srt_model_set_field(model, use_igrf, use_tsyganenko, igrf_coeff_file) &
          bind(C, name="srt_model_set_field")
       import :: c_int, c_ptr
       type(c_ptr), value :: model
       integer(c_int), value :: use_igrf, use_tsyganenko
       type(c_ptr), value :: igrf_coeff_file   ! c_null_ptr = the table shipped beside the library
     end function srt_model_set_field
     integer(c_int) function srt_model_set_tsyganenko_params(model, parmod) bind(C, name="srt_model_set_tsyganenko_params")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: model
       real(c_double), intent(in) :: parmod(10)   ! Pdyn, Dst, ByIMF, BzIMF, W1..W6
     end function srt_model_set_tsyganenko_params
     ! hot-plasma damping along the kept rows: rate(slots,nrays), magnitude(slots,nrays), flag(slots,nrays)
     integer(c_int) function srt_damping(dp, nspec, qs, ms, slots, outputper, nrays, rows, nrows, w0, rate, magnitude, flag) &
          bind(C, name="srt_damping")
       import :: c_int, c_int32_t, c_int64_t, c_double, srt_damping_params
       type(srt_damping_params), intent(in) :: dp
       integer(c_int), value :: nspec
       real(c_double), intent(in) :: qs(*), ms(*)
       integer(c_int32_t), value :: slots, outputper
       integer(c_int64_t), value :: nrays
       real(c_double), intent(in) :: rows(*), w0(*)
       integer(c_int32_t), intent(in) :: nrows(*)
       real(c_double) :: rate(*), magnitude(*)
       integer(c_int32_t) :: flag(*)
     end function srt_damping
     ! surface crossings along packed kept rows: offsets(nrays+1), rows(20, offsets(nrays+1)); event_rows and event_meta come
     ! back as malloc'd C arrays (c_f_pointer to (20, nevents) and (4, nevents); srt_free)
     integer(c_int) function srt_crossings(nsurf, surfaces, nrays, offsets, rows, nevents, event_rows, event_meta) &
          bind(C, name="srt_crossings")
       import :: c_int, c_int64_t, c_double, c_ptr, srt_surface
       integer(c_int), value :: nsurf
       type(srt_surface), intent(in) :: surfaces(*)
       integer(c_int64_t), value :: nrays
       integer(c_int64_t), intent(in) :: offsets(*)
       real(c_double), intent(in) :: rows(*)
       integer(c_int64_t) :: nevents
       type(c_ptr) :: event_rows, event_meta
     end function srt_crossings
     ! the same on device buffers (all type(c_ptr), value, but the host array `surfaces`); asynchronous on `stream`
     integer(c_int) function srt_crossings_device(nsurf, surfaces, nrays, d_offsets, d_rows, d_event_rows, d_event_meta, &
          capacity, d_count, stream) bind(C, name="srt_crossings_device")
       import :: c_int, c_int64_t, c_ptr, srt_surface
       integer(c_int), value :: nsurf
       type(srt_surface), intent(in) :: surfaces(*)
       integer(c_int64_t), value :: nrays, capacity
       type(c_ptr), value :: d_offsets, d_rows, d_event_rows, d_event_meta, d_count, stream
     end function srt_crossings_device
     ! one (4 i10, 20 es24.15e3) record per event: raynum(nevents), event_meta(4, nevents), event_rows(20, nevents)
     integer(c_int) function srt_crossings_file_write(path, nevents, raynum, event_meta, event_rows) &
          bind(C, name="srt_crossings_file_write")
       import :: c_int, c_int32_t, c_int64_t, c_double, c_char
       character(kind=c_char), dimension(*) :: path
       integer(c_int64_t), value :: nevents
       integer(c_int64_t), intent(in) :: raynum(*)
       integer(c_int32_t), intent(in) :: event_meta(*)
       real(c_double), intent(in) :: event_rows(*)
     end function srt_crossings_file_write
     ! closest approaches to observer points along packed kept rows: offsets(nrays+1), rows(20, offsets(nrays+1)); event_rows,
     ! event_meta and event_dist come back as malloc'd C arrays (c_f_pointer to (20, nevents), (4, nevents), (nevents); srt_free)
     integer(c_int) function srt_approaches(nobs, observers, nrays, offsets, rows, nevents, event_rows, event_meta, event_dist) &
          bind(C, name="srt_approaches")
       import :: c_int, c_int64_t, c_double, c_ptr, srt_observer
       integer(c_int), value :: nobs
       type(srt_observer), intent(in) :: observers(*)
       integer(c_int64_t), value :: nrays
       integer(c_int64_t), intent(in) :: offsets(*)
       real(c_double), intent(in) :: rows(*)
       integer(c_int64_t) :: nevents
       type(c_ptr) :: event_rows, event_meta, event_dist
     end function srt_approaches
     ! the same on device buffers (all type(c_ptr), value, but the host array `observers`); asynchronous on `stream`
     integer(c_int) function srt_approaches_device(nobs, observers, nrays, d_offsets, d_rows, d_event_rows, d_event_meta, &
          d_event_dist, capacity, d_count, stream) bind(C, name="srt_approaches_device")
       import :: c_int, c_int64_t, c_ptr, srt_observer
       integer(c_int), value :: nobs
       type(srt_observer), intent(in) :: observers(*)
       integer(c_int64_t), value :: nrays, capacity
       type(c_ptr), value :: d_offsets, d_rows, d_event_rows, d_event_meta, d_event_dist, d_count, stream
     end function srt_approaches_device
     ! one (4 i10, 21 es24.15e3) record per event: raynum(nevents), event_meta(4, nevents), event_dist(nevents), event_rows(20, nevents)
     integer(c_int) function srt_approaches_file_write(path, nevents, raynum, event_meta, event_dist, event_rows) &
          bind(C, name="srt_approaches_file_write")
       import :: c_int, c_int32_t, c_int64_t, c_double, c_char
       character(kind=c_char), dimension(*) :: path
       integer(c_int64_t), value :: nevents
       integer(c_int64_t), intent(in) :: raynum(*)
       integer(c_int32_t), intent(in) :: event_meta(*)
       real(c_double), intent(in) :: event_dist(*), event_rows(*)
     end function srt_approaches_file_write
     ! traced rays binned onto a grid: offsets(nrays+1), rows(20, offsets(nrays+1)), rowweight(offsets(nrays+1)) and
     ! rayweight(nrays) as type(c_ptr) (c_null_ptr = all ones; c_loc of a target array otherwise); ticks and hits come back as
     ! malloc'd C arrays of ncells int64 (c_f_pointer; srt_free); counters(4) = used, skipped, deposited, outside
     integer(c_int) function srt_bin_rays(params, nrays, offsets, rows, rowweight, rayweight, ticks, hits, counters) &
          bind(C, name="srt_bin_rays")
       import :: c_int, c_int64_t, c_double, c_ptr, srt_bin_params
       type(srt_bin_params), intent(in) :: params
       integer(c_int64_t), value :: nrays
       integer(c_int64_t), intent(in) :: offsets(*)
       real(c_double), intent(in) :: rows(*)
       type(c_ptr), value :: rowweight, rayweight
       type(c_ptr) :: ticks, hits
       integer(c_int64_t) :: counters(4)
     end function srt_bin_rays
     ! the same on device buffers (all type(c_ptr), value); ACCUMULATES into d_ticks, d_hits and d_counters, which the caller
     ! zeroes; asynchronous on `stream`
     integer(c_int) function srt_bin_rays_device(params, nrays, d_offsets, d_rows, d_rowweight, d_rayweight, d_ticks, d_hits, &
          d_counters, stream) bind(C, name="srt_bin_rays_device")
       import :: c_int, c_int64_t, c_ptr, srt_bin_params
       type(srt_bin_params), intent(in) :: params
       integer(c_int64_t), value :: nrays
       type(c_ptr), value :: d_offsets, d_rows, d_rowweight, d_rayweight, d_ticks, d_hits, d_counters, stream
     end function srt_bin_rays_device
     integer(c_int) function srt_bin_cells(params, ncells) bind(C, name="srt_bin_cells")
       import :: c_int, c_int64_t, srt_bin_params
       type(srt_bin_params), intent(in) :: params
       integer(c_int64_t) :: ncells
     end function srt_bin_cells
     ! a map as text: ticks(ncells), hits(ncells) as type(c_ptr) (c_null_ptr = zeros)
     integer(c_int) function srt_bin_file_write(path, params, ticks, hits) bind(C, name="srt_bin_file_write")
       import :: c_int, c_char, c_ptr, srt_bin_params
       character(kind=c_char), dimension(*) :: path
       type(srt_bin_params), intent(in) :: params
       type(c_ptr), value :: ticks, hits
     end function srt_bin_file_write
     ! edges, sum and hits come back as malloc'd C arrays (srt_free); params%axis(a)%edges point into edges
     integer(c_int) function srt_bin_file_read(path, params, edges, ncells, sum, hits) bind(C, name="srt_bin_file_read")
       import :: c_int, c_int64_t, c_char, c_ptr, srt_bin_params
       character(kind=c_char), dimension(*) :: path
       type(srt_bin_params) :: params
       type(c_ptr) :: edges, sum, hits
       integer(c_int64_t) :: ncells
     end function srt_bin_file_read
     integer(c_int) function srt_model_nspec(model) bind(C, name="srt_model_nspec")
       import :: c_int, c_ptr
       type(c_ptr), value :: model
     end function srt_model_nspec
     integer(c_int) function srt_model_species(model, qs, ms) bind(C, name="srt_model_species")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: model
       real(c_double) :: qs(*), ms(*)
     end function srt_model_species
     ! funcPlasmaParams, batched: x(3,n) -> qs,Ns,ms,nus(4,n), B0(3,n)
     integer(c_int) function srt_plasma_params(model, n, x, qs, Ns, ms, nus, B0) bind(C, name="srt_plasma_params")
       import :: c_int, c_ptr, c_double, c_int64_t
       type(c_ptr), value :: model
       integer(c_int64_t), value :: n
       real(c_double) :: x(3,*), qs(4,*), Ns(4,*), ms(4,*), nus(4,*), B0(3,*)
     end function srt_plasma_params
     integer(c_int32_t) function srt_rows_per_ray(p) bind(C, name="srt_rows_per_ray")
       import :: c_int32_t, srt_params
       type(srt_params) :: p
     end function srt_rows_per_ray
     ! the batched raytracer_run
     integer(c_int) function srt_trace_batch(model, p, nrays, pos0, dir0, w0, rows, nrows, stopcond, accepted_steps) &
          bind(C, name="srt_trace_batch")
       import :: c_int, c_ptr, c_double, c_int64_t, c_int32_t, srt_params
       type(c_ptr), value :: model
       type(srt_params) :: p
       integer(c_int64_t), value :: nrays
       real(c_double) :: pos0(3,*), dir0(3,*), w0(*), rows(*)
       integer(c_int32_t) :: nrows(*), stopcond(*)
       integer(c_int64_t) :: accepted_steps
     end function srt_trace_batch
     ! the same rays traced in segments of segment_rows kept rows per ray and launch (include/srt.h): open, next until it
     ! returns 0 (at most srt_trace_segments times), close
     integer(c_int32_t) function srt_trace_segments(p, segment_rows) bind(C, name="srt_trace_segments")
       import :: c_int32_t, srt_params
       type(srt_params) :: p
       integer(c_int32_t), value :: segment_rows
     end function srt_trace_segments
     integer(c_int) function srt_trace_run_open(model, p, nrays, pos0, dir0, w0, segment_rows, run) &
          bind(C, name="srt_trace_run_open")
       import :: c_int, c_ptr, c_double, c_int64_t, c_int32_t, srt_params
       type(c_ptr), value :: model
       type(srt_params) :: p
       integer(c_int64_t), value :: nrays
       real(c_double), intent(in) :: pos0(3,*), dir0(3,*), w0(*)
       integer(c_int32_t), value :: segment_rows
       type(c_ptr) :: run
     end function srt_trace_run_open
     integer(c_int) function srt_trace_run_next(run, seg) bind(C, name="srt_trace_run_next")
       import :: c_int, c_ptr, srt_segment
       type(c_ptr), value :: run
       type(srt_segment) :: seg
     end function srt_trace_run_next
     subroutine srt_trace_run_close(run) bind(C, name="srt_trace_run_close")
       import :: c_ptr
       type(c_ptr), value :: run
     end subroutine srt_trace_run_close
     ! the .ray file from packed rows: offsets(nrays+1), rows(20, offsets(nrays+1))
     integer(c_int) function srt_write_ray_file_packed(path, append, raynum0, nrays, nspec, qs, ms, w0, offsets, rows, &
          stopcond) bind(C, name="srt_write_ray_file_packed")
       import :: c_int, c_char, c_double, c_int64_t, c_int32_t
       character(kind=c_char), dimension(*) :: path
       integer(c_int), value :: append, nspec
       integer(c_int64_t), value :: raynum0, nrays
       real(c_double), intent(in) :: qs(*), ms(*), w0(*), rows(*)
       integer(c_int64_t), intent(in) :: offsets(*)
       integer(c_int32_t), intent(in) :: stopcond(*)
     end function srt_write_ray_file_packed
     integer(c_int64_t) function srt_read_rays_file(path, pos0, dir0, w0) bind(C, name="srt_read_rays_file")
       import :: c_int64_t, c_char, c_ptr
       character(kind=c_char), dimension(*) :: path
       type(c_ptr) :: pos0, dir0, w0
     end function srt_read_rays_file
     integer(c_int) function srt_write_ray_file(path, append, raynum0, nrays, p, nspec, qs, ms, w0, rows, nrows, &
          stopcond) bind(C, name="srt_write_ray_file")
       import :: c_int, c_char, c_double, c_int64_t, c_int32_t, srt_params
       character(kind=c_char), dimension(*) :: path
       integer(c_int), value :: append, nspec
       integer(c_int64_t), value :: raynum0, nrays
       type(srt_params) :: p
       real(c_double) :: qs(*), ms(*), w0(*), rows(*)
       integer(c_int32_t) :: nrows(*), stopcond(*)
     end function srt_write_ray_file
     ! dumpmodel.f95: f(4*nspec+3, nx, ny, nz) = (/qs, Ns, ms, nus, B0/) of every node; mag_coords = 1: the grid is in MAG
     integer(c_int) function srt_dump_model(model, nx, ny, nz, bounds, mag_coords, f) bind(C, name="srt_dump_model")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: model
       integer(c_int), value :: nx, ny, nz, mag_coords
       real(c_double), intent(in) :: bounds(6)   ! minx maxx miny maxy minz maxz
       real(c_double) :: f(*)
     end function srt_dump_model
     ! xform_double's sm_to_mag_d (inverse = 0) / mag_to_sm_d (inverse = 1) for x(3,n); itime = (yearday, msec)
     integer(c_int) function srt_sm_to_mag(yearday, msec, inverse, n, x, out) bind(C, name="srt_sm_to_mag")
       import :: c_int, c_int64_t, c_double
       integer(c_int), value :: yearday, msec, inverse
       integer(c_int64_t), value :: n
       real(c_double), intent(in) :: x(3,*)
       real(c_double) :: out(3,*)
     end function srt_sm_to_mag
     ! the text file dumpmodel.f95 writes; the reader's f is a c_ptr to malloc'd doubles (srt_free)
     integer(c_int) function srt_dump_file_write(path, nspec, nx, ny, nz, bounds, f) bind(C, name="srt_dump_file_write")
       import :: c_int, c_char, c_double
       character(kind=c_char), dimension(*) :: path
       integer(c_int), value :: nspec, nx, ny, nz
       real(c_double), intent(in) :: bounds(6), f(*)
     end function srt_dump_file_write
     integer(c_int) function srt_dump_file_read(path, dims, bounds, f) bind(C, name="srt_dump_file_read")
       import :: c_int, c_int32_t, c_char, c_double, c_ptr
       character(kind=c_char), dimension(*) :: path
       integer(c_int32_t) :: dims(4)   ! nspec nx ny nz
       real(c_double) :: bounds(6)
       type(c_ptr) :: f
     end function srt_dump_file_read
     subroutine srt_free(ptr) bind(C, name="srt_free")
       import :: c_ptr
       type(c_ptr), value :: ptr
     end subroutine srt_free
  end interface
end module srt_bindc
