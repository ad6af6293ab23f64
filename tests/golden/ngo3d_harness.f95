! ngo3d_harness.f95 -- golden-vector harness for modelnum 5 (tests/golden/make_ngo3d_golden.py).
!
! Our own driver, in the spirit of oracle/ref_harness.f95 and simple3d_harness.f95: it links against the reference's
! ngo_3d_dens_model_adapter and ngo_3d_dens_model (the objects build() leaves in oracle/_ref/obj) and against the reference's
! raytracer module, calls the adapter's setup with --ngo_configfile, and exposes the model layer by layer:
!   --mode=params   rows "x y z"                -> qs(4) Ns(4) ms(4) nus(4) B0(3) lk
!                                                  (lk: the density module's plasmapause as the call left it)
!   --mode=grad     rows "x(3) k(3) w del"      -> dFdk(3) dFdw dFdx(3) evalrhs(7)
!   --mode=step     rows "args(7) dt del"       -> rk4(7) rk45 4th(7) rk45 5th(7)
!   --mode=run      rows "pos0(3) dir0(3) w"    -> per ray: raynum stopcond nrows, then nrows x
!                                                  (t pos(3) vprel(3) vgrel(3) n(3) B0(3) qs(4) ms(4) Ns(4) nus(4))
! Inputs are text (17 significant digits), outputs raw float64 streams.  Flags use the reference's --name=value grammar
! and the names of raytracer_driver.f95:772-891.
program ngo3d_harness
  use types
  use util
  use constants
  use raytracer
  use ngo_3d_dens_model_adapter, only : fngo3d=>funcPlasmaParams, ngo3dStateData, ngo3dStateDataP, ngo3dsetup=>setup
  use ngo_3d_dens_model, only : lk
  implicit none

  character(len=10000) :: buffer, mode, infile_name, outfile_name, configfile
  character, allocatable :: data(:)
  integer :: foundopt, sz
  real(kind=DP) :: tmpinput
  type(ngo3dStateData), target :: sd
  type(ngo3dStateDataP) :: sdP

  mode = ' '
  infile_name = ' '
  outfile_name = ' '
  configfile = ' '
  sd%itime(1) = 2010001
  sd%itime(2) = 0
  sd%use_tsyganenko = 0
  sd%use_igrf = 0
  sd%fixed_MLT = 0
  sd%MLT = 0.0_DP
  sd%kp = 4.0_DP
  sd%Pdyn = 4.0_DP; sd%Dst = 1.0_DP; sd%ByIMF = 0.0_DP; sd%BzIMF = -5.0_DP
  sd%W1 = 0.132_DP; sd%W2 = 0.303_DP; sd%W3 = 0.083_DP; sd%W4 = 0.070_DP; sd%W5 = 0.211_DP; sd%W6 = 0.308_DP

  call getopt_named('mode', mode, foundopt)
  call getopt_named('in', infile_name, foundopt)
  call getopt_named('out', outfile_name, foundopt)
  call getopt_named('ngo_configfile', configfile, foundopt)
  if (foundopt /= 1) then
     print *, 'ngo3d_harness: --ngo_configfile is required'
     stop 2
  end if
  call getopt_named('yearday', buffer, foundopt)
  if (foundopt == 1) then
     read(buffer,*) tmpinput
     sd%itime(1) = floor(tmpinput)
  end if
  call getopt_named('milliseconds_day', buffer, foundopt)
  if (foundopt == 1) then
     read(buffer,*) tmpinput
     sd%itime(2) = floor(tmpinput)
  end if
  call getopt_named('use_igrf', buffer, foundopt)
  if (foundopt == 1) then
     read(buffer,*) tmpinput
     sd%use_igrf = floor(tmpinput)
  end if
  call getopt_named('use_tsyganenko', buffer, foundopt)
  if (foundopt == 1) then
     read(buffer,*) tmpinput
     sd%use_tsyganenko = floor(tmpinput)
  end if
  call getopt_named('fixed_MLT', buffer, foundopt)
  if (foundopt == 1) then
     read(buffer,*) tmpinput
     sd%fixed_MLT = floor(tmpinput)
  end if
  call getopt_named('MLT', buffer, foundopt)
  if (foundopt == 1) read(buffer,*) sd%MLT
  call getopt_named('kp', buffer, foundopt)
  if (foundopt == 1) read(buffer,*) sd%kp
  call getopt_named('tsyganenko_Pdyn', buffer, foundopt)
  if (foundopt == 1) read(buffer,*) sd%Pdyn
  call getopt_named('tsyganenko_Dst', buffer, foundopt)
  if (foundopt == 1) read(buffer,*) sd%Dst
  call getopt_named('tsyganenko_ByIMF', buffer, foundopt)
  if (foundopt == 1) read(buffer,*) sd%ByIMF
  call getopt_named('tsyganenko_BzIMF', buffer, foundopt)
  if (foundopt == 1) read(buffer,*) sd%BzIMF
  call getopt_named('tsyganenko_W1', buffer, foundopt)
  if (foundopt == 1) read(buffer,*) sd%W1
  call getopt_named('tsyganenko_W2', buffer, foundopt)
  if (foundopt == 1) read(buffer,*) sd%W2
  call getopt_named('tsyganenko_W3', buffer, foundopt)
  if (foundopt == 1) read(buffer,*) sd%W3
  call getopt_named('tsyganenko_W4', buffer, foundopt)
  if (foundopt == 1) read(buffer,*) sd%W4
  call getopt_named('tsyganenko_W5', buffer, foundopt)
  if (foundopt == 1) read(buffer,*) sd%W5
  call getopt_named('tsyganenko_W6', buffer, foundopt)
  if (foundopt == 1) read(buffer,*) sd%W6

  call ngo3dsetup(sd, trim(configfile))
  sdP%p => sd
  sz = size(transfer(sdP, data))
  allocate(data(sz))
  data = transfer(sdP, data)

  open(unit=71, file=trim(infile_name), status='old')
  open(unit=72, file=trim(outfile_name), access='stream', form='unformatted', status='replace')
  select case (trim(mode))
  case ('params')
     call do_params()
  case ('grad')
     call do_grad()
  case ('step')
     call do_step()
  case ('run')
     call do_run()
  case default
     print *, 'ngo3d_harness: unknown mode ', trim(mode)
     stop 2
  end select
  close(71)
  close(72)

contains

  subroutine do_params()
    real(kind=DP) :: x(3), B0(3)
    real(kind=DP), allocatable :: qs(:), Ns(:), ms(:), nus(:)
    integer :: status
    do
       read(71, *, iostat=status) x
       if (status /= 0) exit
       call fngo3d(x, qs, Ns, ms, nus, B0, data)
       write(72) qs, Ns, ms, nus, B0, lk
    end do
  end subroutine do_params

  subroutine do_grad()
    real(kind=DP) :: x(3), k(3), w, del, dfdk(3), dfdw, dfdx(3), rhs(7), args(7)
    integer :: status
    do
       read(71, *, iostat=status) x, k, w, del
       if (status /= 0) exit
       dfdk = dispersion_relation_dFdk(k, w, x, 1.0e-8_DP, fngo3d, data)
       dfdw = dispersion_relation_dFdw(k, w, x, 1.0e-8_DP, fngo3d, data)
       dfdx = dispersion_relation_dFdx(k, w, x, del, fngo3d, data)
       args(1:3) = x
       args(4:6) = k
       args(7) = w
       rhs = raytracer_evalrhs(0.0_DP, args, del, fngo3d, data)
       write(72) dfdk, dfdw, dfdx, rhs
    end do
  end subroutine do_grad

  subroutine do_step()
    real(kind=DP) :: args(7), dt, del, o4(7), o5(7), r4(7)
    integer :: status
    do
       read(71, *, iostat=status) args, dt, del
       if (status /= 0) exit
       r4 = rk4(0.0_DP, args, del, dt, fngo3d, data)
       call rk45(0.0_DP, args, del, dt, fngo3d, data, o4, o5)
       write(72) r4, o4, o5
    end do
  end subroutine do_step

  subroutine do_run()
    real(kind=DP) :: del, pos0(3), w, dir0(3), dt0, dtmax, maxerr, tmax, minalt
    integer :: fixedstep, root, maxsteps, stopcond, raynum, status, i
    real(kind=DP), allocatable :: pos(:,:), time(:), vprel(:,:), vgrel(:,:), &
         n(:,:), B0(:,:), qs(:,:), ms(:,:), Ns(:,:), nus(:,:)

    dt0 = 1.0e-3_DP; dtmax = 0.1_DP; maxerr = 5.0e-4_DP; tmax = 1.0_DP
    minalt = 6.4712e6_DP; fixedstep = 0; root = 2; maxsteps = 2000
    del = 1.0e-6_DP
    call getopt_named('dt0', buffer, foundopt)
    if (foundopt == 1) read(buffer,*) dt0
    call getopt_named('dtmax', buffer, foundopt)
    if (foundopt == 1) read(buffer,*) dtmax
    call getopt_named('tmax', buffer, foundopt)
    if (foundopt == 1) read(buffer,*) tmax
    call getopt_named('maxerr', buffer, foundopt)
    if (foundopt == 1) read(buffer,*) maxerr
    call getopt_named('minalt', buffer, foundopt)
    if (foundopt == 1) read(buffer,*) minalt
    call getopt_named('del', buffer, foundopt)
    if (foundopt == 1) read(buffer,*) del
    call getopt_named('fixedstep', buffer, foundopt)
    if (foundopt == 1) then
       read(buffer,*) tmpinput
       fixedstep = floor(tmpinput)
    end if
    call getopt_named('maxsteps', buffer, foundopt)
    if (foundopt == 1) then
       read(buffer,*) tmpinput
       maxsteps = floor(tmpinput)
    end if
    raynum = 1
    do
       read(71, *, iostat=status) pos0, dir0, w
       if (status /= 0) exit
       call raytracer_run(pos, time, vprel, vgrel, n, B0, qs, ms, Ns, nus, stopcond, &
            pos0, dir0, w, dt0, dtmax, maxerr, maxsteps, minalt, root, tmax, &
            fixedstep, del, fngo3d, data, raytracer_stopconditions)
       write(72) real(raynum,kind=DP), real(stopcond,kind=DP), real(size(time,1),kind=DP)
       do i = 1, size(time,1)
          write(72) time(i), pos(:,i), vprel(:,i), vgrel(:,i), n(:,i), B0(:,i), &
               qs(:,i), ms(:,i), Ns(:,i), nus(:,i)
       end do
       deallocate(pos, time, vprel, vgrel, n, B0, qs, ms, Ns, nus)
       raynum = raynum + 1
    end do
  end subroutine do_run

end program ngo3d_harness
