! at64thch_harness.f95 -- golden-vector harness for modelnum 7 (tests/golden/make_at64thch_golden.py).
!
! Our own driver, in the spirit of oracle/ref_harness.f95: it links against the reference's AT64ThCh_adapter (compiled where it
! lies, with three edits on the way into the compiler: see the generator) and against the reference's raytracer module and
! geopack, and exposes them layer by layer:
!   --mode=params   rows "x y z"                -> qs(3) Ns(3) ms(3) nus(3) B0(3)
!   --mode=trace    rows "x y z" (SM, metres)   -> XF YF ZF (GSM, R_E), |IGRF| there (nT), ending, L: geopack's own TRACE_08
!                                                  called with correctly typed arguments and the adapter's constants
!   --mode=grad     rows "x(3) k(3) w del"      -> dFdk(3) dFdw dFdx(3) evalrhs(7)
!   --mode=step     rows "args(7) dt del"       -> rk4(7) rk45 4th(7) rk45 5th(7)
!   --mode=run      rows "pos0(3) dir0(3) w"    -> per ray: raynum stopcond nrows, then nrows x
!                                                  (t pos(3) vprel(3) vgrel(3) n(3) B0(3) qs(3) ms(3) Ns(3) nus(3))
! Endings of --mode=trace, told from where the line stopped: 1 the outer boundary (r > 60, y^2 + z^2 > 1600 or x > 20), 0 the
! sphere (|r - R0| < 1e-3: the interpolated foot), 2 anything else (TRACE_08's only other exit: more than four reversals).
! Inputs are text (17 significant digits), outputs raw float64 streams.  Flags use the reference's --name=value grammar
! and the names of raytracer_driver.f95:1024-1136.
program at64thch_harness
  use types
  use util
  use constants
  use raytracer
  use AT64ThCh_adapter, only : fat64=>funcPlasmaParams, AT64ThChStateData, AT64ThChStateDataP
  implicit none

  character(len=10000) :: buffer, mode, infile_name, outfile_name
  character, allocatable :: data(:)
  integer :: foundopt, sz
  real(kind=DP) :: tmpinput
  type(AT64ThChStateData), target :: sd
  type(AT64ThChStateDataP) :: sdP

  mode = ' '
  infile_name = ' '
  outfile_name = ' '
  sd%itime(1) = 2010001
  sd%itime(2) = 0
  sd%use_tsyganenko = 0
  sd%use_igrf = 0
  sd%gcpm_kp = 4
  sd%Pdyn = 4.0_DP; sd%Dst = 1.0_DP; sd%ByIMF = 0.0_DP; sd%BzIMF = -5.0_DP
  sd%W1 = 0.132_DP; sd%W2 = 0.303_DP; sd%W3 = 0.083_DP; sd%W4 = 0.070_DP; sd%W5 = 0.211_DP; sd%W6 = 0.308_DP

  call getopt_named('mode', mode, foundopt)
  call getopt_named('in', infile_name, foundopt)
  call getopt_named('out', outfile_name, foundopt)
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
  call getopt_named('gcpm_kp', buffer, foundopt)
  if (foundopt == 1) then
     read(buffer,*) tmpinput
     sd%gcpm_kp = floor(tmpinput)
  end if
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

  sdP%p => sd
  sz = size(transfer(sdP, data))
  allocate(data(sz))
  data = transfer(sdP, data)

  open(unit=71, file=trim(infile_name), status='old')
  open(unit=72, file=trim(outfile_name), access='stream', form='unformatted', status='replace')
  select case (trim(mode))
  case ('params')
     call do_params()
  case ('trace')
     call do_trace()
  case ('grad')
     call do_grad()
  case ('step')
     call do_step()
  case ('run')
     call do_run()
  case default
     print *, 'at64thch_harness: unknown mode ', trim(mode)
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
       call fat64(x, qs, Ns, ms, nus, B0, data)
       write(72) qs, Ns, ms, nus, B0
    end do
  end subroutine do_params

  subroutine do_trace()
    external :: T04_s, IGRF_GSM
    real(kind=DP) :: x(3), x_gsm(3), r0s
    real(kind=SP) :: parmod(10), xx(500), yy(500), zz(500), xf, yf, zf, bx, by, bz, dir, dsmax, err, rlim, r, ryz
    integer :: status, L, lmax, iopt, ending, whole_seconds
    integer :: ymd(2), hms(3)
    ! calendar fields for tsy_recalc: yearday = yyyyddd, then the day's whole seconds as h, m, s
    ymd = (/ sd%itime(1) / 1000, modulo(sd%itime(1), 1000) /)
    whole_seconds = sd%itime(2) / 1000
    hms = (/ whole_seconds / 3600, modulo(whole_seconds, 3600) / 60, modulo(whole_seconds, 60) /)
    parmod = real((/ sd%Pdyn, sd%Dst, sd%ByIMF, sd%BzIMF, sd%W1, sd%W2, sd%W3, sd%W4, sd%W5, sd%W6 /))
    iopt = 0
    lmax = 500
    dir = 1
    dsmax = 1
    err = 0.0001
    rlim = 60
    r0s = (400.0e3_DP+R_E)/R_E
    do
       read(71, *, iostat=status) x
       if (status /= 0) exit
       call SM_TO_GSM_d(sd%itime, x, x_gsm)
       call tsy_recalc(ymd(1), ymd(2), hms(1), hms(2), hms(3))
       call TRACE_08(real(x_gsm(1)/R_E), real(x_gsm(2)/R_E), real(x_gsm(3)/R_E), dir, dsmax, err, rlim, real(r0s), &
            iopt, parmod, T04_s, IGRF_GSM, xf, yf, zf, xx, yy, zz, L, lmax)
       call IGRF_GSM(xf, yf, zf, bx, by, bz)
       ryz = yf**2 + zf**2
       r = sqrt(xf**2 + ryz)
       if (r > rlim .or. ryz > 1600.0 .or. xf > 20.0) then
          ending = 1
       else if (abs(r - real(r0s)) < 1.0e-3) then
          ending = 0
       else
          ending = 2
       end if
       write(72) real(xf,kind=DP), real(yf,kind=DP), real(zf,kind=DP), real(sqrt(bx*bx + by*by + bz*bz),kind=DP), &
            real(ending,kind=DP), real(L,kind=DP)
    end do
  end subroutine do_trace

  subroutine do_grad()
    real(kind=DP) :: x(3), k(3), w, del, dfdk(3), dfdw, dfdx(3), rhs(7), args(7)
    integer :: status
    do
       read(71, *, iostat=status) x, k, w, del
       if (status /= 0) exit
       dfdk = dispersion_relation_dFdk(k, w, x, 1.0e-8_DP, fat64, data)
       dfdw = dispersion_relation_dFdw(k, w, x, 1.0e-8_DP, fat64, data)
       dfdx = dispersion_relation_dFdx(k, w, x, del, fat64, data)
       args(1:3) = x
       args(4:6) = k
       args(7) = w
       rhs = raytracer_evalrhs(0.0_DP, args, del, fat64, data)
       write(72) dfdk, dfdw, dfdx, rhs
    end do
  end subroutine do_grad

  subroutine do_step()
    real(kind=DP) :: args(7), dt, del, o4(7), o5(7), r4(7)
    integer :: status
    do
       read(71, *, iostat=status) args, dt, del
       if (status /= 0) exit
       r4 = rk4(0.0_DP, args, del, dt, fat64, data)
       call rk45(0.0_DP, args, del, dt, fat64, data, o4, o5)
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
    del = 1.0e-4_DP
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
            fixedstep, del, fat64, data, raytracer_stopconditions)
       write(72) real(raynum,kind=DP), real(stopcond,kind=DP), real(size(time,1),kind=DP)
       do i = 1, size(time,1)
          write(72) time(i), pos(:,i), vprel(:,i), vgrel(:,i), n(:,i), B0(:,i), &
               qs(:,i), ms(:,i), Ns(:,i), nus(:,i)
       end do
       deallocate(pos, time, vprel, vgrel, n, B0, qs, ms, Ns, nus)
       raynum = raynum + 1
    end do
  end subroutine do_run

end program at64thch_harness
