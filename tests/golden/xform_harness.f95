! xform_harness.f95 -- golden-vector harness for the frame rotations SM <-> MAG (tests/golden/make_dumpmodel_golden.py).
!
! Our own driver, in the spirit of oracle/ref_harness.f95 and ngo3d_harness.f95: it links against the reference's xform_double
! objects (oracle/_ref/obj/xd_*.o) and calls sm_to_mag_d and mag_to_sm_d, the two procedures dumpmodel.f95's --mag_coords goes
! through, for one date and a list of points:
!   --yearday=YYYYDDD --milliseconds_day=N --in=<rows "x y z", 17 significant digits> --out=<raw float64 stream>
!   per row: sm_to_mag_d(x) (3), mag_to_sm_d(x) (3), mag_to_sm_d(sm_to_mag_d(x)) (3)
program xform_harness
  use types
  use util
  implicit none
  character(len=10000) :: buffer, infile_name, outfile_name
  integer :: foundopt, ios
  integer*4 :: itime(2)
  real(kind=DP) :: tmpinput, x(3), a(3), b(3), c(3)
  integer, parameter :: infile = 60, outfile = 61

  itime(1) = 2010001
  itime(2) = 0
  infile_name = ' '
  outfile_name = ' '
  call getopt_named('in', infile_name, foundopt)
  call getopt_named('out', outfile_name, foundopt)
  call getopt_named('yearday', buffer, foundopt)
  if (foundopt == 1) then
     read(buffer,*) tmpinput
     itime(1) = floor(tmpinput)
  end if
  call getopt_named('milliseconds_day', buffer, foundopt)
  if (foundopt == 1) then
     read(buffer,*) tmpinput
     itime(2) = floor(tmpinput)
  end if
  open(unit=infile, file=trim(infile_name), status='old')
  open(unit=outfile, file=trim(outfile_name), status='replace', access='stream', form='unformatted')
  do
     read(infile, *, iostat=ios) x
     if (ios /= 0) exit
     call sm_to_mag_d(itime, x, a)
     call mag_to_sm_d(itime, x, b)
     call mag_to_sm_d(itime, a, c)
     write(outfile) a, b, c
  end do
  close(infile)
  close(outfile)
end program xform_harness
