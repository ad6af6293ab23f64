/* srt.h -- C ABI of the MI355X-native many-ray Haselgrove integrator (libsrt_hip.so).
 *
 * Drop-in boundary for ONE path of rareid2/Stanford_Raytracer: the ray loop of
 * fortran/raytracer_driver.f95:1144-1232, i.e. the per-ray call
 *     call raytracer_run(pos,time,vprel,vgrel,n,B0,qs,ms,Ns,nus,stopcond, pos0,dir0,w,dt0,dtmax,
 *                        maxerr,maxsteps,minalt,root,tmax,fixedstep,del,funcPlasmaParams,data,
 *                        raytracer_stopconditions)            (signature fortran/raytracer.f95:609-642)
 * becomes one batched call, srt_trace_batch().  The reference's plugin callback
 *     subroutine funcPlasmaParams(x, qs, Ns, ms, nus, B0, funcPlasmaParamsData)   (raytracer.f95:121-129)
 * cannot be a host callback on a GPU path; its six in-scope implementations are selected by the
 * model handle instead (modelnum 1 / 3 / 4 / 5 / 6 / 7 of raytracer_driver.f95:256-1136) and are exposed for
 * point queries through srt_plasma_params().
 *
 * Conventions: plain pointers and sizes, no C++ or torch types.  All arrays are HOST memory unless a
 * function name ends in _device.  Vectors are AoS: pos0[i*3+c].  Every function returns 0 on success
 * or a negative SRT_E* code; srt_last_error() gives the text.  Per-ray failures never abort a batch:
 * they are reported through stopcond (same codes as raytracer.f95:324-353, plus SRT_STOP_NUMERIC for
 * the reference's process-killing `stop` on an SVD failure, blas.f95:208-211, or in modelnum 6's check_crossing, and for
 * a field line of modelnum 7 that has not ended after 500 points).
 * The library needs a gfx950 GPU; there is no CPU fallback.
 */
#ifndef SRT_H
#define SRT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SRT_VERSION 1
#define SRT_MAXSPEC 4
/* one trajectory row: t, pos[3], vprel[3], vgrel[3], n[3], B0[3], Ns[4]  (the per-step outputs of
 * raytracer_run; qs/ms/nus are per-model constants, see srt_model_species) */
#define SRT_ROW 20

enum {
  SRT_OK = 0,
  SRT_EINVAL = -1,  /* bad argument */
  SRT_EIO = -2,     /* file could not be read / written / parsed */
  SRT_EDEVICE = -3, /* HIP error or no gfx950 device */
  SRT_ENOMEM = -4
};

/* stop codes, raytracer.f95:324-353 and :749-754 */
enum {
  SRT_STOP_TMAX = 0,    /* t >= tmax (also: fixed-step ray left the resonance cone, :900-905) */
  SRT_STOP_MINALT = 1,  /* |pos| < minalt */
  SRT_STOP_KZERO = 2,   /* |k| == 0 */
  SRT_STOP_VGROUP = 3,  /* |vgrel| > 1.01 */
  SRT_STOP_DT = 5,      /* dt < 1e-14 */
  SRT_STOP_MAXSTEPS = 6,
  SRT_STOP_NUMERIC = 9  /* ours: non-finite state where the reference would `stop` the process */
};

/* integrator parameters = the scalar arguments of raytracer_run + the driver's outputper */
typedef struct srt_params {
  double dt0, dtmax, tmax, maxerr, minalt;
  double del;        /* FD step for dF/dx: 1e-4 for model 1, 1e-6 for models 3,4 (driver:251-252) */
  int32_t maxsteps;
  int32_t root;      /* 1 or 2 (2 = whistler) */
  int32_t fixedstep; /* 1 = RK4, 0 = adaptive RKF45 */
  int32_t outputper; /* keep rows 0, outputper, 2*outputper, ... (driver:1197) */
  int32_t first_attempt_policy; /* a ray's FIRST adaptive attempt, where raytracer.f95:778 reads an unset local (SURVEY A-1):
                                   0: NaN error term => accepted at dt0, dt not grown (what a flang build of the reference does,
                                      hence the goldens of this repository, api.make_params and bench.py);
                                   1: error from the k term alone (what the reference's own gfortran toolchain does; the
                                      `raytracer` executable's default, --first_attempt_policy).
                                   THE LIBRARY HAS NO DEFAULT: this member is read as given (a zeroed struct = 0); callers
                                   that replace a gfortran-built reference set 1.  INTEGRATION.md section 3. */
  int32_t refill_threshold;     /* free lanes per wave before new rays are claimed (0 = default) */
  int32_t ray_order;            /* order in which the launch set is WORKED ON (results and their order are unchanged):
                                   0 = as given; 1 = sorted on the device by the Morton code of the launch cell, so
                                   that the lanes of a wave start in neighbouring cells of the interp grid and share
                                   coefficient lines (SURVEY.md 8d allows this input permutation; other models ignore it);
                                   2 = as 1 with the rays that are likely to stop early (above 6 kHz, launched inwards)
                                   behind all others -- an experiment switch for the launch's tail, not a gain (HISTORY.md section 9) */
} srt_params;

typedef struct srt_model srt_model; /* opaque; owns device copies of all model data */

/* ---- library ---- */
/* Binds the CALLING THREAD to a HIP device (and makes it the default for threads that never call srt_init).  Models are
 * created on the calling thread's device and remember it: one host thread per GPU can drive its own model replica
 * (the CLI's --devices=0,1,..; the reference has no parallel mode, raytracer_driver.f95:1144-1232 is a serial loop). */
int srt_init(int device);
const char *srt_last_error(void);
int srt_device_info(char *name, int name_len, int *cu_count, int64_t *hbm_bytes);

/* ---- models (replace ngosetup / interpsetup / scatteredinterpsetup + the TRANSFER'd state blob) ---- */
/* modelnum=1: Ngo diffusive-equilibrium model; configfile is the legacy newray.in card file
 * (ngo_dens_model.f95:29-160).  yearday/msec = itime of the adapters (dipole tilt). */
int srt_model_create_ngo(const char *configfile, int yearday, int msec, srt_model **out);
/* modelnum=3: regular grid of ln(N_s), text file in the format of
 * gcpm_dens_model_buildgrid.f95:302-327 as read by interp_dens_model_adapter.f95:58-117 */
int srt_model_create_interp_file(const char *gridfile, int yearday, int msec, srt_model **out);
/* same, from host arrays: F[nz][ny][nx][nspec] (file order: species fastest, then x, y, z);
 * derivs = NULL (finite differences as libtricubic.f95:722-793) or 7 arrays of F's shape in the
 * order dfdx, dfdy, dfdz, d2fdxdy, d2fdxdz, d2fdydz, d3fdxdydz */
int srt_model_create_interp(int nspec, int nx, int ny, int nz, const double bounds[6],
                            const double *qs, const double *ms, const double *F,
                            const double *const *derivs, int yearday, int msec, srt_model **out);
/* modelnum=4: scattered ln(N_s) samples, text file of gcpm_dens_model_buildgrid_random.f95:210-225;
 * parameters are the --scattered_interp_* flags of raytracer_driver.f95:690-728.  order = degree of the fitted monomials: 0..3 (the
 * reference's tabular_monomials, lsinterp_mod.f95:70-99) on the kernels built for speed, 4 and 5 (its generate_monomials, :114-164:
 * 35 / 56 monomials) on one cooperative path that answers at ~1 % of order 2's rate; order >= 6 is refused with SRT_EINVAL */
int srt_model_create_scattered_file(const char *ptsfile, int yearday, int msec, double window_scale,
                                    int order, int exact, double local_window_scale, srt_model **out);
/* The same with the reference's kd-tree ROOT reproduced (opt-in, for diffing against a reference binary): the reference's
 * kdtree_nearest starts its search at the tree's root (kdtree_mod.f95:386-444), so for the ONE sample that is the root
 * "the nearest other sample" is the sample itself -- its stored spacing stays 0 and does not enter maxnearest
 * (scattered_interp_dens_model_adapter.f95:167-203).  Every lookup whose search window holds that sample sees
 * it.  Which sample it is comes from the reference build's RNG (randperm, :137-140), so the caller names it:
 * root_sample = its 0-based record number in the file (the reference prints nothing; a harness linked against its modules can
 * ask the tree -- oracle/ref_harness.f95 --mode=scatroot), -1 = none = srt_model_create_scattered_file, which stores the true
 * distance for every sample (the documented default). */
int srt_model_create_scattered_file_root(const char *ptsfile, int yearday, int msec, double window_scale,
                                         int order, int exact, double local_window_scale, int64_t root_sample,
                                         srt_model **out);
/* modelnum=6: simple_3d_model_adapter.f95; fixed_MLT = 1 holds every point at MLT hours.
 * The closed-form "simplified GCPM": Carpenter-Anderson plasmasphere, Kp- and MLT-dependent plasmapause (pp_profile_d.f95),
 * MLT-dependent trough, a fitted ionosphere merged at an altitude the model searches for, He+ / O+ / H+ fractions; no
 * tables.  kp = the driver's --kp, yearday / msec = itime (day of year for the plasmasphere's annual term, dipole tilt).
 * DEFINED BEHAVIOUR where the adapter reads three locals that nothing sets (the reference's toolchain zeroes them with
 * -finit-local-zero); all three are 0 at every call:
 *   rz12 in ne_ps (:106, shadows the module parameter): the sunspot term of x234 is 0.00127*0 - 0.0635;
 *   diff in find_intersection_iono_ps (:585): the first trip of the altitude search never flips its step, 2000 -> 3000 km;
 *   switch_cap in funcPlasmaParams (:790): aHeH is not reduced.
 * With do_cap = 0 the polar-cap code (ne_cap, poleward_edge) is dead and is not part of this library.  Where the
 * reference stops the process ("Failed to find knee in check_crossing") the densities are NaN and a traced ray ends with
 * SRT_STOP_NUMERIC. */
/* modelnum=5: ngo_3d_dens_model_adapter.f95 + ngo_3d_dens_model.f95, the 3-D Ngo model.  Modelnum 1's diffusive-equilibrium
 * plasmasphere, read from the same card file, with the plasmapause moved at every evaluated point to where pp_profile_d.f95's
 * bulge puts it for the point's MLT and Kp: lk = a8(MLT, kp) - ddk, in the knee and in the sinusoidal perturbation of the ducts.
 * The file's own lk serves only the normalisation of ane0 at setup (readinput), never a density.  MLT comes from the point's
 * longitude, mod(24 phi / 2 pi + 12, 24); fixed_MLT = 1 holds every point at MLT hours instead.  The driver maps
 * --ngo_configfile, --kp, --yearday, --milliseconds_day, --use_tsyganenko, --use_igrf and the ten --tsyganenko_* flags to this
 * model (raytracer_driver.f95:772-891; the field flags go through srt_model_set_field / srt_model_set_tsyganenko_params); it
 * never sets fixed_MLT or MLT itself, so a run of the driver is fixed_MLT = 0.  The driver's step for this model is
 * del = 1e-6.  Kind 5, four species (electrons, H+, He+, O+). */
int srt_model_create_ngo3d(const char *configfile, double kp, int fixed_MLT, double MLT, int yearday, int msec, srt_model **out);
int srt_model_create_simple3d(double kp, int fixed_MLT, double MLT, int yearday, int msec, srt_model **out);
/* modelnum=7: AT64ThCh_adapter.f95, a diffusive-equilibrium plasmasphere (electrons, O+, H+: kind 7, three species) whose
 * electron density above 400 km is scaled by |B(point)| / |B(foot)|: for EVERY evaluated point geopack's TRACE_08 follows the
 * field line of T04_s + IGRF from the point to the sphere r = R_E + 400 km (srt_field_line_foot below is that trace alone).
 * gcpm_kp = the driver's --gcpm_kp, an integer; parmod = the ten --tsyganenko_* values; igrf_coeff_file as for
 * srt_model_set_field (NULL = the table shipped with the library).  The trace always uses T04_s and IGRF, whatever
 * srt_model_set_field says later: use_igrf / use_tsyganenko choose only the base field of |B(point)| and the returned B0, so the
 * model always owns a coefficient table and parmod (srt_model_set_tsyganenko_params replaces the latter).  A point at or below
 * 400 km takes the ratio 1 without a trace; a line that leaves through the outer boundary (r > 60, y^2 + z^2 > 1600, x > 20 R_E or
 * more than four reversals) has no foot on the sphere, and |B(foot)| is IGRF wherever the trace stopped, as in the Fortran.
 * The driver's step for this model is del = 1e-4.
 * Three things the adapter leaves undefined, and what this library does:
 *  1. it hands its DOUBLE parmod to TRACE_08, whose PARMOD is REAL, so the reference's trace runs T04_s on reinterpreted bytes
 *     (Pdyn = 0 for the usual --tsyganenko_Pdyn=4; a segmentation fault for 1.7).  Here the trace sees real(parmod), as the
 *     adapter's own final T04_s call does.
 *  2. its local `psi`, read by that final T04_s call (use_tsyganenko = 1), is never set; the reference's toolchain zeroes
 *     locals, so it is 0 here.  The trace itself uses geopack's own dipole tilt PSI for the date (RECALC_08).
 *  3. TRACE_08's bounds check is commented out and the adapter's arrays hold 500 points.  Here a line that has not ended after
 *     500 points (or whose step was halved 64 times in a row) gives NaN densities, and a traced ray ends with SRT_STOP_NUMERIC. */
int srt_model_create_at64thch(int gcpm_kp, const double parmod[10], const char *igrf_coeff_file, int yearday, int msec,
                              srt_model **out);
/* The step before the path: sample a model's funcPlasmaParams on a regular nx x ny x nz grid in
 * log space ON THE DEVICE -- gcpm_dens_model_buildgrid.f95:160-300 with any model handle in place of GCPM.
 * compder = 1 adds the seven explicit finite-difference blocks (d = 1e-3*|pos|, :197-296); compder = 0 leaves the
 * derivatives to the interp model's own finite differences, as the adapter does.
 *   srt_build_grid: host outputs F[nz][ny][nx][nspec] and derivs (7 blocks concatenated; may be NULL if !compder),
 *                   ready for srt_grid_file_write.
 *   srt_model_create_interp_from_model: the same grid becomes a modelnum=3 model without leaving the device. */
int srt_build_grid(srt_model *src, int compder, int nx, int ny, int nz, const double bounds[6], double *F,
                   double *derivs);
int srt_model_create_interp_from_model(srt_model *src, int compder, int nx, int ny, int nz,
                                       const double bounds[6], int yearday, int msec, srt_model **out);
/* modelnum=3 has two device layouts of the same model (same lookups, same answers):
 *   SRT_INTERP_EXPANDED: coef[cell][species][64], the 64 tricubic coefficients of every cell expanded once at creation; a
 *     lookup is one contiguous read.  (nx+1)(ny+1)(nz+1) nspec 512 bytes.  What the three creators above make.
 *   SRT_INTERP_NODES: nodes[k][j][i][species][8], the eight values per node the coefficients are formed from, which a
 *     lookup does itself.  nx ny nz nspec 64 bytes: an eighth, for grids (or sets of grids) the expanded table has no room
 *     for; more arithmetic per lookup.
 *   SRT_INTERP_AUTO: EXPANDED when creation fits into the device's free memory, else NODES, else SRT_ENOMEM
 *     (srt_interp_layout_choose applied to hipMemGetInfo's free bytes).
 * The _layout creators take the arguments of their namesakes plus the layout; any other layout number is SRT_EINVAL.
 * srt_model_interp_layout: the layout a handle has (0 or 1), -1 for other kinds; srt_model_kind answers 3 for both. */
#define SRT_INTERP_EXPANDED 0
#define SRT_INTERP_NODES 1
#define SRT_INTERP_AUTO 2
int srt_model_create_interp_layout(int nspec, int nx, int ny, int nz, const double bounds[6],
                                   const double *qs, const double *ms, const double *F,
                                   const double *const *derivs, int yearday, int msec, int layout, srt_model **out);
int srt_model_create_interp_file_layout(const char *gridfile, int yearday, int msec, int layout, srt_model **out);
int srt_model_create_interp_from_model_layout(srt_model *src, int compder, int nx, int ny, int nz,
                                              const double bounds[6], int yearday, int msec, int layout, srt_model **out);
int srt_model_interp_layout(const srt_model *m);
/* Pure host code, needs no GPU.  layout = SRT_INTERP_EXPANDED or SRT_INTERP_NODES.
 *   srt_interp_layout_bytes: *table = bytes of the table, *peak = the most that creation holds at once (the eight grid
 *     arrays and the table); either may be NULL.
 *   srt_interp_layout_choose: SRT_INTERP_EXPANDED if its peak fits into free_bytes, else SRT_INTERP_NODES if that fits,
 *     else SRT_ENOMEM. */
int srt_interp_layout_bytes(int nspec, int nx, int ny, int nz, int layout, int64_t *table, int64_t *peak);
int srt_interp_layout_choose(int nspec, int nx, int ny, int nz, int64_t free_bytes);
/* The other builder of the step before the path: the random / adaptive sample set of
 * gcpm_dens_model_buildgrid_random.f95:228-407 + randomsampling_mod.f95:27-200 (recursivesampler), with any model
 * handle in place of GCPM, generated and refined ON THE DEVICE.  Stage order and per-stage rules are the reference's:
 * points of an existing file first (in_pts, kept and pushed to the output), n_initial_radial shell samples retried
 * until inside the box, n_initial_uniform samples, adaptive passes with tol = initial_tol, tol/2, ... until
 * adaptive_nmax adaptive samples exist, n_zero_altitude samples on the sphere r = R_E and n_iri_pad samples in the
 * shell R_E .. R_E+2000 km (both kept only when inside the box).  The recursion of one pass is evaluated level by
 * level (all half-boxes of one depth at once) from counter-based random numbers, so the set is a pure function of
 * `seed` (the reference seeds from the clock).  max_passes bounds the tolerance-halving loop, which the reference
 * leaves unbounded (0 = 64).  out = malloc'd [n_out][3+nspec] records "x y z lnN_1..lnN_nspec", the lines of the
 * model-4 file (srt_free); stage_counts[6] = samples from {input, radial, uniform, adaptive, zero altitude, iri}. */
typedef struct srt_sampler_params {
  double bounds[6];          /* minx maxx miny maxy minz maxz */
  int64_t n_zero_altitude, n_iri_pad, n_initial_radial, n_initial_uniform, adaptive_nmax;
  double initial_tol;
  int32_t max_recursion;
  int32_t numincrease;       /* the reference passes 5 (gcpm_dens_model_buildgrid_random.f95:338); 0 = 5 */
  int32_t max_passes;
  int32_t reserved;
  uint64_t seed;
} srt_sampler_params;
int srt_build_samples(srt_model *src, const srt_sampler_params *sp, int64_t n_in, const double *in_pts,
                      int64_t *n_out, double **out, int64_t stage_counts[6]);
/* Field options of the adapters (driver flags --use_igrf / --use_tsyganenko; interp_dens_model_adapter.f95:214-267
 * and its twins), evaluated on the device at every lookup, in the arithmetic types of the Fortran:
 *   use_igrf = 1: IGRF main field instead of the dipole (geopack2008.for IGRF_GSW_08 after RECALC_08 for the model's
 *     yearday / milliseconds_day, REAL);
 *   use_tsyganenko = 1: the T04_s (Tsyganenko & Sitnov 2005) external field added to it (TS05_aka_TS04.for, REAL*8
 *     inside, REAL interface), with PARMOD from srt_model_set_tsyganenko_params and geopack's dipole tilt for the date.
 * igrf_coeff_file = table of the published Gauss coefficients, needed by either option (NULL: $SRT_IGRF_COEFFS, else the
 * data/igrf_coeffs.txt shipped beside the library). */
int srt_model_set_field(srt_model *m, int use_igrf, int use_tsyganenko, const char *igrf_coeff_file);
/* parmod[10] = Pdyn (nPa), Dst (nT), ByIMF, BzIMF (nT), W1 .. W6: the driver's --tsyganenko_* flags */
int srt_model_set_tsyganenko_params(srt_model *m, const double parmod[10]);
void srt_model_destroy(srt_model *m);
int srt_model_kind(const srt_model *m);  /* 1, 3, 4, 5, 6 or 7 */
int srt_model_nspec(const srt_model *m);
int srt_model_species(const srt_model *m, double qs[SRT_MAXSPEC], double ms[SRT_MAXSPEC]);
int64_t srt_model_device_bytes(const srt_model *m);
/* device address of the handle's model struct, as the kernels read it (its type belongs to the handle's kind and layout: csrc/);
 * for probes of device-only code that run beside the library in the same process.  Valid until srt_model_destroy. */
const void *srt_model_device_struct(const srt_model *m);

/* ---- layered entry points (each mirrors one reference procedure, batched over n items) ---- */
/* funcPlasmaParams: x[n][3] -> qs,Ns,ms,nus [n][4], B0[n][3] */
int srt_plasma_params(srt_model *m, int64_t n, const double *x, double *qs, double *Ns, double *ms,
                      double *nus, double *B0);
/* dispersion_relation + stix_parameters + solve_dispersion_relation at (x,k,w):
 * out[n][10] = F, S, D, P, R, L, Re k1, Im k1, Re k2, Im k2   (raytracer.f95:41-102, 408-502) */
int srt_dispersion(srt_model *m, int64_t n, const double *x, const double *k, const double *w,
                   double *out);
/* is_right_handed(n2, phi[deg, as the reference passes it], S, D, P) for in[n][5] -> out[n] (0/1)
 * (raytracer.f95:373-405; model-independent) */
int srt_is_right_handed(int64_t n, const double *in, int32_t *out);
/* dFdk(del=1e-8), dFdw(1e-8), dFdx(del), raytracer_evalrhs: out[n][14]  (raytracer.f95:118-314) */
int srt_gradients(srt_model *m, int64_t n, const double *x, const double *k, const double *w,
                  double del, double *out);
/* one rk4 and one rk45 step from args[n][7] with dt[n]: out[n][21] = rk4(7), out4(7), out5(7)
 * (raytracer.f95:504-596) */
int srt_rk_step(srt_model *m, int64_t n, const double *args, const double *dt, double del,
                double *out);
/* geopack's TRACE_08 (geopack2008.for:1649-1840), batched: the field line of T04_s + IGRF from x[n][3] (SM, metres) with the
 * AT64ThCh adapter's constants (DIR 1, DSMAX 1, ERR 1e-4, RLIM 60, R0 = (R_E + 400 km) / R_E), in default REAL like the Fortran.
 * out[n][6] = XF, YF, ZF (GSM, Earth radii), |IGRF| there (nT), how the line ended, TRACE_08's L (number of points).
 * Endings: 0 the foot on the sphere r = R0 (interpolated between the last two points), 1 the outer boundary (r > RLIM,
 * y^2 + z^2 > 1600 or x > 20), 2 more than four reversals of the radial direction, 3 no end within 500 points (NaN).
 * Works on a handle of any kind whose coefficient table is loaded (srt_model_set_field with use_igrf or use_tsyganenko, or a
 * modelnum-7 handle) and whose parmod is set (srt_model_set_tsyganenko_params, or a modelnum-7 handle): SRT_EINVAL otherwise. */
int srt_field_line_foot(srt_model *m, int64_t n, const double *x, double *out);
/* dumpmodel.f95: f[nz][ny][nx][4*nspec+3] = (qs, Ns, ms, nus, B0) of every node; file order (the Fortran's
 * f(:,i,j,k)).  Any of nx, ny, nz may be 1 (that axis sits at its minimum, as the Fortran's linspace does).
 * mag_coords = 1: each node goes through sm_to_mag_d for the model's date before the model sees it.
 * The nodes are formed on the device as the Fortran forms them, x(i) = i*del + min with del = (max - min)/(n - 1.0), and every
 * node's record is what srt_plasma_params returns at its coordinates (at srt_sm_to_mag of them for mag_coords = 1), bit for
 * bit, less the unused species slot: nspec = srt_model_nspec, 3 for modelnum 7 and 4 otherwise.  nus is all zeros, as in every
 * adapter of the reference.  The reference's dumpmodel reads --mag_coords for modelnum 6 and 7 only and leaves the variable
 * unset when the flag is absent (its toolchain zeroes it): DEFINED BEHAVIOUR here is that the caller always says 0 or 1, that an
 * absent flag is 0 (SM), and that the rotation is applied to a handle of any kind when asked for.
 * SRT_EINVAL, by name: an axis with fewer than 1 node, empty bounds (max <= min) on an axis of more than one node, more than
 * 2^31 - 1 nodes, mag_coords other than 0 or 1.  SRT_ENOMEM: the output does not fit on the device.
 * srt_last_kernel_ms afterwards gives the duration of the dump's launches. */
int srt_dump_model(srt_model *m, int nx, int ny, int nz, const double bounds[6], int mag_coords, double *f);
/* SM -> MAG (inverse = 0) or MAG -> SM (inverse = 1) for x[n][3], xform_double's sm_to_mag_d / mag_to_sm_d for
 * itime = (yearday, msec): seven plane rotations about the dipole tilt, the GSM, GSE, GEI and GEO angles of the date and the
 * pole's position, applied one after the other in the Fortran's order and arithmetic.  Pure host code, needs no GPU; the
 * device applies the same rotations, from the same sines and cosines, in srt_dump_model. */
int srt_sm_to_mag(int yearday, int msec, int inverse, int64_t n, const double *x, double *out);

/* ---- the hot path: replaces the driver's whole ray loop ---- */
/* slots per ray = ceil(maxsteps/outputper) */
int32_t srt_rows_per_ray(const srt_params *p);
/* Inputs pos0/dir0 [nrays][3], w0[nrays].  Outputs (caller-allocated host arrays):
 *   rows     [nrays][slots][SRT_ROW]   kept rows (row index r*outputper is stored in slot r)
 *   nrows    [nrays]                   total rows T the ray produced (= accepted steps + 1)
 *   stopcond [nrays]
 * accepted_steps (optional) receives sum(nrows-1).
 * One call per model at a time: the device staging of this entry point is owned by the model handle and reused from call
 * to call (grow-only; srt_model_trim() gives it back).  A second host thread calling it on the SAME model waits for the
 * first (per-model lock); different models run concurrently. */
int srt_trace_batch(srt_model *m, const srt_params *p, int64_t nrays, const double *pos0,
                    const double *dir0, const double *w0, double *rows, int32_t *nrows,
                    int32_t *stopcond, int64_t *accepted_steps);
/* Frees the grow-only device scratch a model has accumulated (host-buffer staging of srt_trace_batch, per-launch sort and
 * staging buffers); the tables stay.  The next call allocates what it needs again. */
int srt_model_trim(srt_model *m);
/* Same with every buffer already resident in device memory (what bench.py times).
 * d_pos0/d_dir0 are SoA on the device: [3][nrays].  stream = hipStream_t (NULL = default).
 * d_counters: 4 x int64 scratch/outputs: [0] queue head (zeroed by the call), [1] accepted steps,
 * [2] attempts, [3] wave-attempts (lane occupancy = [2] / (64 * [3])).  Asynchronous: returns after enqueue. */
int srt_trace_batch_device(srt_model *m, const srt_params *p, int64_t nrays, const double *d_pos0,
                           const double *d_dir0, const double *d_w0, double *d_rows,
                           int32_t *d_nrows, int32_t *d_stopcond, int64_t *d_counters, void *stream);
/* Packed form of a row buffer for transport (multi-GPU gather; the driver's own loop writes exactly
 * these rows, raytracer_driver.f95:1197): a ray keeps rows 0, outputper, 2*outputper, .. < nrows, i.e.
 * kept = (nrows-1)/outputper + 1 of its `slots` slots.  d_offsets[nrays+1] receives the exclusive prefix sums of the
 * kept counts (d_offsets[nrays] = total), d_packed[total][SRT_ROW] the kept rows of ray 0, ray 1, ... back to back.
 * capacity_rows = rows d_packed can hold (nrays*slots always suffices; 0 = offsets only).  If the total exceeds the
 * capacity, the rays that do not fit are left out: compare d_offsets[nrays] with the capacity after synchronising.
 * All pointers are device memory of ONE device -- the call finds that device from the buffers themselves (not from the
 * calling thread's binding), works there and leaves the thread's device as it found it; buffers on different devices or
 * host pointers fail with SRT_EINVAL.  `stream` must belong to the same device.  Asynchronous on `stream`. */
int srt_pack_rows_device(int32_t slots, int32_t outputper, int64_t nrays, const double *d_rows,
                         const int32_t *d_nrows, int64_t *d_offsets, double *d_packed, int64_t capacity_rows,
                         void *stream);
/* ---- the hot path in segments: bounded row memory, pause and resume ----
 * A launch of srt_trace_batch_device needs rows[nrays][slots][SRT_ROW] up front, whatever the rays turn out to need.  A
 * SEGMENTED trace runs the same rays as a sequence of launches.  With N = segment_rows and S = N * outputper, segment
 * s = 0, 1, .. owns the row indices [s S, (s + 1) S): a kept row r of that range goes to slot r / outputper - s N of a row
 * buffer [nrays][N][SRT_ROW].  A ray that has not stopped when it reaches the end of the range is PAUSED at the loop top,
 * behind the reference's own tests (t >= tmax, then the stop conditions: a ray at maxsteps stops with SRT_STOP_MAXSTEPS and is
 * never paused): nrows = (s + 1) S, stopcond = SRT_RUNNING, and its integrator state goes to its record of SRT_STATE doubles:
 *     [0..5] pos, k   [6..11] the right-hand side there (the carried first RK stage)   [12..14] vgrel   [15] t   [16] dt
 * The step counter travels in nrows; a ray can pause only right after an accepted step (or its launch), where the
 * controller's two flags are determined: no refinement pending, and "first attempt" exactly when nrows == 1.  The next
 * segment restores the record and the ray goes on as if it had never left its lane: the rows of a segmented trace, nrows and
 * stopcond are those of srt_trace_batch_device BIT FOR BIT, for every N and every model but one.
 * DEFINED BEHAVIOUR for modelnum 4 (scattered samples): a lane's block of candidate samples is forgotten when the lane takes a
 * ray, and the block's contents fix the order of the model's sums.  Segment 0 is bit-equal to the unsegmented launch; rows
 * behind the first pause agree to the rounding of a reordered sum, grown by the trajectory's own sensitivity.  nrows and
 * stopcond agree.  (Rebuilding the block about a saved centre would remove this; it is not done.) */
#define SRT_RUNNING (-1) /* stopcond of a paused ray */
#define SRT_STATE 17     /* doubles in a paused ray's record */
/* segments a segmented trace has at most = ceil(srt_rows_per_ray(p) / segment_rows); 0 for bad arguments.  Pure host code. */
int32_t srt_trace_segments(const srt_params *p, int32_t segment_rows);
/* One segment, beside srt_trace_batch_device (same inputs, same d_counters, same asynchrony).
 *   d_queue  segment 0: NULL, every ray is launched (ray_order applies here only).  Later segments: nqueue ray ids (int32),
 *            the rays to resume -- what srt_running_rays_device returned after the previous segment.  nqueue = 0 launches nothing.
 *   d_state[nrays][SRT_STATE], d_nrows[nrays], d_stopcond[nrays] persist from segment to segment; the entries of rays that
 *            are not in the queue are not touched.
 *   d_rows[nrays][segment_rows][SRT_ROW] receives this segment's kept rows (a ray's slot 0 is kept row segment * segment_rows).
 *   d_counters[1] = steps accepted in THIS launch; over all segments they sum to the unsegmented figure.
 * SRT_EINVAL, by name, before the device is touched: segment_rows < 1; segment_rows > srt_rows_per_ray(p); nrays >= 2^31;
 * segment < 0; a later segment without a queue; a queue in segment 0.  (After srt_trace_segments(p, segment_rows) segments
 * no ray is left running: every ray has stopped at maxsteps at the latest.) */
int srt_trace_segment_device(srt_model *m, const srt_params *p, int64_t nrays, const double *d_pos0, const double *d_dir0,
                             const double *d_w0, int32_t segment_rows, int32_t segment, const int32_t *d_queue,
                             int64_t nqueue, double *d_state, double *d_rows, int32_t *d_nrows, int32_t *d_stopcond,
                             int64_t *d_counters, void *stream);
/* d_queue[0 .. *d_count) = the ids of the rays with stopcond == SRT_RUNNING, ascending (a stable compaction); d_queue has room
 * for nrays ids, d_count is one int32 on the device.  The device is found from the buffers, as in srt_pack_rows_device.
 * Asynchronous on `stream`. */
int srt_running_rays_device(int64_t nrays, const int32_t *d_stopcond, int32_t *d_queue, int32_t *d_count, void *stream);
/* The host iterator over the segments of one launch set: device memory nrays * segment_rows rows (twice: traced and packed)
 * instead of nrays * slots, and only rows that exist reach the host.
 *   srt_trace_run_open   uploads the launch set (pos0 / dir0 [nrays][3], w0 [nrays], host) and allocates; no launch yet.
 *   srt_trace_run_next   runs the next segment; returns 1 and fills *seg, 0 when the run is over (no ray left running, or
 *                        srt_trace_segments(p, segment_rows) segments done -- the bound of every loop over it), < 0 on error.
 *   srt_trace_run_close  frees everything (NULL is allowed).
 * *seg is valid until the next call on the same run:
 *   nrays               rays that ran in this segment (all of them in segment 0)
 *   ray[nrays]          their ids, ascending
 *   offsets[nrays + 1]  exclusive prefix sums of their kept-row counts IN THIS SEGMENT
 *   rows[offsets[nrays]][SRT_ROW]  those rows, ray after ray: ray[i]'s kept rows number segment * segment_rows onwards
 *   nrows[nrays], stopcond[nrays]  each ray's rows so far and SRT_RUNNING or its stop code
 *   accepted_steps      steps accepted in this segment */
typedef struct srt_trace_run srt_trace_run;
typedef struct srt_segment {
  int32_t segment, reserved;
  int64_t nrays;
  const int32_t *ray;
  const int64_t *offsets;
  const double *rows;
  const int32_t *nrows;
  const int32_t *stopcond;
  int64_t accepted_steps;
} srt_segment;
int srt_trace_run_open(srt_model *m, const srt_params *p, int64_t nrays, const double *pos0, const double *dir0,
                       const double *w0, int32_t segment_rows, srt_trace_run **run);
int srt_trace_run_next(srt_trace_run *run, srt_segment *seg);
void srt_trace_run_close(srt_trace_run *run);
/* duration in ms of the most recent trace kernel on this model (or of the launches of the most recent srt_dump_model), measured
 * with HIP events on the stream it ran on (synchronises that stream) */
int srt_last_kernel_ms(srt_model *m, float *ms);
/* the same for the launch `back` launches before the most recent one (0 .. 3): lets a caller that keeps several
 * launches in flight on different streams read their durations afterwards */
int srt_launch_ms(srt_model *m, int back, float *ms);
/* The tail stash of that launch (unsegmented launches of the interp model, both layouts): while the queue has fresh rays every
 * wave banks a few of its own rays when their step count reaches 1/2, 3/4, 7/8, 15/16 of maxsteps, and finishes them in the
 * lanes that fall idle once the queue is empty.  Rows, nrows, stopcond and counters[0..2] are those of a launch without;
 * counters[3] (loop trips of all waves) gets smaller.  stats[SRT_STASH_STATS]: rays banked at each of the four marks, rays
 * resumed, the most records one wave held, loop trips run after a wave saw the queue empty (summed over the waves).  All zero
 * for a launch that banked nothing: no more rays than lanes, maxsteps < 32, another model, a segmented launch, a refused
 * allocation, or SRT_TAIL_STASH=0 in the environment (SRT_TAIL_STASH=n: at most n records per wave and mark; read per launch,
 * like SRT_MAX_BLOCKS=n, which caps the launch's number of waves).  Synchronises the launch's stream. */
#define SRT_STASH_STATS 7
int srt_launch_stash_stats(srt_model *m, int back, int64_t *stats);

/* ---- the step after the path: hot-plasma damping along the kept rows ----
 * Replaces the MATLAB post-processor matlab/damping/: test_dampray.m:24-99 (per-row driver, running magnitude),
 * spatialdamping.m / temporaldamping.m, hot_dispersion_imag.m (adaptive Gauss-Kronrod quadrature, quadva.m, of
 * integrand.m over vperp), fG1.m, fG2.m, suprathermal.m, maxwellboltzmann.m.  It consumes exactly the columns a kept
 * row holds (n, vgrel, pos, B0, Ns) plus the ray's w and the model's qs, ms; collisions are ignored as the scripts do.
 * One hot species (electrons: qh = -1.60217646e-19 C, mh = 9.10938188e-31 kg, const.m). */
typedef struct srt_damping_params {
  int32_t dist;    /* 0: suprathermal.m (Bell 2002); 1: Ne_h * maxwellboltzmann(vperp,vpar,ME,kT) */
  int32_t mode;    /* 0: spatial rate ki along vg (test_dampray.m); 1: temporal rate gamma (temporaldamping.m) */
  int32_t nres;    /* number of resonances, 1..8; 0 = the script's m = [-1 0 1] */
  int32_t m[8];    /* resonance orders (0 = Landau, +-1 = cyclotron) */
  double Ne_h, kT; /* dist 1: hot density in m^-3, temperature in J */
  double tol;      /* relative tolerance of the quadrature; 0 = the scripts' 1e-3 */
} srt_damping_params;
/* rows/nrows/w0 as returned by srt_trace_batch with the same slots = srt_rows_per_ray(p) and outputper.
 * Outputs [nrays][slots]: rate (ki along vg in 1/m, or gamma in 1/s; 0 in slot 0), magnitude (1 in slot 0, then
 * magnitude(i-1)*exp(-|pos_i - pos_{i-1}| ki_i) or *exp(gamma_i (t_i - t_{i-1})); 0 beyond the ray), flag (0 ok,
 * 1 quadrature stopped before its error test was met, 2 integrand not finite (rate = NaN), 3 k = 0 (the scripts'
 * "not solving evanescent mode": magnitude is 0 from there on)).  magnitude and flag may be NULL. */
int srt_damping(const srt_damping_params *dp, int nspec, const double *qs, const double *ms, int32_t slots,
                int32_t outputper, int64_t nrays, const double *rows, const int32_t *nrows, const double *w0,
                double *rate, double *magnitude, int32_t *flag);
/* the same on buffers already resident in device memory (the row buffer srt_trace_batch_device filled);
 * d_magnitude may be NULL, d_flag may not.  Asynchronous on `stream`. */
int srt_damping_device(const srt_damping_params *dp, int nspec, const double *qs, const double *ms, int32_t slots,
                       int32_t outputper, int64_t nrays, const double *d_rows, const int32_t *d_nrows,
                       const double *d_w0, double *d_rate, double *d_magnitude, int32_t *d_flag, void *stream);

/* ---- surface crossings along the kept rows: where and when each ray crosses a surface ----
 * No piece of the reference does this (matlab/ only plots); it is what users of many rays do next, on the device instead of a
 * host loop over the rows or a .ray file.  Input is the PACKED layout that srt_pack_rows_device, a segmented trace and
 * srt_read_ray_file produce: offsets[nrays + 1] (offsets[0] = 0) and rows[offsets[nrays]][SRT_ROW].
 * g(x) of a surface, x in SM metres as the rows are (R_E = 6371.2e3):
 *   kind 0, sphere             g = |x| - p[0]
 *   kind 1, dipole L-shell     g = |x|^3 - p[0] R_E (x^2 + y^2)      (no division on the axis; g > 0 <=> L > p[0])
 *   kind 2, magnetic latitude  g = z - |x| sin(p[0])                 (p[0] in radians; the sine is taken once, on the host)
 *   kind 3, plane              g = p[0] x + p[1] y + p[2] z - p[3]
 * The interval (i, i + 1) of a ray's consecutive kept rows holds an EVENT of surface s when (g_i < 0) != (g_{i+1} < 0): a row
 * exactly on the surface gives one event per pass, not two.  An interval with t_{i+1} == t_i, or with a non-finite t, pos or
 * vgrel at either end, holds none; a ray with fewer than two rows has none.  SAMPLING: an interval in which g changes sign twice
 * holds no event either -- the kept rows decide what can be seen, so outputper decides how often that happens.
 * Between the rows the ray is the cubic Hermite curve whose end slopes are the rows' own C vgrel, the right-hand side of the
 * position equation at the row (C as the models compute it, constants.f95:7).  With h = t1 - t0, D = p1 - p0, m0 = C vg0 h,
 * m1 = C vg1 h:   p(sigma) = p0 + sigma m0 + sigma^2 (3 D - 2 m0 - m1) + sigma^3 (m0 + m1 - 2 D).
 * Rows with vgrel = 0 (the n.n <= 0 rows) are used as they stand.  sigma* is a point of [0, 1] within 2^-50 of a sign change of
 * g(p(sigma)) that has the interval's end signs either side of it: 52 bisections of [0, 1], of whose last bracket the end with
 * g >= 0 is returned, deterministic, the same on host and device.
 * An event is a row of SRT_ROW doubles in the kept-row layout (t = t0 + sigma* h, pos = p(sigma*), columns 4 .. 19 -- vprel,
 * vgrel, n, B0, Ns -- linear in sigma*; srt_damping and the writers can take it as a row) and four int32: the ray, the surface's
 * index, the interval i (0-based among the ray's kept rows), and the direction (+1: g goes from < 0 to >= 0, else -1).
 * Events are ordered by (ray, interval, surface index).
 * SRT_EINVAL, by name, before the device is looked at: nsurf outside 1 .. SRT_MAXSURF, an unknown kind, a non-finite parameter,
 * a sphere radius <= 0, L <= 0, |latitude| >= pi/2, a zero plane normal; host offsets that decrease or do not start at 0. */
#define SRT_MAXSURF 16
typedef struct srt_surface {
  int32_t kind;
  int32_t reserved;
  double p[4];
} srt_surface;
/* On buffers resident in device memory (`surfaces` is host memory).  d_event_rows[capacity][SRT_ROW], d_event_meta[capacity][4],
 * d_count one int64: it always receives the total; events beyond `capacity` are left out (the first `capacity` events of the
 * defined order are kept).  capacity = 0 with NULL outputs is a count-only call.  The device is found from the buffers, as in
 * srt_pack_rows_device.  The call reads d_offsets[nrays] (8 bytes) behind the work already on `stream`, to size its launches,
 * and checks it against the allocation d_rows points into, runs its passes on `stream` and returns when they are done (its
 * scratch is freed then). */
int srt_crossings_device(int nsurf, const srt_surface *surfaces, int64_t nrays, const int64_t *d_offsets, const double *d_rows,
                         double *d_event_rows, int32_t *d_event_meta, int64_t capacity, int64_t *d_count, void *stream);
/* The same on host buffers; *event_rows[*nevents][SRT_ROW] and *event_meta[*nevents][4] are malloc'd (srt_free; NULL when there
 * are no events). */
int srt_crossings(int nsurf, const srt_surface *surfaces, int64_t nrays, const int64_t *offsets, const double *rows,
                  int64_t *nevents, double **event_rows, int32_t **event_meta);
/* One record per event, (4 i10, 20 es24.15e3): raynum[e] (the caller's number of the event's ray, e.g. raynum of
 * srt_read_ray_file indexed by the event's ray), surface index + 1, interval + 1, direction, then the event's row, formatted as
 * the .ray writer formats.  Pure host code, needs no GPU. */
int srt_crossings_file_write(const char *path, int64_t nevents, const int64_t *raynum, const int32_t *event_meta,
                             const double *event_rows);

/* ---- traced rays binned onto a grid: dwell time and power maps ----
 * No piece of the reference does this either (matlab/ only plots); it is what a million rays are traced for: how much ray
 * time, or damped wave power, lies in each cell of an (L, magnetic latitude) meridian grid, an (x, z) plane or an (r, latitude,
 * MLT) volume -- on the device, instead of a host loop over the rows.
 * INPUT: the PACKED layout of the crossings above, offsets[nrays + 1] and rows[offsets[nrays]][SRT_ROW], and two optional
 * weights: rowweight[offsets[nrays]], one per packed row (e.g. the square of srt_damping's magnitude), and rayweight[nrays]
 * (e.g. a source spectrum).  A NULL weight means 1.
 * SUB-SAMPLES: the interval (j, j + 1) of two consecutive kept rows of one ray is USABLE exactly when the crossings' rule says
 * so (t, pos, vgrel finite at both ends, t_{j+1} != t_j) and w_j, w_{j+1} and the ray's weight are finite.  A usable interval
 * is cut into nsub equal pieces of sigma (1 <= nsub <= 64); piece k = 0 .. nsub - 1 is one SAMPLE at sigma = (k + 1/2) / nsub,
 * at the position p(sigma) on the crossings' cubic Hermite curve, with the weight W = rayweight (w_j + sigma (w_{j+1} - w_j))
 * and the DEPOSIT d = W (h / nsub) seconds, h = t_{j+1} - t_j.
 * COORDINATES: the grid has 1 .. 3 axes; an axis is a coordinate function of x (SM metres, R_E = 6371.2e3) and n >= 1 cells
 * given by n + 1 strictly increasing finite edges; cell i holds edges[i] <= c < edges[i + 1].
 *   kind 0, 1, 2   x, y, z
 *   kind 3         r = |x|
 *   kind 4         rho = sqrt(x^2 + y^2)
 *   kind 5         dipole L = r^3 / (R_E rho^2)
 *   kind 6         s = z / r, the sine of the magnetic latitude (edges within [-1, 1])
 *   kind 7         MLT in hours = mod(24 phi / 2 pi + 12, 24), phi = atan2(y, x), as ngo_3d_dens_model_adapter takes it
 *                  (edges within [0, 24])
 * Kinds 0 .. 6 use only +, *, / and sqrt, products not fused into sums.
 * CELL INDEX: a sample with any coordinate outside its axis, or not finite (rho = 0 for L, r = 0 for s), is OUTSIDE and deposits
 * nothing.  The cell index is (i2 n1 + i1) n0 + i0.
 * ACCUMULATION: ticks[cell] += llrint(d / quantum), rounded to nearest even; quantum > 0 is finite (2^-30 s is a good default),
 * the accumulator is int64.  hits[cell] += 1.  An interval whose |d / quantum| >= 2^62 (or is not a number) at ANY of its
 * samples is skipped whole.
 * counters[4], int64: intervals used, intervals skipped (not usable, or a deposit too large), samples deposited, samples
 * outside.  deposited + outside = nsub * used; the sum of hits = deposited; used + skipped = the sum over rays of (rows - 1).
 * Cells hold INTEGERS so that the map is the same from run to run, from a host build and the device, for any launch geometry and
 * for any split of the rays over calls, segments or GPUs (int64 maps add exactly).  What follows from that:
 *   - a cell's sum wraps beyond 2^63 ticks: the caller chooses quantum accordingly (2^-30 s leaves 8.6e9 weighted seconds);
 *   - each deposit is rounded by at most quantum / 2;
 *   - as with crossings, what the kept rows do not show is not seen: the curve between two rows is the Hermite cubic, a sample
 *     is a point, and a piece that straddles a cell boundary goes whole to the cell of its midpoint.
 * SRT_EINVAL, by name, before a device is looked at: naxes outside 1 .. 3, nsub outside 1 .. 64, an unknown kind, n < 1 or
 * > 1024, NULL, non-finite or non-increasing edges, a kind-6 edge outside [-1, 1], a kind-7 edge outside [0, 24], a non-finite
 * or non-positive quantum, more than 2^31 - 1 cells, both outputs NULL, host offsets that decrease or do not start at 0. */
typedef struct srt_bin_axis {
  int32_t kind;
  int32_t n;
  const double *edges; /* host memory, n + 1 values */
} srt_bin_axis;
typedef struct srt_bin_params {
  int32_t naxes;
  int32_t nsub;
  double quantum;
  srt_bin_axis axis[3];
} srt_bin_params;
/* On buffers resident in device memory (`params` and its edges are host memory).  The call ACCUMULATES into d_ticks[ncells],
 * d_hits[ncells] (int64; either may be NULL, not both) and d_counters[4], which the caller zeroes: calls over shards, segments
 * or launch sets add up exactly.  The interval between the last row of one segment and the first of the next belongs to
 * neither packed set and is not binned (a carry across segments is the caller's).  The device is found from the buffers; the
 * call reads d_offsets[nrays] (8 bytes) behind the work already on `stream`, checks it against the allocation d_rows points
 * into, takes its scratch from hipMallocAsync, and from there on is asynchronous on `stream`.  Grids of up to 4096 cells are
 * accumulated in a block-private copy in LDS first, larger ones straight in device memory; the integers are the same. */
int srt_bin_rays_device(const srt_bin_params *params, int64_t nrays, const int64_t *d_offsets, const double *d_rows,
                        const double *d_rowweight, const double *d_rayweight, int64_t *d_ticks, int64_t *d_hits,
                        int64_t *d_counters, void *stream);
/* The same on host buffers: zeroes, runs, and returns malloc'd *ticks[ncells] and *hits[ncells] (srt_free; either pointer
 * argument may be NULL, not both) and counters[4]. */
int srt_bin_rays(const srt_bin_params *params, int64_t nrays, const int64_t *offsets, const double *rows, const double *rowweight,
                 const double *rayweight, int64_t **ticks, int64_t **hits, int64_t counters[4]);
/* The number of cells of a grid; validates `params` as the calls above do.  Host only. */
int srt_bin_cells(const srt_bin_params *params, int64_t *ncells);
/* A map as text.  Line 1: naxes, nsub (2 i10), quantum (es24.15e3).  Per axis two lines: kind, n (2 i10); its n + 1 edges
 * (es24.15e3 each).  Then one record per cell in index order: ticks * quantum (es24.15e3), hits (i20).  A NULL ticks or hits is
 * written as zeros.  The reader returns the grid (params->axis[a].edges point into the malloc'd *edges), *ncells and malloc'd
 * *sum[ncells] = ticks * quantum as the file keeps it and *hits[ncells] (srt_free all three), and refuses (SRT_EIO) a file that
 * is cut short or holds more than its header announces.  Pure host code, needs no GPU. */
int srt_bin_file_write(const char *path, const srt_bin_params *params, const int64_t *ticks, const int64_t *hits);
int srt_bin_file_read(const char *path, srt_bin_params *params, double **edges, int64_t *ncells, double **sum, int64_t **hits);

/* ---- closest approaches along the kept rows: which rays pass an observer point, when, how close, and in what state ----
 * No piece of the reference does this (matlab/ only plots).  A point is not a surface, so the crossings above cannot answer it.
 * Input is the PACKED layout of the crossings: offsets[nrays + 1] (offsets[0] = 0) and rows[offsets[nrays]][SRT_ROW].  Observers
 * are nobs (1 .. SRT_MAXOBS) entries of srt_observer: x in SM metres, radius in metres (the detection radius).
 * USABLE: the interval (j, j + 1) of one ray's consecutive kept rows is usable when the crossings' condition holds (t, pos and
 * vgrel finite at both ends, t_{j+1} != t_j) and t_{j+1} > t_j.
 * CURVE AND TEST FUNCTION: with the crossings' Hermite curve in its Delta form (h = t1 - t0, D = p1 - p0, m0 = C vg0 h,
 * m1 = C vg1 h, c2 = 3 D - 2 m0 - m1, c3 = m0 + m1 - 2 D):
 *   p(sigma) = p0 + sigma (m0 + sigma (c2 + sigma c3)),   p'(sigma) = m0 + sigma (2 c2 + 3 sigma c3),
 *   f(sigma) = (p(sigma) - o) . p'(sigma)     (half the derivative of the squared distance to the observer o),
 * every product and sum as written, unfused, summed x, y, z in that order.  At the ends f(0) = (p0 - o) . m0 and
 * f(1) = (p1 - o) . m1, from the rows themselves.
 * APPROACH: the interval holds an approach of observer m when f(0) < 0 and !(f(1) < 0): the ray is approaching at the start and
 * no longer approaching at the end.  sigma* comes from 52 halvings of [0, 1]: a step keeps lo = mid where f(mid) < 0, else
 * hi = mid; hi is returned.  A row exactly at the closest point therefore gives one event, at sigma = 1 of the interval before
 * it, and none in the next.  d = sqrt(sum (p(sigma*) - o)^2); the approach is an EVENT exactly when d <= radius.
 * An event is a row of SRT_ROW doubles in the kept-row layout exactly as a crossing's (t = t0 + sigma* h, pos = p(sigma*),
 * columns 4 .. 19 linear in sigma*), four int32 -- the ray, the observer's index, the interval (0-based among the ray's kept
 * rows), 0 -- and one double, d.  Events are ordered by (ray, interval, observer index).
 * SAMPLING -- what is NOT an event: a ray whose first kept row already recedes from the observer; a ray whose last kept row still
 * approaches it; an interval whose ends are both approaching or both not, whatever the curve does inside; an interval with a
 * non-finite t, pos or vgrel at either end, or with t_{j+1} <= t_j.  Rows with vgrel = 0 are used as they stand (f = 0 is "not
 * < 0").  The kept rows decide what can be seen, so outputper decides how often an approach is missed.
 * The definition has no early reject; the implementation's (the hull of the cubic's Bezier points against the radius) is
 * conservative and changes no event.
 * SRT_EINVAL, by name, before the device is looked at: nobs outside 1 .. SRT_MAXOBS, null observers, a non-finite coordinate, a
 * radius that is not finite or not > 0; host offsets that decrease or do not start at 0. */
#define SRT_MAXOBS 65536
typedef struct srt_observer {
  double x[3];
  double radius;
} srt_observer;
/* On buffers resident in device memory (`observers` is host memory).  d_event_rows[capacity][SRT_ROW], d_event_meta[capacity][4],
 * d_event_dist[capacity], d_count one int64: it always receives the total; events beyond `capacity` are left out (the first
 * `capacity` events of the defined order are kept).  capacity = 0 with NULL outputs is a count-only call.  The device is found
 * from the buffers, as in srt_pack_rows_device.  The call reads d_offsets[nrays] (8 bytes) behind the work already on `stream`,
 * to size its launches, and checks it against the allocation d_rows points into (at most 2^31 - 2 rows); it copies the
 * observers up, runs its passes on `stream` and returns when they are done (its scratch is freed then). */
int srt_approaches_device(int nobs, const srt_observer *observers, int64_t nrays, const int64_t *d_offsets, const double *d_rows,
                          double *d_event_rows, int32_t *d_event_meta, double *d_event_dist, int64_t capacity, int64_t *d_count,
                          void *stream);
/* The same on host buffers; *event_rows[*nevents][SRT_ROW], *event_meta[*nevents][4] and *event_dist[*nevents] are malloc'd
 * (srt_free; NULL when there are no events). */
int srt_approaches(int nobs, const srt_observer *observers, int64_t nrays, const int64_t *offsets, const double *rows,
                   int64_t *nevents, double **event_rows, int32_t **event_meta, double **event_dist);
/* One record per event, (4 i10, 21 es24.15e3): raynum[e] (the caller's number of the event's ray), observer index + 1,
 * interval + 1, 0, the distance, then the event's row, formatted as the .ray writer formats.  Pure host code, needs no GPU. */
int srt_approaches_file_write(const char *path, int64_t nevents, const int64_t *raynum, const int32_t *event_meta,
                              const double *event_dist, const double *event_rows);

/* ---- ray tubes: the cross-section a ray and two neighbour rays span, and with it geometric spreading ----
 * No piece of the reference does this (matlab/ only plots).  In geometric optics the power a ray carries divides by the
 * cross-section of the tube that the ray and its neighbours span; the power maps above weight by the damping alone.
 * INPUT: the PACKED layout of the crossings, offsets[nrays + 1] (offsets[0] = 0) and rows[offsets[nrays]][SRT_ROW], and
 * neighbours[nrays][2], int64, in HOST memory (as surfaces and observers are): for ray a the indices b, c of the two rays that
 * span its tube; -1, -1 means "ray a has no tube".
 * POSITION OF A NEIGHBOUR AT TIME t (t = column 0 of a centre row).  The neighbour ray has n kept rows r_0 .. r_{n-1}.
 *   1. Search: lo = 0, hi = n; while lo < hi: mid = lo + (hi - lo) / 2; if t_mid <= t then lo = mid + 1, else hi = mid;
 *      i = lo - 1.  A NaN t_mid compares false.  Nothing else is assumed about the order of the times.
 *   2. i < 0: there is no row at this time.
 *   3. t_i == t: q = pos_i as it stands, provided its three components are finite; if they are not, the result is unusable.  No
 *      curve and no interval are needed: a fixed-step trace, whose rays share their time stamps, never interpolates, and a
 *      neighbour of one row answers at its own time.
 *   4. Otherwise, i == n - 1: there is no row at this time (the neighbour stopped earlier).
 *   5. Otherwise the interval (i, i + 1) must be usable by the crossings' rule (t, pos, vgrel finite at both ends,
 *      t_{i+1} != t_i) and t_{i+1} > t; if not, the result is unusable.
 *   6. sigma = (t - t_i) / (t_{i+1} - t_i), and q = p(sigma) on the crossings' cubic Hermite curve of the interval, evaluated
 *      as p0 + sigma (m0 + sigma (c2 + sigma c3)).
 * SECTION: with p the centre row's position, d_b = q_b - p, d_c = q_c - p:
 *   Sigma = 1/2 (d_b x d_c), the area vector of the equal-group-time triangle, in m^2;
 *   A_perp = (Sigma . vg) / |vg|, vg the centre row's vgrel (columns 7 .. 9), |vg| = sqrt(vx^2 + vy^2 + vz^2).
 * Every product and sum is as written, unfused, summed x, y, z in that order; only + - * / and sqrt are used.  A_perp is
 * signed: a change of sign along a ray means the tube has folded (a caustic).  The flux of a tube that carries power P is
 * P magnitude^2 / |A_perp|, to first order in the tube's width.
 * OUTPUT per packed row: section[total][4] = (Sigma x, Sigma y, Sigma z, A_perp) and flag[total], int32.  The steps run in
 * this order and the first flag that is met is set -- neighbour b is examined before c:
 *   0  ok                                                                               all four values
 *   1  the ray has no tube                                                              four NaN
 *   2  the centre row's t or pos is not finite                                          four NaN
 *   3  a neighbour has no row at this time (no rows at all, before its first, after its last)   four NaN
 *   4  a neighbour's row or interval is unusable                                        four NaN
 *   5  vg has a component that is not finite, or |vg| as computed is 0 or not finite    Sigma written, A_perp NaN
 * Rows of different packed sets (the segments of a segmented trace, taken one by one) do not see each other: a neighbour row
 * that lies in another set is "no row at this time".  What the kept rows do not show is not seen: between its rows the
 * neighbour moves on the Hermite cubic.
 * SRT_EINVAL, by name, before a device is looked at: neighbours NULL, a pair with exactly one -1, an index outside
 * [0, nrays), b == c, b == a or c == a, both outputs NULL; host offsets that decrease or do not start at 0. */
/* On buffers resident in device memory (`neighbours` is host memory).  d_section[offsets[nrays]][4], d_flag[offsets[nrays]];
 * either may be NULL, not both.  The device is found from the buffers, as in srt_pack_rows_device.  The call reads
 * d_offsets[nrays] (8 bytes) behind the work already on `stream`, to size its launch, and checks it against the allocations
 * d_rows and the outputs point into (at most 2^31 - 2 rows); it copies the neighbours up, runs its pass on `stream` and
 * returns when it is done (the neighbours' copy is freed then). */
int srt_tubes_device(int64_t nrays, const int64_t *neighbours, const int64_t *d_offsets, const double *d_rows, double *d_section,
                     int32_t *d_flag, void *stream);
/* The same on host buffers; section[offsets[nrays]][4] and flag[offsets[nrays]] are the caller's (either may be NULL, not
 * both). */
int srt_tubes(int64_t nrays, const int64_t *neighbours, const int64_t *offsets, const double *rows, double *section, int32_t *flag);
/* One record per packed row whose flag is not 1, (3 i10, 5 es24.15e3): raynum[ray] (the caller's number of the row's ray), the
 * row's index among its ray's kept rows + 1, the flag, t, Sigma x, Sigma y, Sigma z, A_perp, formatted as the .ray writer
 * formats (NaN as that writer writes it).  A ray number outside 0 .. 9999999999 is refused.  Pure host code, needs no GPU. */
int srt_tubes_file_write(const char *path, int64_t nrays, const int64_t *raynum, const int64_t *offsets, const double *rows,
                         const double *section, const int32_t *flag);

/* ---- file formats of the boundary ---- */
/* ray input file: 7 list-directed reals per line (raytracer_driver.f95:1146); returns count, fills
 * malloc'd arrays the caller frees with srt_free */
int64_t srt_read_rays_file(const char *path, double **pos0, double **dir0, double **w0);
/* .ray writer, record format of raytracer_driver.f95:1197-1217; raynum0 = number of first ray (1).
 * qs/ms: the model's species constants (srt_model_species); pure host code, needs no GPU. */
int srt_write_ray_file(const char *path, int append, int64_t raynum0, int64_t nrays,
                       const srt_params *p, int nspec, const double *qs, const double *ms,
                       const double *w0, const double *rows, const int32_t *nrows,
                       const int32_t *stopcond);
/* The same file from the packed layout srt_read_ray_file returns and a segmented trace delivers: rows[offsets[nrays]][SRT_ROW]
 * = the kept rows of ray 0, ray 1, .. back to back, offsets[nrays + 1] their exclusive prefix sums (offsets[0] = 0).  One
 * formatting routine serves both writers: equal rows give equal bytes.  Pure host code, needs no GPU. */
int srt_write_ray_file_packed(const char *path, int append, int64_t raynum0, int64_t nrays, int nspec, const double *qs,
                              const double *ms, const double *w0, const int64_t *offsets, const double *rows,
                              const int32_t *stopcond);
/* .ray reader: the inverse of srt_write_ray_file, for files written by this library or by the reference's driver (what
 * matlab/readrayoutput.m is to the MATLAB damping scripts): returns the number of rays (< 0: error) and malloc'd arrays
 * (srt_free): raynum / stopcond / kept (records of the ray) / w0 per ray, rows[nrecords][SRT_ROW] = the kept rows of all rays
 * back to back (the packed layout of srt_pack_rows_device), plus the record's constants nspec, qs, ms.  Host code, no GPU. */
int64_t srt_read_ray_file(const char *path, int32_t *nspec, double qs[4], double ms[4], int64_t *nrecords,
                          int64_t **raynum, int32_t **stopcond, int32_t **kept, double **w0, double **rows);
void srt_free(void *p);

/* model-3 grid files, the step before the path: the text format written by
 * gcpm_dens_model_buildgrid.f95:302-327 and read by interp_dens_model_adapter.f95:58-117, and a binary
 * side-format ("SRTGRID1": 144-byte header {magic, compder, nspec, nx, ny, nz, bounds[6], qs[4], ms[4]} + the
 * same value blocks as raw little-endian doubles) for grids whose text takes longer to parse than to trace.
 * srt_model_create_interp_file() accepts either (detected by the magic).  Pure host code, needs no GPU.
 *   dims = {compder, nspec, nx, ny, nz}; F[nz][ny][nx][nspec]; derivs = 7 blocks of F's shape, concatenated
 *   (dfdx dfdy dfdz d2fdxdy d2fdxdz d2fdydz d3fdxdydz), or NULL.  *F / *derivs are malloc'd: srt_free(). */
int srt_grid_file_read(const char *path, int32_t dims[5], double bounds[6], double qs[4], double ms[4],
                       double **F, double **derivs);
int srt_grid_file_write(const char *path, int binary, int nspec, int nx, int ny, int nz,
                        const double bounds[6], const double *qs, const double *ms, const double *F,
                        const double *derivs);
int srt_grid_file_convert(const char *in_text_or_binary, const char *out_binary);
int srt_grid_file_is_binary(const char *path);

/* model-4 sample files: the text format written by gcpm_dens_model_buildgrid_random.f95:196-225 (+ helper
 * module :37-43) and read by scattered_interp_dens_model_adapter.f95:85-133, and a binary side-format ("SRTPTS01":
 * 136-byte header {magic, nspec, 0, npts, bounds[6], qs[4], ms[4]} + npts records of 3 + nspec raw doubles).
 * srt_model_create_scattered_file() accepts either (detected by the magic).  records = [npts][3 + nspec]
 * "x y z lnN_1 .. lnN_nspec", e.g. the output of srt_build_samples.  Pure host code, needs no GPU. */
int srt_points_file_write(const char *path, int binary, int nspec, int64_t npts, const double bounds[6],
                          const double *qs, const double *ms, const double *records);
int srt_points_file_convert(const char *in_text, const char *out_binary);
int srt_points_file_is_binary(const char *path);

/* dump files, the output of the reference's dumpmodel (dumpmodel.f95:1284-1292) and of srt_dump_model: one (5i10) record
 * nspec nx ny nz, one (6es24.15e3) record minx maxx miny maxy minz maxz, then every value of f[nz][ny][nx][4*nspec+3] on a
 * line of its own, (es24.15e3), in array order.  The writer is byte-exact against the reference.  The reader returns
 * dims = {nspec, nx, ny, nz} and a malloc'd *f (srt_free) and refuses (SRT_EIO) a file whose value count is not the
 * (4 nspec + 3) nx ny nz of its header.  Text only.  Pure host code, needs no GPU. */
int srt_dump_file_write(const char *path, int nspec, int nx, int ny, int nz, const double bounds[6], const double *f);
int srt_dump_file_read(const char *path, int32_t dims[4] /* nspec nx ny nz */, double bounds[6], double **f /* srt_free */);

#ifdef __cplusplus
}
#endif
#endif
