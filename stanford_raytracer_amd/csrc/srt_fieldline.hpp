// srt_fieldline.hpp -- geopack's field-line tracer (geopack2008.for: RHAND_08 :1545-1572, STEP_08 :1576-1645, TRACE_08
// :1649-1840) restated in default REAL (fp32), operation for operation: the Fortran's order of evaluation is kept and
// products are not fused into sums (fp contract off in every function).
//
// The field is a functor, field(x, y, z, bx, by, bz) = EXNAME + INNAME at a GSM position in Earth radii, so that the same
// source compiles for the device (T04_s + the wave's IGRF synthesis, srt_at64thch.hpp) and for the host (tests/native).
//
// Organised for a wave: TRACE_08's point loop and STEP_08's halving loop are ONE flat loop whose trip is one Runge-Kutta-
// Merson attempt (five field evaluations) of every lane.  The device's IGRF synthesis reads its terms by v_readlane and may
// only run in wave-uniform control flow (srt_device.hpp), so the field is evaluated by all lanes in every trip, the loop
// ends when the ballot says that every lane has ended, and a lane that has ended holds its state.
//
// Defined behaviour where the Fortran has none:
//  * TRACE_08's check of L against LMAX is commented out (:1762) and its caller's arrays hold 500 points.  No point is
//    stored here; a line that has not ended after LMAX points ends with END_LIMIT and a NaN foot.
//  * STEP_08 halves its step for as long as the error estimate says so.  Here at most MAXHALVE times per point (fp32's
//    0.5 reaches zero after 150 halvings, where the Fortran would accept a step of no length); then END_LIMIT too.
//  No loop depends on the data for its termination: the flat loop has the product of the two bounds as its trip count.
//  * XR, YR, ZR (the previous point) are unset when the very first point already lies inside R0; here they are the start.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define FL_HD __host__ __device__
#else
#define FL_HD
#endif
#if defined(__clang__)
#define FL_NOCONTRACT _Pragma("clang fp contract(off)")
#else
#define FL_NOCONTRACT // (g++: built with -ffp-contract=off)
#endif

namespace srt {
namespace fl {

constexpr int LMAX = 500;    // AT64ThCh_adapter.f95:99,191
constexpr int MAXHALVE = 64; // halvings of one step

// how a line ended
enum Ending {
  END_SPHERE = 0,    // crossed r = R0 from outside: the foot, by linear interpolation between the last two points
  END_OUTER = 1,     // r > RLIM, y^2 + z^2 > 1600 or x > 20: the point where that was seen
  END_REVERSALS = 2, // more than four changes of the radial direction: the point where that was seen
  END_LIMIT = 3      // LMAX points or MAXHALVE halvings: NaN
};

struct TraceConst {
  float dir, dsmax, err, rlim, r0;
  int lmax;
};
struct Foot {
  float x, y, z;
  int kind, npts; // npts: TRACE_08's L (LMAX + 1 when the points ran out)
};

// true when every lane of the wave has ended (host: this one line)
FL_HD static inline bool all_ended(bool done) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __ballot(!done) == 0ull;
#else
  return done;
#endif
}

// RHAND_08: the right-hand side of the field-line equation, DS3 * B / |B|
template <class F>
FL_HD static inline void rhand(const F &field, float ds3, float x, float y, float z, float &r1, float &r2, float &r3) {
  FL_NOCONTRACT
  float bx, by, bz;
  field(x, y, z, bx, by, bz);
  const float b = ds3 / sqrtf(bx * bx + by * by + bz * bz);
  r1 = bx * b;
  r2 = by * b;
  r3 = bz * b;
}

// TRACE_08 from (xi, yi, zi).  live = false: this lane has no line to trace (it rides along and returns its start).
template <class F>
FL_HD static inline Foot trace(const F &field, const TraceConst &c, float xi, float yi, float zi, bool live) {
  FL_NOCONTRACT
  int L = 0, nrev = 0, nhalve = 0, kind = END_LIMIT;
  float ds = 0.5f * c.dir;
  float x = xi, y = yi, z = zi;
  // the first RHAND_08 call only decides the sign of AD; TRACE_08's DD and STEP_08's DS3 are the same word: DS3 = DIR here
  float r1, r2, r3;
  rhand(field, c.dir, x, y, z, r1, r2, r3);
  float ad = 0.01f;
  if (x * r1 + y * r2 + z * r3 < 0.f) ad = -0.01f;
  float rr = sqrtf(x * x + y * y + z * z) + ad;
  float xr = x, yr = y, zr = z, drp = 0.f;
  bool done = !live, newpoint = true;
  const int maxtrips = c.lmax * (MAXHALVE + 2) + 1;
  for (int trip = 0; trip < maxtrips; ++trip) {
    if (!done && newpoint) { // label 1: a new point of the line
      L = L + 1;
      const float ryz = y * y + z * z;
      const float r = sqrtf(x * x + ryz);
      if (L > c.lmax) {
        done = true;
        kind = END_LIMIT;
        x = y = z = NAN;
      } else if (r > c.rlim || ryz > 1600.f || x > 20.f) {
        done = true;
        kind = END_OUTER;
      } else if (r < c.r0 && rr > r) { // label 6
        const float q = (c.r0 - r) / (rr - r);
        x = x - (x - xr) * q;
        y = y - (y - yr) * q;
        z = z - (z - zr) * q;
        done = true;
        kind = END_SPHERE;
      } else {
        if (!(r >= rr || r >= 3.f)) { // inward inside r = 3: smaller steps towards the sphere
          float fc = 0.2f;
          if (r - c.r0 < 0.05f) fc = 0.05f;
          const float al = fc * (r - c.r0 + 0.2f);
          ds = c.dir * al;
        }
        xr = x;
        yr = y;
        zr = z;
        drp = r - rr;
        rr = r;
        newpoint = false;
        nhalve = 0;
      }
    }
    if (all_ended(done)) break;
    // STEP_08, one attempt (every lane evaluates the field; a lane that has ended changes nothing)
    const float ds3 = -ds / 3.f;
    float r11, r12, r13, r21, r22, r23, r31, r32, r33, r41, r42, r43, r51, r52, r53;
    rhand(field, ds3, x, y, z, r11, r12, r13);
    rhand(field, ds3, x + r11, y + r12, z + r13, r21, r22, r23);
    rhand(field, ds3, x + .5f * (r11 + r21), y + .5f * (r12 + r22), z + .5f * (r13 + r23), r31, r32, r33);
    rhand(field, ds3, x + .375f * (r11 + 3.f * r31), y + .375f * (r12 + 3.f * r32), z + .375f * (r13 + 3.f * r33), r41, r42, r43);
    rhand(field, ds3, x + 1.5f * (r11 - 3.f * r31 + 4.f * r41), y + 1.5f * (r12 - 3.f * r32 + 4.f * r42),
          z + 1.5f * (r13 - 3.f * r33 + 4.f * r43), r51, r52, r53);
    if (!done) {
      const float errcur = fabsf(r11 - 4.5f * r31 + 4.f * r41 - .5f * r51) + fabsf(r12 - 4.5f * r32 + 4.f * r42 - .5f * r52) +
                           fabsf(r13 - 4.5f * r33 + 4.f * r43 - .5f * r53);
      if (errcur > c.err) { // repeat with half the step
        ds = ds * .5f;
        nhalve = nhalve + 1;
        if (nhalve > MAXHALVE) {
          done = true;
          kind = END_LIMIT;
          x = y = z = NAN;
        }
      } else if (fabsf(ds) > c.dsmax) { // repeat with DSMAX
        ds = copysignf(c.dsmax, ds);
      } else { // label 2: the step
        x = x + .5f * (r11 + 4.f * r41 + r51);
        y = y + .5f * (r12 + 4.f * r42 + r52);
        z = z + .5f * (r13 + 4.f * r43 + r53);
        if (errcur < c.err * .04f && ds < c.dsmax / 1.5f) ds = ds * 1.5f;
        const float r = sqrtf(x * x + y * y + z * z);
        const float dr = r - rr;
        if (drp * dr < 0.f) nrev = nrev + 1;
        if (nrev > 4) {
          done = true;
          kind = END_REVERSALS;
        }
        newpoint = true;
      }
    }
  }
  if (!done) { // (not reached: the per-lane bounds end every lane within maxtrips)
    kind = END_LIMIT;
    x = y = z = NAN;
  }
  Foot f;
  f.x = x;
  f.y = y;
  f.z = z;
  f.kind = kind;
  f.npts = L;
  return f;
}

} // namespace fl
} // namespace srt
