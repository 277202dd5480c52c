// lrnde_stepctl.hpp — the scalar arithmetic of every adaptive loop (device + host), stated once: OrdinaryDiffEq's PI
// step-size controller, the accept snap onto the end time, the proposal floor, loopheader!'s clamp and status checks,
// and ode_determine_initdt's dt0 rule and tail (DESIGN.md §2 lists which loop uses which form).
//
// Like lrnde_math.hpp: fixed sequences of IEEE-754 fp32 operations (pow / log10 in fp64 where upstream calls libm),
// compiled with -ffp-contract=off, so an expression has the same bits wherever it is inlined.  Everything takes and
// returns values; counters, trace rows, save and record bookkeeping stay with the loops.
#pragma once
#include <math.h>

#include "lrnde_math.hpp"

namespace lrnde {

// ---- PI controller ----
struct PiConsts { float gamma, qmin, qmax, beta1, beta2; };
// Tsit5 (order 5): beta1 = 7/50, beta2 = 2/25.  VCAB3 / VCABM3 (order 3): 7/30, 2/15.  The SDE loops fill the struct
// from the caller's options.
LRNDE_HD PiConsts pi_tsit5() { return {0.9f, 0.2f, 10.0f, (float)(7.0 / 50.0), (float)(2.0 / 25.0)}; }
LRNDE_HD PiConsts pi_order3() { return {0.9f, 0.2f, 10.0f, (float)(7.0 / 30.0), (float)(2.0 / 15.0)}; }
constexpr float QOLDINIT = 1e-4f;  // qold of a fresh integrator and its floor after an accepted step (qoldinit)

LRNDE_HD float pi_pow(int exact_pow, float x, float y) { return exact_pow ? (float)pow((double)x, (double)y) : fastpow(x, y); }

// The step factor q (dt_new = dt / q) from the error estimate.  qold_pow = pi_pow(exact_pow, qold, k.beta2) is an
// argument: it does not depend on eest, and the loops that wait for a norm compute it while they wait.  q11 goes in as
// the previous attempt's value and comes out unchanged when eest == 0.
struct PiStep { float q, q11; };
LRNDE_HD PiStep pi_step(const PiConsts k, int exact_pow, float eest, float qold_pow, float q11) {
  PiStep s;
  s.q11 = q11;
  if (eest == 0.0f) {
    s.q = 1.0f / k.qmax;
  } else {
    s.q11 = pi_pow(exact_pow, eest, k.beta1);
    s.q = s.q11 / qold_pow;
    s.q = fmaxf_(1.0f / k.qmax, fminf_(1.0f / k.qmin, s.q / k.gamma));
  }
  return s;
}
LRNDE_HD float pi_qold(float eest) { return fmaxf_(eest, QOLDINIT); }  // after an accepted step
LRNDE_HD float pi_reject_dt(const PiConsts k, float dt, float q11) { return dt / fminf_(1.0f / k.qmin, q11 / k.gamma); }
// dtpropose after an accepted step that ended at t
LRNDE_HD float dt_floor(float t, float dtmin) { return fmaxf_(eps_f(t), dtmin); }
LRNDE_HD float pi_propose(float dt, float q, float dtmax, float floor) { return fmaxf_(fminf_(dtmax, dt / q), floor); }

// ---- the accepted step's new time: t + dt, or tend when within 100 eps of it ----
// Two forms that differ for negative times and are both kept: the forward loops take eps at the signed maximum of the
// two times (upstream's expression); the reversed-time and Adams loops at the larger magnitude (s = -t <= 0: the signed
// maximum is the time nearer zero, whose eps is far below the rounding of t + dt).
LRNDE_HD float snap_signed(float t, float dt, float tend) {
  const float ttmp = t + dt;
  return (__builtin_fabsf(ttmp - tend) < 100.0f * eps_f(fmaxf_(t, tend))) ? tend : ttmp;
}
LRNDE_HD float snap_magnitude(float t, float dt, float tend) {
  const float ttmp = t + dt;
  return (__builtin_fabsf(ttmp - tend) < 100.0f * eps_f(fmaxf_(__builtin_fabsf(t), __builtin_fabsf(tend)))) ? tend : ttmp;
}

// ---- loopheader!: the dt of the next attempt, and whether there is one ----
LRNDE_HD float header_clamp(float dt, float dtmax, float dtmin, float t, float tend) {
  dt = fminf_(dtmax, dt);
  dt = fmaxf_(dt, dtmin);
  return fminf_(__builtin_fabsf(dt), __builtin_fabsf(tend - t));
}
// STEP_OK: take the step.  iter counts this attempt.  The values are lrnde.h's LRNDE_OK, LRNDE_MAXITERS,
// LRNDE_DT_LESS_THAN_MIN and LRNDE_DT_NAN (asserted where both headers meet), so a loop stores the result as its status.
enum { STEP_OK = 0, STEP_MAXITERS = 1, STEP_DT_LESS_THAN_MIN = 2, STEP_DT_NAN = 3 };
LRNDE_HD int header_status(int iter, int maxiters, float dt, float dtmin) {
  if (iter > maxiters) return STEP_MAXITERS;
  if (dt != dt) return STEP_DT_NAN;
  if (__builtin_fabsf(dt) <= __builtin_fabsf(dtmin)) return STEP_DT_LESS_THAN_MIN;
  return STEP_OK;
}

// ---- ode_determine_initdt from its three norms ----
LRNDE_HD float initdt_dt0(float d0, float d1, float dtmax) {
  const float dt0 = ((double)d0 < 1e-5 || (double)d1 < 1e-5) ? 1e-6f : (d0 / d1) / 100.0f;
  return fminf_(dt0, dtmax);
}
// d2: the norm of f(u + dt0 f0) - f0, not yet divided by dt0.  order: 5 (Tsit5), 3 (Adams), alg order + 1/2 (SDE).
LRNDE_HD float initdt_tail(float dt0, float d1, float d2, float order, float dtmax) {
  const float maxd = fmaxf_(d1, d2 / dt0);
  float dt1;
  if ((double)maxd <= 1e-15) {
    dt1 = fmaxf_(1e-6f, dt0 * 1e-3f);
  } else {
    const float l10 = (float)log10((double)maxd);
    const float e = (-(2.0f + l10)) / order;
    dt1 = (float)pow(10.0, (double)e);
  }
  return fminf_(fminf_(100.0f * dt0, dt1), dtmax);
}

}  // namespace lrnde
