// lrnde_stepctl.hpp — the scalar arithmetic of every adaptive loop (device + host), stated once: OrdinaryDiffEq's PI
// step-size controller, the accept snap onto the end time, the proposal floor, loopheader!'s clamp and status checks,
// ode_determine_initdt's dt0 rule and tail, and the SDE loops' controller on the grid of the caller's Brownian path
// (DESIGN.md §2 lists which loop uses which form).
//
// Like lrnde_math.hpp: fixed sequences of IEEE-754 fp32 operations (pow / log10 in fp64 where upstream calls libm),
// compiled with -ffp-contract=off, so an expression has the same bits wherever it is inlined.  Everything takes and
// returns values (the host loops' AttemptLoop and TstopCursor are such values, advanced in place) and makes no HIP call;
// counters, trace rows, save and record bookkeeping stay with the loops.
#pragma once
#include <math.h>
#include <stddef.h>

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

// ---- the attempt loop of a host-controlled solve, stated once ----
// The state machine around the pieces above, in the order that matters to the bit: q11 survives a reject, qold changes
// only on an accept, iter counts an attempt before header_status sees it, a NaN estimate stops the loop before the
// controller runs.  A loop is
//   AttemptLoop L = attempt_begin(...);
//   while (L.t < t1) { [swap buffers if L.iter > 0 && L.accept]  if (!attempt_header(L, tend)) break;
//                      [a step of L.dt from L.t -> eest]  attempt_judge(L, eest);  if (L.status) break;  [bookkeeping] }
// and L.status is its retcode.  snap_mag: 0 = snap_signed (the forward loops), 1 = snap_magnitude (reversed time, Adams).
// The device loops keep this state in their double-buffered control blocks and call the pieces themselves.
struct AttemptLoop {
  PiConsts pi; int exact_pow, maxiters; int snap_mag;
  float t, dt, dtpropose, dtmax, dtmin, qold, q11;
  float tend;   // the end time the last header clamped to: the one an accepted step snaps onto
  int accept, iter, status;
};
LRNDE_HD AttemptLoop attempt_begin(const PiConsts pi, int exact_pow, int maxiters, int snap_mag, float t0, float t1, float dt_init) {
  AttemptLoop L;
  L.pi = pi; L.exact_pow = exact_pow; L.maxiters = maxiters; L.snap_mag = snap_mag;
  L.t = t0; L.dt = L.dtpropose = dt_init;
  L.dtmax = t1 - t0;
  L.dtmin = fmaxf_(eps_f(t1), eps_f(t0));
  L.qold = QOLDINIT; L.q11 = 1.0f;
  L.tend = t1;
  L.accept = L.iter = 0; L.status = STEP_OK;
  return L;
}
// the dt of the next attempt towards tend (a tstop, or the end of the span); false: there is none, L.status says why
LRNDE_HD bool attempt_header(AttemptLoop& L, float tend) {
  if (L.iter > 0) L.dt = L.accept ? L.dtpropose : pi_reject_dt(L.pi, L.dt, L.q11);
  ++L.iter;
  L.tend = tend;
  L.dt = header_clamp(L.dt, L.dtmax, L.dtmin, L.t, tend);
  L.status = header_status(L.iter, L.maxiters, L.dt, L.dtmin);
  return L.status == STEP_OK;
}
// the attempt's error estimate: accepted (L.t moves, L.dtpropose is the next dt) or not; L.dt stays the attempted step
LRNDE_HD bool attempt_judge(AttemptLoop& L, float eest) {
  if (eest != eest) { L.status = STEP_DT_NAN; L.accept = 0; return false; }
  const PiStep ps = pi_step(L.pi, L.exact_pow, eest, pi_pow(L.exact_pow, L.qold, L.pi.beta2), L.q11);
  L.q11 = ps.q11;
  L.accept = (eest <= 1.0f);
  if (L.accept) {
    L.qold = pi_qold(eest);
    L.t = L.snap_mag ? snap_magnitude(L.t, L.dt, L.tend) : snap_signed(L.t, L.dt, L.tend);
    L.dtpropose = pi_propose(L.dt, ps.q, L.dtmax, dt_floor(L.t, L.dtmin));
  }
  return L.accept;
}

// ---- the SDE loops' controller on the grid of the caller's Brownian path ----
// Steps are whole grid intervals of length h: position i, step length m intervals, at least one.  dtc: the proposal as a
// REAL number; the step taken is its floor on the grid.  Growth accumulates in dtc — with qmax = 1.125 a proposal quantised
// after every step could never leave m = 1.  The block is the device loops' control block (cur: which of the two state
// buffers is current) and the host loop's state.  status: STEP_OK while running, STEP_DONE at the end of the grid, else an
// lrnde_status error (STEP_CAPACITY is LRNDE_CAPACITY; asserted where the headers meet).
enum { STEP_CAPACITY = 5, STEP_DONE = 100 };
struct SdeCtl { int status, i, m, cur, naccept, nreject, iters, nf; float qold, eest_last, dtc; };
struct SdeGrid { PiConsts pi; float h; int nfine, maxiters; };
// a fresh solve: dt0 quantised to the grid; iters counts the first attempt (the caller refuses maxiters < 1)
LRNDE_HD SdeCtl sde_grid_begin(float dt0, float h, int nfine) {
  int m0 = (int)(dt0 / h); if (m0 < 1) m0 = 1;
  if (m0 > nfine) m0 = nfine;
  SdeCtl c;
  c.status = STEP_OK; c.i = 0; c.m = m0; c.cur = 0; c.naccept = 0; c.nreject = 0; c.iters = 1; c.nf = 0;
  c.qold = QOLDINIT; c.eest_last = 0.f; c.dtc = dt0;
  return c;
}
// One attempt's verdict.  eest, dt: the attempt's estimate and length; qpow = fastpow(c.qold, g.pi.beta2) (it does not depend on
// eest: a loop that waits for the estimate computes it meanwhile); nfa: the attempt's drift evaluations, what nf counts;
// rec_cap: slots of the caller's record of accepted steps, negative for none.  The caller writes what the result names, with
// the i and m the block held BEFORE the call: trace row `trace` (-1: none, a NaN estimate) and the pair (i, m) into record
// slot `rec` (-1: none).  An accepted step that finds the record full sets STEP_CAPACITY and is still counted (naccept, i),
// iters is not, and neither STEP_DONE nor STEP_MAXITERS replaces the status.
struct SdeVerdict { int accepted, rec, trace; };
LRNDE_HD SdeVerdict sde_grid_update(SdeCtl& c, float eest, float dt, float qpow, int nfa, const SdeGrid g, int rec_cap) {
  SdeVerdict v = {0, -1, -1};
  c.nf += nfa; c.eest_last = eest;
  if (eest != eest) { c.status = STEP_DT_NAN; return v; }
  const float q = pi_step(g.pi, 0, eest, qpow, 1.0f).q;
  v.accepted = eest <= 1.0f;
  v.trace = c.naccept + c.nreject;
  c.dtc = (v.accepted ? fmaxf_(c.dtc, dt) : dt) / q;
  int mnew = (int)(c.dtc / g.h);
  if (mnew < 1) mnew = 1;
  if (v.accepted) {
    if (rec_cap >= 0) {
      if (c.naccept < rec_cap) v.rec = c.naccept;
      else c.status = STEP_CAPACITY;
    }
    c.naccept++;
    c.qold = pi_qold(eest);
    c.i += c.m;
    c.cur ^= 1;
    c.m = mnew;
    if (c.i >= g.nfine && c.status == STEP_OK) c.status = STEP_DONE;
  } else {
    c.nreject++;
    if (c.m == 1) c.status = STEP_DT_LESS_THAN_MIN;  // the path's grid cannot be refined further
    else c.m = mnew < c.m ? mnew : c.m - 1;
  }
  if (c.status == STEP_OK) {
    if (c.m > g.nfine - c.i) c.m = g.nfine - c.i;
    if (++c.iters > g.maxiters) c.status = STEP_MAXITERS;
  }
  return v;
}

// ---- tstops of a solve over (s0, s1), ascending: the end time of the attempt that starts at t ----
// Entries <= t are passed (so are those <= s0 on the first call, and equal ones together); the next one is the stop if
// it lies strictly before s1, else s1 is.  t never decreases between calls.
struct TstopCursor { const float* tstops; size_t n, i; };
LRNDE_HD float tstop_next(TstopCursor& c, float t, float s1) {
  while (c.i < c.n && c.tstops[c.i] <= t) ++c.i;
  return (c.i < c.n && c.tstops[c.i] < s1) ? c.tstops[c.i] : s1;
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
