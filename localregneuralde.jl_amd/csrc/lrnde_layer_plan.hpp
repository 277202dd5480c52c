// lrnde_layer_plan.hpp — the bookkeeping of `(n::NeuralODE)(x, ps, st)` / `(n::NeuralDSDE)(...)` that every layer forward
// shares, stated once (src/layers/neural_ode.jl:56-116, src/utils.jl:31-33): the `saveat` the global
// solve gets for :none / :unbiased / :biased, the save slot that will hold sol(t1), the index one uniform draw selects
// in :biased, the entries _CorrectedDESolution removes from the caller's series, the stop list of the backward pass, and
// the SDE layer's series on its accepted steps (save_start rule, interpolated entries, where the local step starts).
//
// Like lrnde_stepctl.hpp: values in, values out, no HIP call and no handle, so the host compiler builds it alone
// (tests/test_host_layer_plan.py).  The MLP / Dense-chain handles (lrnde_kernels.hip), the conv handle (lrnde_conv.hip)
// and the SDE layer (lrnde_sde_node.hpp) call it.
#pragma once
#include <algorithm>
#include <vector>

#include "lrnde.h"

namespace lrnde {

// ---- the solve's saveat for a mode ----
// user / nuser: the layer's own `saveat` kwarg (ascending; nuser == 0: none).
//   :none      the user's saveat, or [t2]
//   :unbiased  [t1, t2], or the user's saveat with t1 behind any entries equal to it (vcat(saveat, t1), sorted stably);
//              the caller's series then leaves the entries at t1 out again (needs_correction)
//   :biased    the user's saveat, or nothing and every accepted step
struct SolveSaveat {
  std::vector<float> saveat;
  int save_everystep = 0;
  bool needs_correction = false;
};
inline SolveSaveat solve_saveat(int mode, float t1, float t2, const float* user, int nuser) {
  SolveSaveat p;
  if (nuser > 0) p.saveat.assign(user, user + nuser);
  if (mode == LRNDE_MODE_UNBIASED) {
    if (nuser > 0) { p.saveat.insert(std::upper_bound(p.saveat.begin(), p.saveat.end(), t1), t1); p.needs_correction = true; }
    else p.saveat = {t1, t2};
  } else if (nuser == 0) {
    if (mode == LRNDE_MODE_BIASED) p.save_everystep = 1;
    else p.saveat = {t2};
  }
  return p;
}

// ---- :biased: t1 = rand(sol.t[1:(end - 1)]) from one uniform draw r, m = length(sol.t) - 1 >= 1 (the caller's check) ----
inline int biased_pick(float r, int m) {
  int idx = (int)(r * (float)m);
  if (idx >= m) idx = m - 1;
  if (idx < 0) idx = 0;
  return idx;
}

// ---- _CorrectedDESolution: `sol.u[t1 .!= sol.t]`, only where t1 was added to the user's saveat (a NaN t1 drops nothing) ----
inline bool series_keeps(bool needs_correction, float t1, float t) { return !(needs_correction && t == t1); }

// ---- the NeuralDSDE layer's series on the accepted steps of its solve (src/layers/neural_sde.jl:50-123) ----
// sol.t / sol.u as StochasticDiffEq would hold them (UPSTREAM-RECALL): accepted step k covers im[k].x .. im[k].x + im[k].y on
// the path's grid of nfine intervals over (t0, t2) (Step: anything with int members x, y); a saveat value lies inside the
// step that contains it, by the solvers' linear interpolant; saveat = [] saves every step; save_start < 0: DiffEq's default
// rule.  The times are float32 products in this order, the end of the grid is t2 itself.
struct SdeSeriesEntry { float t; int k; float theta; };  // value = (1-theta) * state_before(step k) + theta * rec_u[k]; k = -1: the start value
enum { SERIES_OK = 0, SERIES_T1_OUTSIDE, SERIES_SAVES_NOTHING, SERIES_BIASED_NEEDS_TWO, SERIES_T1_AT_END };   // refusals, in the order they are found
struct SdeSeriesPlan {
  int status = SERIES_OK;
  std::vector<SdeSeriesEntry> sol;      // what the solve saves
  SdeSeriesEntry e1{}; float t1 = 0.f;  // where the local step starts (t1 = t2 for :none, which has none)
  std::vector<SdeSeriesEntry> series;   // the caller's view: sol after the _CorrectedDESolution filter
};
template <class Step>
inline SdeSeriesPlan sde_series_plan(float t0, float t2, int nfine, const Step* im, int K, int mode, float t1_or_rand, int save_start,
                                     const float* user, int nuser) {
  SdeSeriesPlan p;
  const float h = (t2 - t0) / (float)nfine;
  auto tk = [&](int k) { return t0 + (float)im[k].x * h; };                       // start of accepted step k
  auto tk1 = [&](int k) { return (im[k].x + im[k].y >= nfine) ? t2 : t0 + (float)(im[k].x + im[k].y) * h; };
  auto entry_at = [&](float ts) {
    SdeSeriesEntry e; e.t = ts; e.k = -1; e.theta = 0.f;
    if (!(ts > t0)) return e;
    int k = 0;
    while (k < K - 1 && tk1(k) < ts) ++k;
    e.k = k;
    e.theta = (ts >= tk1(k)) ? 1.0f : (ts - tk(k)) / ((float)im[k].y * h);
    return e;
  };
  p.t1 = t2;
  if (mode == LRNDE_MODE_UNBIASED) {
    p.t1 = t1_or_rand;
    if (!(p.t1 >= t0 && p.t1 <= t2)) { p.status = SERIES_T1_OUTSIDE; return p; }
  }
  const SolveSaveat plan = solve_saveat(mode, p.t1, t2, user, nuser);
  const std::vector<float>& sv = plan.saveat;   // the solve's saveat
  const bool everystep = plan.save_everystep != 0;
  bool with_start = save_start > 0;
  if (save_start < 0) with_start = everystep || (!sv.empty() && sv.front() == t0);   // DiffEq: save_everystep || isempty(saveat) || tspan[1] in saveat
  if (with_start) { SdeSeriesEntry e; e.t = t0; e.k = -1; e.theta = 0.f; p.sol.push_back(e); }
  if (everystep) {
    for (int k = 0; k < K; ++k) { SdeSeriesEntry e; e.t = tk1(k); e.k = k; e.theta = 1.0f; p.sol.push_back(e); }
  } else {
    for (float ts : sv) { if (ts == t0 && with_start) continue; p.sol.push_back(entry_at(ts)); }
  }
  if (p.sol.empty()) { p.status = SERIES_SAVES_NOTHING; return p; }
  p.e1.t = t2; p.e1.k = K - 1; p.e1.theta = 1.0f;
  if (mode == LRNDE_MODE_BIASED) {      // :114-115  t1 = rand(rng, sol.t[1:(end - 1)])
    const int m = (int)p.sol.size() - 1;
    if (m < 1) { p.status = SERIES_BIASED_NEEDS_TWO; return p; }
    p.e1 = p.sol[biased_pick(t1_or_rand, m)]; p.t1 = p.e1.t;
  } else if (mode == LRNDE_MODE_UNBIASED) {
    p.e1 = entry_at(p.t1);
  }
  if (mode != LRNDE_MODE_NONE && !(p.t1 < t2)) { p.status = SERIES_T1_AT_END; return p; }
  // the caller's view: _CorrectedDESolution drops the entries at t1 (src/utils.jl:31-33: `sol.u[t1 .!= sol.t]`)
  for (const SdeSeriesEntry& e : p.sol) if (series_keeps(plan.needs_correction, p.t1, e.t)) p.series.push_back(e);
  return p;
}

// ---- save-slot predictions of the ODE solves (lrnde_solve, lrnde_conv_solve) ----
// The slot of the LAST saveat entry equal to t1: its index among the entries inside the span (those at or before t0 are
// the start value and take no slot), behind the save_start slot if there is one.  -1: not known before the solve (t1 is
// not an entry, or lies at or before t0).
inline int slot_of_t1(const float* sv, int nsv, float t0, float t1, int save_start) {
  const int kpos = (int)(std::upper_bound(sv, sv + nsv, t1) - sv) - 1;
  int nskip = 0;
  while (nskip < nsv && sv[nskip] <= t0) ++nskip;
  if (kpos < nskip || !(sv[kpos] == t1)) return -1;
  return kpos - nskip + (save_start ? 1 : 0);
}
// sol.u[end] is the last save slot; when there is no start slot and every saveat time lies in (t0, t2] that slot is
// known before the solve (which then copies it to the caller's array itself).  -1: not known.
inline int end_slot_known(const float* sv, int nsv, float t0, float t2, int save_start) {
  if (save_start || nsv < 1) return -1;
  for (int i = 0; i < nsv; ++i) if (!(sv[i] > t0 && sv[i] <= t2)) return -1;
  return nsv - 1;
}
// save slots the layer forward asks for: [t1, t2] and a start value; the user's entries, t1 and a start value; or every
// accepted step of a :biased solve without a user saveat (at most 512 slots)
inline size_t slots_needed(int mode, int nuser, int maxiters) {
  if (nuser > 0) return (size_t)nuser + 3;
  if (mode == LRNDE_MODE_BIASED) return (size_t)(maxiters < 510 ? maxiters + 2 : 512);
  return 3;
}

// ---- tstops of the backward pass: the saved times strictly inside (t0, t2), in reversed time s = -t, ascending ----
inline std::vector<float> backward_stops(const std::vector<float>& ts, float t0, float t2) {
  std::vector<float> stops;
  for (int i = (int)ts.size() - 1; i >= 0; --i)
    if (ts[i] > t0 && ts[i] < t2) stops.push_back(-ts[i]);
  return stops;
}

// ---- what a recorded layer forward leaves for lrnde_*_node_backward_recorded, the part every ODE handle keeps ----
// (the handles add their own: NodeRecord in lrnde_kernels.hip; u(t1) and the dense vectors of the conv handle)
struct LayerRecord {
  bool valid = false;
  unsigned long long gen = 0;   // counts the recorded forwards of the handle
  int B = 0, mode = 0, reg_type = 0;
  float t0 = 0.f, t2 = 0.f, t1 = 0.f;
  int solver_alg = 0;           // LRNDE_ALG_* of the solve that made the record: what form its dense slots have
  lrnde_solve_opts opts{};
  std::vector<float> ts;        // sol.t of the solve: the cotangent times of the adjoint
  void invalidate() { valid = false; }
  unsigned long long generation() const { return valid ? gen : 0; }   // 0: no usable record
  void set(int B_, int mode_, int reg_type_, float t0_, float t2_, float t1_, const lrnde_solve_opts& o, int solver_alg_ = 0) {
    valid = true; ++gen; B = B_; mode = mode_; reg_type = reg_type_; t0 = t0_; t2 = t2_; t1 = t1_; opts = o; solver_alg = solver_alg_;
  }
};

}  // namespace lrnde
