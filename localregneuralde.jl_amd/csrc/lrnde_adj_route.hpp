// lrnde_adj_route.hpp — which of its six ways lrnde_node_backward_recorded(_ts) runs the reversed solve, and the launch
// plan of that way, stated once: the route as an enum, the four gates (LDS, workgroups, scratch) of the
// routes that have one, and the order in which a handle's settings choose between them.
//
// Like lrnde_layer_plan.hpp and lrnde_stepctl.hpp: values in, values out, no HIP call, no handle and no device header, so
// the host compiler builds it alone (tests/test_host_adj_route.py).  lrnde_kernels.hip fills AdjRouteIn from a handle and
// a batch (adj_route_in) and switches on the answer (node_backward_recorded_impl).
//
// The routes, by the number lrnde_last_adjoint_info reports (Handle.ADJOINT_LOOP_NAMES has the same order):
//   0 ADJ_ROUTE_HOST            the host-controlled loop (vec_tsit5_solve): every handle, every batch
//   1 ADJ_ROUTE_MLP_DEVICE      the MLP handle's device-controlled loop (adj_solve_device, lrnde_adjoint.hpp)
//   2 ADJ_ROUTE_CHAIN_DEVICE    the small Dense-chain handle's device-controlled loop (lrnde_chain_adjoint.hpp)
//   3 ADJ_ROUTE_WIDE_DEVICE     the wide Dense-chain handle's device-controlled loop (lrnde_wide_adjoint.hpp), opt-in
//   4 ADJ_ROUTE_CHAIN_DISCRETE  the small chain's discrete adjoint, one launch over the step record (lrnde_chain_discrete.hpp)
//   5 ADJ_ROUTE_WIDE_DISCRETE   the wide chain's discrete adjoint, two launches per recorded step (lrnde_wide_discrete.hpp)
//
// Precedence (adj_route; the first point that applies decides):
//   1. wide handle, adj_loop == DEVICE, not sharded, LRNDE_ADJ_HOST off: the wide device gate must pass, otherwise the
//      call is refused with "wide adjoint loop: <why>".  Route 3.
//   2. wide handle, adj_loop == DISCRETE (LRNDE_ADJ_HOST does not override it): the wide discrete gate must pass, otherwise
//      "wide discrete adjoint: <why>".  Route 5.
//   3. sensealg == DISCRETE: the small discrete gate must pass, otherwise "discrete adjoint: <why>" (among the reasons: not
//      a small Dense-chain handle, the handle is sharded).  Route 4.
//   4. small chain, not sharded, LRNDE_ADJ_HOST off, and the small device gate passes.  Route 2.  A gate that does not pass
//      is no refusal: the solve falls through.
//   5. the 4-column VJP runs this batch, not sharded, LRNDE_ADJ_HOST off.  Route 1.
//   6. route 0.
// adj_loop == DISCRETE on a handle that is not wide is ignored (lrnde_set_adjoint_loop refuses it anyway); a wide handle with
// DEVICE while sharded or with LRNDE_ADJ_HOST on falls to route 0.  A discrete route never falls back to a continuous one.
#pragma once
#include <algorithm>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <string>
#include <vector>

#include "lrnde.h"

namespace lrnde {

enum AdjRoute { ADJ_ROUTE_HOST = 0, ADJ_ROUTE_MLP_DEVICE = 1, ADJ_ROUTE_CHAIN_DEVICE = 2, ADJ_ROUTE_WIDE_DEVICE = 3, ADJ_ROUTE_CHAIN_DISCRETE = 4, ADJ_ROUTE_WIDE_DISCRETE = 5 };

// ---- the gates' limits ----
constexpr int CHADJ_MAX_WG = 4096;           // workgroups whose norm partials one wave sums per attempt
constexpr int CHADJ_MAX_MU_BLOCKS = 256;     // grid of the mu-family launches
constexpr size_t CHADJ_LDS_MAX = 160 * 1024;
constexpr size_t CHADJ_SCRATCH_MAX = (size_t)256 << 20;   // bytes of the small chain's parameter partials (gpart)
constexpr size_t WIDE_LDS_MAX = 160 * 1024;
// scratch of one launch of a wide handle (stage / activation records, partial vectors, sweep vectors)
constexpr size_t WIDE_SCRATCH_MAX = (size_t)256 << 20;

// ---- dynamic LDS of the kernels behind the gates; tail: the fixed part behind the images and buffers, which the device
// headers own (reduction scratch, broadcast and control blocks, padding) ----
// small chain: forward image, backward image and parameter partial (each rounded to 4 floats; 0: not in LDS), the VJP's record
inline size_t chain_lds_bytes(int wfloats, int gfloats_lds, size_t pfloats_lds, size_t vjp_lds, size_t tail) {
  return ((size_t)wfloats + (size_t)((gfloats_lds + 3) & ~3) + ((pfloats_lds + 3) & ~(size_t)3)) * sizeof(float) + vjp_lds + tail;
}
// wide chain: two activation buffers and the segment-partial region
inline size_t wide_lds_bytes(int bufw, int partcap, size_t tail) { return (2 * (size_t)bufw + (size_t)partcap) * sizeof(float) + tail; }

// what the device headers own of the gates' arithmetic, as numbers (lrnde_kernels.hip adj_route_in fills them)
struct AdjDevSizes {
  int chain_tile = 0, wide_tile = 0;        // batch columns per workgroup (CNB, NB)
  int mu_block = 0;                         // WADJ_MB: a mu work item is mu_block x mu_block output blocks of 16 x 16
  int wadj_slots = 0, wdisc_slots = 0;      // stage-record slots of the wide device loop / the wide discrete sweep
  int wdisc_vecs = 0;                       // B*D vectors the wide discrete sweep keeps beside z
  size_t ctrl_bytes = 0;                    // sizeof(ChAdjCtrl)
  size_t chadj_tail = 0, chdisc_tail = 0;   // LDS tails of k_chadj_step / k_chain_dsweep (chain_lds_bytes)
  size_t wide_tail = 0, wadj_tail = 0;      // LDS tails of the wide forward carve / k_wadj_step (wide_lds_bytes)
};

struct AdjRouteIn {
  int field = 0;                            // 0 MLP, 1 small Dense chain, 2 wide Dense chain
  int adj_loop = LRNDE_ADJ_LOOP_AUTO;       // lrnde_set_adjoint_loop
  int sensealg = LRNDE_SENSE_INTERPOLATING; // lrnde_set_sensealg
  bool sharded = false;
  bool adj_host = false;                    // LRNDE_ADJ_HOST: the host-controlled loop, as a diagnostic
  bool qvjp = false;                        // the 4-column VJP runs this batch (an MLP handle only)
  int B = 0, D = 0;
  size_t P = 0;
  // small chain
  int wfloats = 0, gfloats = 0;             // forward / backward weight image
  size_t vjp_lds = 0;                       // the VJP's activation record (bytes)
  // wide chain
  int bufw = 0, partcap = 0, recfloats = 0; // one activation buffer, the forward kernels' partial region, one tile's record
  std::vector<int> dims;                    // layer widths, nlayers + 1 of them
  AdjDevSizes dev;
};

// fields a route does not use are zero
struct AdjPlan {
  AdjRoute route = ADJ_ROUTE_HOST;
  int nwg = 0, nmu = 0;                     // grids of the step-family and mu-family launches
  int nitems = 0;                           // the wide handle's mu work items
  int wg_lds = 0, p_lds = 0;                // small chain: the backward image / the parameter partial live in LDS
  int partcap = 0;                          // wide device loop: the partial region left beside the control block
  size_t lds = 0;                           // dynamic LDS of the step-family launch
  size_t rec_floats = 0, vec_floats = 0;    // wide chain: stage records, sweep vectors
};

// ---- shared pieces of the gates ----
// a gate's "no": false, and the limit missed to why (may be null)
__attribute__((format(printf, 2, 3))) inline bool adj_no(std::string* why, const char* fmt, ...) {
  char msg[240];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(msg, sizeof msg, fmt, ap);
  va_end(ap);
  if (why) *why = msg;
  return false;
}
inline bool adj_wg_cap(int B, int nwg, std::string* why) {
  return nwg <= CHADJ_MAX_WG || adj_no(why, "B = %d is %d workgroups, CHADJ_MAX_WG is %d", B, nwg, CHADJ_MAX_WG);
}
// work items of the wide handle's mu launches: per layer the groups of mu_block x mu_block blocks of vec(W), then the
// 64-output chunks of the t column and the bias
inline int wide_mu_items(const std::vector<int>& dims, int mu_block) {
  int n = 0;
  for (size_t l = 0; l + 1 < dims.size(); ++l) {
    const int MT = (dims[l + 1] + 15) / 16, KG = (dims[l] + 15) / 16;
    n += ((MT + mu_block - 1) / mu_block) * ((KG + mu_block - 1) / mu_block) + (dims[l + 1] + 63) / 64;
  }
  return n;
}

// ---- the gates: true and the plan (its route left to adj_route), or false, the plan untouched and why (may be null) ----
// Small chain, device loop: the step kernel's LDS (forward image + activation record + reduction scratch; the backward image
// rides along when it fits too) within CHADJ_LDS_MAX, at most CHADJ_MAX_WG workgroups, and the per-(stage, workgroup)
// parameter cotangents (7 x workgroups x P floats) within CHADJ_SCRATCH_MAX.
inline bool chain_device_gate(const AdjRouteIn& in, AdjPlan* pl, std::string* why = nullptr) {
  if (in.field != 1) return adj_no(why, "not a small Dense-chain handle");
  const int nwg = (in.B + in.dev.chain_tile - 1) / in.dev.chain_tile;
  const size_t lds0 = chain_lds_bytes(in.wfloats, 0, 0, in.vjp_lds, in.dev.chadj_tail);
  const size_t lds1 = chain_lds_bytes(in.wfloats, in.gfloats, 0, in.vjp_lds, in.dev.chadj_tail);
  const size_t bytes = 7 * (size_t)nwg * in.P * sizeof(float);
  if (lds0 > CHADJ_LDS_MAX) return adj_no(why, "the step kernel needs %zu bytes of LDS, CHADJ_LDS_MAX is %zu", lds0, CHADJ_LDS_MAX);
  if (!adj_wg_cap(in.B, nwg, why)) return false;
  if (bytes > CHADJ_SCRATCH_MAX) return adj_no(why, "B = %d needs %zu bytes of parameter cotangents, CHADJ_SCRATCH_MAX is %zu", in.B, bytes, CHADJ_SCRATCH_MAX);
  pl->nwg = nwg;
  pl->nmu = (int)std::min<size_t>((in.P + 63) / 64, CHADJ_MAX_MU_BLOCKS);
  pl->wg_lds = lds1 <= CHADJ_LDS_MAX ? 1 : 0;
  pl->lds = pl->wg_lds ? lds1 : lds0;
  return true;
}

// Small chain, discrete sweep: a small-chain handle, not sharded; the sweep's LDS (forward image + activation record; the
// backward image and then the workgroup's parameter partial ride along when they fit too) within CHADJ_LDS_MAX, at most
// CHADJ_MAX_WG workgroups, and the per-workgroup parameter partials (workgroups x P floats) within CHADJ_SCRATCH_MAX.
inline bool chain_discrete_gate(const AdjRouteIn& in, AdjPlan* pl, std::string* why) {
  if (in.field != 1) return adj_no(why, "not a small Dense-chain handle");
  if (in.sharded) return adj_no(why, "the handle is sharded");
  const int nwg = (in.B + in.dev.chain_tile - 1) / in.dev.chain_tile;
  const size_t lds0 = chain_lds_bytes(in.wfloats, 0, 0, in.vjp_lds, in.dev.chdisc_tail);
  const size_t lds1 = chain_lds_bytes(in.wfloats, in.gfloats, 0, in.vjp_lds, in.dev.chdisc_tail);
  const size_t lds2 = chain_lds_bytes(in.wfloats, in.gfloats, in.P, in.vjp_lds, in.dev.chdisc_tail);
  const size_t bytes = (size_t)nwg * in.P * sizeof(float);
  if (lds0 > CHADJ_LDS_MAX) return adj_no(why, "the sweep needs %zu bytes of LDS, CHADJ_LDS_MAX is %zu", lds0, CHADJ_LDS_MAX);
  if (!adj_wg_cap(in.B, nwg, why)) return false;
  if (bytes > CHADJ_SCRATCH_MAX) return adj_no(why, "B = %d needs %zu bytes of parameter partials, CHADJ_SCRATCH_MAX is %zu", in.B, bytes, CHADJ_SCRATCH_MAX);
  pl->nwg = nwg;
  pl->wg_lds = lds1 <= CHADJ_LDS_MAX ? 1 : 0;
  pl->p_lds = lds2 <= CHADJ_LDS_MAX ? 1 : 0;
  pl->lds = pl->p_lds ? lds2 : (pl->wg_lds ? lds1 : lds0);
  return true;
}

// Wide chain, device loop: the step kernel's LDS (the forward kernels' carve, its segment-partial region cut back by what
// the control block takes) within WIDE_LDS_MAX; at most CHADJ_MAX_WG workgroups; the stage-record slots for the batch plus
// the two control blocks and the five sets of norm partials within WIDE_SCRATCH_MAX.
inline bool wide_device_gate(const AdjRouteIn& in, AdjPlan* pl, std::string* why) {
  if (in.field != 2) return adj_no(why, "not a wide-chain handle");
  const int nwg = (in.B + in.dev.wide_tile - 1) / in.dev.wide_tile;
  const size_t fixed = wide_lds_bytes(in.bufw, 0, in.dev.wadj_tail);
  const int partcap = fixed > WIDE_LDS_MAX ? 0 : (int)std::min<size_t>((size_t)in.partcap, ((WIDE_LDS_MAX - fixed) / sizeof(float)) & ~(size_t)255);
  const size_t lds = wide_lds_bytes(in.bufw, partcap, in.dev.wadj_tail);
  if (lds > WIDE_LDS_MAX) return adj_no(why, "the step kernel needs %zu bytes of LDS, WIDE_LDS_MAX is %zu", lds, WIDE_LDS_MAX);
  if (!adj_wg_cap(in.B, nwg, why)) return false;
  const int nitems = wide_mu_items(in.dims, in.dev.mu_block);
  const int nmu = std::min(nitems, CHADJ_MAX_MU_BLOCKS);
  const size_t rec_floats = (size_t)in.dev.wadj_slots * nwg * in.recfloats;
  const size_t bytes = rec_floats * sizeof(float) + 2 * in.dev.ctrl_bytes + 5 * (size_t)(nwg + nmu) * sizeof(double);
  if (bytes > WIDE_SCRATCH_MAX)
    return adj_no(why, "B = %d needs %zu bytes of stage records (%d slots), WIDE_SCRATCH_MAX is %zu", in.B, bytes, in.dev.wadj_slots, WIDE_SCRATCH_MAX);
  pl->nwg = nwg; pl->nitems = nitems; pl->nmu = nmu; pl->partcap = partcap; pl->lds = lds; pl->rec_floats = rec_floats;
  return true;
}

// Wide chain, discrete sweep: a wide-chain handle, not sharded; the step kernel's LDS (the forward kernels' carve) within
// WIDE_LDS_MAX; at most CHADJ_MAX_WG tiles; the stage-record slots plus the sweep's B*D vectors within WIDE_SCRATCH_MAX.
inline bool wide_discrete_gate(const AdjRouteIn& in, AdjPlan* pl, std::string* why) {
  if (in.field != 2) return adj_no(why, "not a wide-chain handle");
  if (in.sharded) return adj_no(why, "the handle is sharded");
  const int nwg = (in.B + in.dev.wide_tile - 1) / in.dev.wide_tile;
  const size_t lds = wide_lds_bytes(in.bufw, in.partcap, in.dev.wide_tail);
  if (lds > WIDE_LDS_MAX) return adj_no(why, "the step kernel needs %zu bytes of LDS, WIDE_LDS_MAX is %zu", lds, WIDE_LDS_MAX);
  if (!adj_wg_cap(in.B, nwg, why)) return false;
  const int nitems = wide_mu_items(in.dims, in.dev.mu_block);
  const size_t rec_floats = (size_t)in.dev.wdisc_slots * nwg * in.recfloats;
  const size_t vec_floats = (size_t)in.dev.wdisc_vecs * in.B * in.D;
  const size_t bytes = (rec_floats + vec_floats) * sizeof(float);
  if (bytes > WIDE_SCRATCH_MAX)
    return adj_no(why, "B = %d needs %zu bytes of stage records (%d slots) and sweep vectors (%d), WIDE_SCRATCH_MAX is %zu", in.B, bytes,
                  in.dev.wdisc_slots, in.dev.wdisc_vecs, WIDE_SCRATCH_MAX);
  pl->nwg = nwg; pl->nitems = nitems; pl->nmu = std::min(nitems, CHADJ_MAX_MU_BLOCKS); pl->lds = lds;
  pl->rec_floats = rec_floats; pl->vec_floats = vec_floats;
  return true;
}

// ---- the decision: LRNDE_OK and the plan, or LRNDE_UNSUPPORTED and the refusal's text (the precedence in the head comment) ----
inline int adj_route(const AdjRouteIn& in, AdjPlan* pl, std::string* refusal) {
  *pl = AdjPlan{};
  std::string why;
  auto took = [&](AdjRoute r) { pl->route = r; return (int)LRNDE_OK; };
  auto refuse = [&](const char* what) { *refusal = std::string(what) + ": " + why; return (int)LRNDE_UNSUPPORTED; };
  const bool wide = in.field == 2;
  const bool device_ok = !in.sharded && !in.adj_host;
  if (wide && in.adj_loop == LRNDE_ADJ_LOOP_DEVICE && device_ok)
    return wide_device_gate(in, pl, &why) ? took(ADJ_ROUTE_WIDE_DEVICE) : refuse("wide adjoint loop");
  if (wide && in.adj_loop == LRNDE_ADJ_LOOP_DISCRETE)
    return wide_discrete_gate(in, pl, &why) ? took(ADJ_ROUTE_WIDE_DISCRETE) : refuse("wide discrete adjoint");
  if (in.sensealg == LRNDE_SENSE_DISCRETE)
    return chain_discrete_gate(in, pl, &why) ? took(ADJ_ROUTE_CHAIN_DISCRETE) : refuse("discrete adjoint");
  if (in.field == 1 && device_ok && chain_device_gate(in, pl)) return took(ADJ_ROUTE_CHAIN_DEVICE);
  if (in.qvjp && device_ok) return took(ADJ_ROUTE_MLP_DEVICE);
  return took(ADJ_ROUTE_HOST);
}

// ---- what follows from the route ----
// The caller zeroes z = [lambda; mu] before the solve.  Not for the MLP loop with a single end cotangent (its first launch
// sets z = [du_end; 0] itself) and not for the small chain's sweep (it writes all of z; the wide chain's adds to a zeroed mu).
inline bool adj_caller_zeroes_z(AdjRoute r, bool single_end_cotangent) {
  return !(r == ADJ_ROUTE_MLP_DEVICE && single_end_cotangent) && r != ADJ_ROUTE_CHAIN_DISCRETE;
}
// Impulses and tstops are built: the continuous routes (a discrete sweep takes the cotangents from the caller's array)
inline bool adj_builds_impulses(AdjRoute r) { return r != ADJ_ROUTE_CHAIN_DISCRETE && r != ADJ_ROUTE_WIDE_DISCRETE; }
// A regulariser sweep the forward left pending is enqueued behind the loop's first attempt: the MLP device loop only.  (The
// condition was "the 4-column VJP runs this batch, not sharded, LRNDE_ADJ_HOST off", which is route 1 exactly: that VJP runs
// for no chain handle, so points 1..4 of the precedence cannot apply where it holds.)  Every other route runs it before the solve.
inline bool adj_sweep_rides_first_attempt(AdjRoute r) { return r == ADJ_ROUTE_MLP_DEVICE; }

}  // namespace lrnde
