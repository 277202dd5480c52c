// lrnde_report.hpp — what the device-controlled solve loops report to pinned host memory, and how a host driver waits for
// it, stated once: the three report layouts (encoder and decoder side by side), the one bounded wait, the forward
// loop's feed rule, the adjoint drivers' trace cursor, and the status -> retcode / lrnde_stats mapping (DESIGN.md §4.7.2
// lists who writes and who reads each report and what each driver does on each outcome of the wait).
//
// Like lrnde_stepctl.hpp: values in, values out, no HIP call, no lrnde_ctx; compiles on its own with g++, and
// tests/test_host_report.py runs every branch of it on the host — the late, drained, error and hung branches of the
// wait cannot be run on a GPU at all.
#pragma once
#include <chrono>

#include "lrnde.h"
#include "lrnde_math.hpp"

namespace lrnde {

enum { ST_RUNNING = 0, ST_DONE = 100 };   // a control block's status: else an lrnde_status error

// ---- the forward solve's ring word: [rem : 16][nsaved : 16][status : 8][launches : 24], rem in the top bits ----
// One word per launch, in slot (launch index mod PROG_RING); launches = launch index + 1, so a word validates itself.
constexpr int PROG_RING = 32;  // > the deepest queue the host keeps (16 launches ahead of the last report it has read)
struct SolveReport { int launches, status, nsaved, rem; };   // rem: steps still to go at the current dt
// The report of launch j as the step prologue packs it (solve_progress keeps its own flat expression of the same word:
// the step kernels' text changes with any regrouping of it; tests/test_host_report.py holds this statement to the layout).
// The launch count j + 1 wraps at 24 bits, the status keeps its low 8, nsaved stops at 65535, and steps_left becomes rem
// by ceil, then the 16-bit cap, then the floor at zero (NaN and negatives give 0).
LRNDE_HD int solve_report_rem(float steps_left) {
  const float sl = __builtin_ceilf(steps_left);
  return sl > 65535.f ? 65535 : (sl > 0.f ? (int)sl : 0);
}
LRNDE_HD SolveReport solve_report(int j, int status, int nsaved_done, float steps_left) {
  return {(j + 1) & 0xffffff, status & 0xff, nsaved_done > 65535 ? 65535 : nsaved_done, solve_report_rem(steps_left)};
}
LRNDE_HD constexpr unsigned long long solve_report_pack(const SolveReport r) {
  return (unsigned long long)(r.launches & 0xffffff) | ((unsigned long long)(r.status & 0xff) << 24) |
         ((unsigned long long)(r.nsaved & 0xffff) << 32) | ((unsigned long long)(r.rem & 0xffff) << 48);
}
LRNDE_HD constexpr SolveReport solve_report_unpack(unsigned long long w) {
  return {(int)(w & 0xffffffull), (int)((w >> 24) & 0xff), (int)((w >> 32) & 0xffff), (int)((w >> 48) & 0xffff)};
}

// ---- the adaptive SDE solve's word: (launches whose footer ran) | status << 32 ----
struct SdeReport { unsigned count, status; };
LRNDE_HD constexpr unsigned long long sde_report_pack(unsigned count, unsigned status) {
  return (unsigned long long)count | ((unsigned long long)status << 32);
}
LRNDE_HD constexpr SdeReport sde_report_unpack(unsigned long long w) { return {(unsigned)(w & 0xffffffffull), (unsigned)(w >> 32)}; }

// ---- the adjoint loops' progress block: ADJ_R_LEN ints, floats as their bits ----
// Written by the first launch of every attempt (adj_hstat_fill), seq last (release): everything the driver needs of the
// integrator's state, so that a finished solve costs no read-back copy.  seq of attempt j is seq0 + j + 1.
// ADJ_R_OVL_TIMEOUT: a wait between overlapped stage launches timed out (the results are not to be used).
enum { ADJ_R_SEQ = 0, ADJ_R_STATUS, ADJ_R_T, ADJ_R_DT, ADJ_R_CUR, ADJ_R_NF, ADJ_R_NACCEPT, ADJ_R_NREJECT, ADJ_R_ITER, ADJ_R_EEST_LAST,
       ADJ_R_DT_INIT, ADJ_R_OVL_TIMEOUT, ADJ_R_LEN = 16 };
struct AdjReport { int status; float t, dt; int cur, nf, naccept, nreject, iter; float eest_last, dt_init; int ovl_timeout; };
inline AdjReport adj_report_read(const volatile int* hs) {
  const auto f = [hs](int i) { return __builtin_bit_cast(float, (int)hs[i]); };
  return {hs[ADJ_R_STATUS], f(ADJ_R_T), f(ADJ_R_DT), hs[ADJ_R_CUR], hs[ADJ_R_NF], hs[ADJ_R_NACCEPT], hs[ADJ_R_NREJECT], hs[ADJ_R_ITER],
          f(ADJ_R_EEST_LAST), f(ADJ_R_DT_INIT), hs[ADJ_R_OVL_TIMEOUT]};
}

// ---- layout checks: every pack / unpack pair at the field limits ----
static_assert(solve_report_pack({1, 0, 0, 0}) == 1ull && solve_report_pack({0, 1, 0, 0}) == 1ull << 24 &&
              solve_report_pack({0, 0, 1, 0}) == 1ull << 32 && solve_report_pack({0, 0, 0, 1}) == 1ull << 48, "ring word: field offsets");
static_assert(solve_report_pack(solve_report_unpack(~0ull)) == ~0ull && solve_report_pack(solve_report_unpack(0x0123456789abcdefull)) == 0x0123456789abcdefull &&
              solve_report_pack({0xffffff, 0xff, 0xffff, 0xffff}) == ~0ull && solve_report_unpack(~0ull).launches == 0xffffff && solve_report_unpack(~0ull).rem == 0xffff &&
              solve_report_pack({0x1000000, 0x100 + ST_DONE, 0, 0}) == (unsigned long long)ST_DONE << 24, "ring word: round trip at the field limits, wrap of the launch count");
static_assert(ST_DONE == (ST_DONE & 0xff), "every status fits the ring word's 8 bits");
static_assert((PROG_RING & (PROG_RING - 1)) == 0 && PROG_RING > 16, "slot = launch index & (PROG_RING - 1); deeper than the feed rule's cap");
static_assert(sde_report_pack(0xffffffffu, 0) == 0xffffffffull && sde_report_pack(0, 0xffffffffu) == 0xffffffff00000000ull &&
              sde_report_unpack(sde_report_pack(7u, (unsigned)ST_DONE)).count == 7u && sde_report_unpack(sde_report_pack(7u, (unsigned)ST_DONE)).status == (unsigned)ST_DONE &&
              sde_report_unpack(~0ull).count == 0xffffffffu && sde_report_unpack(~0ull).status == 0xffffffffu, "SDE word: 32 + 32 bits");
static_assert(ADJ_R_DT_INIT == 10 && ADJ_R_OVL_TIMEOUT == 11 && ADJ_R_OVL_TIMEOUT < ADJ_R_LEN, "adjoint block: eleven words and the timeout word");

// ---- the one wait for a report ----
// Spin on ready(); every `every` failed checks (and, with stall_us, only once that long has passed since the wait began
// or since the last query) ask the queue: a query is a marker packet in the queue, so it is kept for a report that is
// LATE.  Two cadences: a forward step launch is one of a queue a launch or two deep, where a marker is a 6-us bubble
// between two steps, so its loops ask only after 20 ms without a report; an adjoint attempt is >= 130 us of launches
// behind its report and 2^20 spins last far longer than that, so the adjoint loops ask then, without a clock.
struct WaitCadence { long every; long long stall_us; };   // every: a power of two
constexpr WaitCadence WAIT_PER_ATTEMPT{0x100000, 0};      // the adjoint loops
constexpr WaitCadence WAIT_PER_LAUNCH{0x4000, 20000};     // the forward solve and the SDE loop
constexpr int LRNDE_SPIN_DEADLINE_S = 90;  // (above the local communicator's 60-s rendezvous timeout)
enum { QUERY_DRAINED = 0, QUERY_NOT_READY = -1 };   // query(): one of these, or an error code of the caller's (any other value)
// ready: the report is there.  drained: everything enqueued has run and one more look finds no report.  queue error: the
// queue's answer is in ReportWait::code.  hung: "not ready" for LRNDE_SPIN_DEADLINE_S since the wait began.
enum WaitResult { WAIT_READY, WAIT_DRAINED, WAIT_QUEUE_ERROR, WAIT_HUNG };
struct SteadyUs { long long operator()() const { using namespace std::chrono; return duration_cast<microseconds>(steady_clock::now().time_since_epoch()).count(); } };
// clock(): microseconds, monotonic.  One object per wait, awaited once: its clocks start when it is made.
template <class Clock = SteadyUs> struct ReportWait {
  WaitCadence cad; Clock clock; long long t0, t_last; int code = 0;
  explicit ReportWait(WaitCadence cadence, Clock clk = Clock()) : cad(cadence), clock(clk), t0(clock()), t_last(t0) {}
  template <class Ready, class Query> WaitResult await(Ready&& ready, Query&& query) {
    for (long spins = 1; !ready(); ++spins) {
      if ((spins & (cad.every - 1)) != 0 || (cad.stall_us && clock() - t_last < cad.stall_us)) continue;
      t_last = clock();
      const int q = query();
      if (q == QUERY_DRAINED) return ready() ? WAIT_READY : WAIT_DRAINED;
      if (q != QUERY_NOT_READY) { code = q; return WAIT_QUEUE_ERROR; }
      if (clock() - t0 > 1000000ll * LRNDE_SPIN_DEADLINE_S) return WAIT_HUNG;
    }
    return WAIT_READY;
  }
};

// ---- the forward loop's feed rule ----
// After the report of launch seen - 1 said `rem` steps to go: keep launches up to seen + ahead enqueued; those from
// `certain` on carry the speculative kernel name.  fT, fE, fM: the LRNDE_FEED_T / _E / _M options (3, 1, 2): near the
// end (rem <= fT) the estimate is exact — rem launches and the fE that find the solve finished; far from it dt still
// grows and half the estimate is enough; never fewer than fM ahead, never more than 16.
struct Feed { int ahead, certain; };
LRNDE_HD constexpr Feed feed_rule(int rem, int seen, int fT, int fE, int fM) {
  int ahead = rem <= fT ? rem + fE : rem / 2 + fE + 1;
  if (ahead < fM) ahead = fM;
  if (ahead > 16) ahead = 16;
  return {ahead, seen + (rem > 1 ? rem / 2 : 1)};
}

// ---- status -> retcode, report -> lrnde_stats ----
LRNDE_HD constexpr int status_retcode(int status) { return status == ST_DONE ? LRNDE_OK : (status == ST_RUNNING ? LRNDE_MAXITERS : status); }
// extra_nf: evaluations the driver enqueued outside the attempts (the re-evaluation after each cotangent impulse)
inline void adj_stats_fill(const AdjReport& r, int extra_nf, lrnde_stats* st) {
  st->retcode = status_retcode(r.status); st->nf = r.nf + extra_nf; st->naccept = r.naccept; st->nreject = r.nreject; st->iters = r.iter;
  st->t_final = r.t; st->dt_final = r.dt; st->eest_last = r.eest_last; st->dt_init = r.dt_init;
}

// ---- the adjoint drivers' trace: one row per attempt, from the reports alone ----
// The report of attempt j (1-based within a segment) carries that attempt's (s, dt) and the error estimate / decision
// of the attempt BEFORE it: the previous row is completed, then a row is opened — only for an attempt that runs and
// while the array has room.
struct AdjTraceCursor { int prev = -1, nacc = 0; };
inline void adj_trace_report(AdjTraceCursor& k, int j, const AdjReport& r, lrnde_trace_row* rows, int& n, int cap) {
  if (j > 1 && k.prev >= 0) { rows[k.prev].eest = r.eest_last; rows[k.prev].accepted = (r.naccept > k.nacc); }
  k.prev = -1; k.nacc = r.naccept;
  if (r.status == ST_RUNNING && n < cap) rows[k.prev = n++] = {r.t, r.dt, 0.f, -1};
}

// ---- may the reported attempt be the segment's last? ----
// Its end within 100 eps of the segment's: the next attempt is then enqueued as its first launch only.  <=, where the
// accept snap (snap_magnitude) has <: an attempt exactly on the bound is treated as possibly last, which costs a host
// round trip and never a wrong result.
LRNDE_HD bool adj_maybe_last(float t, float dt, float s1) {
  return __builtin_fabsf(t + dt - s1) <= 100.0f * eps_f(fmaxf_(__builtin_fabsf(t + dt), __builtin_fabsf(s1)));
}

}  // namespace lrnde
