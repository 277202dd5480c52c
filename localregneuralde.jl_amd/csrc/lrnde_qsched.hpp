// lrnde_qsched.hpp — the compile-time issue schedule of the 4-column kernels' weight stream (lrnde_qtile.hpp, feval_qs).
// Plain constexpr C++17 without HIP types: the device code reads the tables as template constants, and the host checker
// (tests/test_host_qsched.py) simulates them with the host compiler.
//
// An f-eval consumes NB = 14 stream blocks of NQ = 4 quads in order: "point" pt = 4 * I + j is the eight MFMAs of quad j
// of block I (for the partial last block, and for nothing else, a point can be empty).  A block's quad j lives in quad j
// of ONE ring slot.  A table says, for every point, what is requested in front of its MFMAs (`pre`) and behind them
// (`post`), and which slot the MFMAs of block I read (`slot_of`).  Block numbers 14 .. 27 in a request are blocks 0 .. 13
// of the NEXT f-eval of the launch, which streams the same addresses.
//
// Two policies:
//   LEGACY  the closed form the kernels had: point (I, j) requests quad j of block I + R - 1 into slot
//           (slot0 + I + R - 1) % R in front of its MFMAs, whatever kind of block it is (R = ring slots).
//   EARLY   (three slots) a block's quad j is requested the moment the registers that will receive it are dead:
//           - global blocks are requested in block order, quad by quad, at most one quad per point, in front of the
//             MFMAs — that is, right behind the MFMAs that last read those registers;
//           - a register-parked block reserves nothing and requests nothing;
//           - an LDS-parked block is read `lead` points ahead of its own MFMAs, behind the MFMAs of that point, into the
//             slot of the block consumed before it: it inherits that slot (the quad it overwrites was read `lead`
//             points earlier at the latest) and never holds one of its own.  A slot therefore belongs to a CHAIN: a
//             global block and the LDS-parked blocks that directly follow it (register-parked ones skipped);
//           - a global block claims the slot whose chain was consumed longest ago, once quad 0 of that chain's last
//             block has been multiplied; its quad j follows when quad j of that last block has;
//           - a global quad is requested only while at most cap[F] slot quads are busy (requested and not yet
//             multiplied).  The closed form never has more than 9 of the 12 busy: it refills the slot of the block
//             before, and the quads of the current block lie dead behind its MFMAs.  Each quad above 9 is 8 VGPRs,
//             and what the register form of k_step_q has left depends on the stage: every stage adds a k vector (8
//             VGPRs) to the operands a lane keeps;
//           - the last f-eval of a launch requests nothing past block 13; the others at most `wrap` blocks of the next
//             f-eval.  wrap = 2 is what the closed form had in flight across a stage epilogue: with a third block on
//             its way there the epilogue of the register form of k_step_q, which computes in the ring registers the
//             one-quad last block leaves free, spilled 37 VGPRs.
#ifndef LRNDE_QSCHED_HPP
#define LRNDE_QSCHED_HPP

namespace qsched {

constexpr int NB = 14;         // stream blocks per f-eval
constexpr int NQ = 4;          // quads per block
constexpr int NP = NB * NQ;    // points per f-eval
constexpr int MAXSLOT = 4;     // ring slots a table can describe (LRNDE_QRING builds; EARLY is written for three)
constexpr int NEVER = -1000;   // "no block": a slot never used
constexpr int NFEVAL = 6;      // f-evals of a step launch (stages 2 .. 7)

enum : int { SRC_NONE = 0, SRC_GLOBAL = 1, SRC_LDS = 2 };
enum : int { LEGACY = 0, EARLY = 1 };

struct Params {
  unsigned park;   // LDS-parked blocks (bit B)
  unsigned rpark;  // register-parked block
  int kt;          // quads of the last block (13) that exist
  int nslot;       // ring slots
  int policy;
  int lead;        // EARLY: points between the read of an LDS-parked quad and its MFMAs (1 .. NQ)
  int wrap;        // EARLY: blocks of the next f-eval that may be requested before this one ends (0 .. NB)
  int cap[NFEVAL]; // EARLY: slot quads that may hold a requested, not yet multiplied quad at once in f-eval F (<= 4 * nslot)
};

struct Req { int block, quad, slot, src; };

// Slot state between two f-evals.  Block numbers are relative to the f-eval that is about to run; a negative one is a
// block of the f-eval before (all its MFMAs are done).
struct State {
  int slot0;             // LEGACY: slot of block 0
  unsigned resident;     // blocks the head of the launch left in their slots, whatever their kind (first f-eval: 0 and 1)
  int last[MAXSLOT];     // last block of the chain that owns the slot, NEVER = free
  int prev[MAXSLOT];     // last block of the chain that owned it before
  int slot_of[2 * NB];   // slot of every block that has one already, -1 = none yet
  int nreq[2 * NB];      // quads of it requested so far
  int next_global;       // the global block whose quads are requested next
  int busy;              // slot quads requested and not yet multiplied
};

struct Table {
  Req pre[NP], post[NP];
  int slot_of[NB];       // slot the MFMAs of block I read (-1: the register-parked block)
  int slot0;             // LEGACY: the slot of block 0, whatever kind of block it is (the rotation's origin); EARLY: -1
  State exit;
};

constexpr bool has_quad(const Params& p, int b, int j) { return (b % NB) < NB - 1 || j < p.kt; }
constexpr bool is_resident(const State& s, int b) { return b < NB && ((s.resident >> b) & 1u) != 0; }
constexpr bool is_rparked(const Params& p, int b) { return ((p.rpark >> (b % NB)) & 1u) != 0; }
constexpr bool is_lparked(const Params& p, const State& s, int b) {
  return ((p.park >> (b % NB)) & 1u) != 0 && !is_rparked(p, b) && !is_resident(s, b);
}
constexpr bool is_global(const Params& p, const State& s, int b) {
  return !is_rparked(p, b) && !is_lparked(p, s, b) && !is_resident(s, b);
}
// last block of the chain that begins with block b: the LDS-parked blocks that directly follow it, below `limit`
constexpr int chain_end(const Params& p, const State& s, int b, int limit) {
  int e = b;
  for (int n = b + 1; n < limit; ++n) {
    if (is_rparked(p, n)) continue;
    if (is_lparked(p, s, n)) { e = n; continue; }
    break;
  }
  return e;
}

// what the head of k_step_q leaves: blocks 0 and 1 in slots 0 and 1 (stream_init_q), the third slot free
constexpr State entry_state(const Params& p) {
  State s{};
  s.slot0 = 0;
  s.resident = 0x3u;
  for (int i = 0; i < MAXSLOT; ++i) { s.last[i] = NEVER; s.prev[i] = NEVER; }
  for (int b = 0; b < 2 * NB; ++b) { s.slot_of[b] = -1; s.nreq[b] = 0; }
  s.next_global = 0;
  s.busy = 2 * NQ;
  if (p.policy == EARLY) {
    for (int b = 0; b < 2; ++b) {
      const int e = chain_end(p, s, b, b == 0 ? 1 : 2 * NB);  // (block 1 is resident: block 0's chain is itself)
      s.last[b] = e;
      for (int n = b; n <= e; ++n)
        if (n == b || is_lparked(p, s, n)) s.slot_of[n] = b;
      s.nreq[b] = NQ;
    }
  }
  return s;
}

constexpr Req no_req() { return Req{-1, -1, -1, SRC_NONE}; }

// The most slot quads that are busy at once between point pt and the MFMAs of quad g of block G if that quad is
// requested in front of point pt and no other global quad after it: the reads of the LDS-parked blocks on the way are
// not a choice, and the register-parked block multiplies for a whole block without freeing anything.
constexpr int peak_busy(const Params& p, const State& s, int pt, int G, int g, int limit) {
  int b = s.busy + 1, peak = b;
  for (int x = pt; x < G * NQ + g; ++x) {
    const int at = x + p.lead, L = at / NQ, q = at % NQ;
    if (L < limit && is_lparked(p, s, L) && has_quad(p, L, q)) ++b;  // behind the MFMAs of point x
    if (b > peak) peak = b;
    if ((!is_rparked(p, x / NQ) || is_resident(s, x / NQ)) && has_quad(p, x / NQ, x % NQ)) --b;  // quad x is dead
  }
  return peak;
}

constexpr Table legacy_table(const Params& p, const State& in) {
  Table t{};
  const int R = p.nslot;
  for (int pt = 0; pt < NP; ++pt) {
    const int I = pt / NQ, j = pt % NQ, b = I + R - 1;
    Req r = no_req();
    if (!is_rparked(p, b) && has_quad(p, b, j)) {
      r.block = b; r.quad = j; r.slot = (in.slot0 + I + R - 1) % R;
      r.src = ((p.park >> (b % NB)) & 1u) ? SRC_LDS : SRC_GLOBAL;
    }
    t.pre[pt] = r;
    t.post[pt] = no_req();
  }
  for (int I = 0; I < NB; ++I) t.slot_of[I] = is_rparked(p, I) ? -1 : (in.slot0 + I) % R;
  t.slot0 = in.slot0;
  t.exit = in;
  t.exit.slot0 = (in.slot0 + NB) % R;
  t.exit.resident = 0;
  return t;
}

constexpr Table early_table(const Params& p, const State& in, int f) {
  Table t{};
  State s = in;
  const bool lastf = f == NFEVAL - 1;
  const int limit = lastf ? NB : 2 * NB, glimit = lastf ? NB : NB + p.wrap;
  for (int pt = 0; pt < NP; ++pt) {
    t.pre[pt] = no_req();
    t.post[pt] = no_req();
    if (pt > 0) {  // the quad multiplied at the point before is dead
      const int Ip = (pt - 1) / NQ;
      if ((!is_rparked(p, Ip) || is_resident(s, Ip)) && has_quad(p, Ip, (pt - 1) % NQ)) --s.busy;
    }
    // in front of the MFMAs of this point: one quad of the next global block
    while (s.next_global < limit && !is_global(p, s, s.next_global)) ++s.next_global;
    const int G = s.next_global;
    if (G < glimit) {
      if (s.slot_of[G] < 0) {  // claim the slot whose chain was consumed longest ago
        int best = -1;
        for (int c = 0; c < p.nslot; ++c) {
          const bool dead0 = s.last[c] == NEVER || s.last[c] * NQ < pt;
          if (dead0 && (best < 0 || s.last[c] < s.last[best])) best = c;
        }
        if (best >= 0) {
          const int e = chain_end(p, s, G, limit);
          s.prev[best] = s.last[best];
          s.last[best] = e;
          for (int n = G; n <= e; ++n)
            if (n == G || is_lparked(p, s, n)) s.slot_of[n] = best;
        }
      }
      const int c = s.slot_of[G];
      if (c >= 0) {
        const int g = s.nreq[G];
        if ((s.prev[c] == NEVER || s.prev[c] * NQ + g < pt) && peak_busy(p, s, pt, G, g, limit) <= p.cap[f]) {
          t.pre[pt] = Req{G, g, c, SRC_GLOBAL};
          ++s.busy;
          int n = g + 1;
          while (n < NQ && !has_quad(p, G, n)) ++n;
          s.nreq[G] = n;
          if (n == NQ) ++s.next_global;
        }
      }
    }
    // behind them: the quad of an LDS-parked block that is multiplied `lead` points on
    const int at = pt + p.lead, L = at / NQ, q = at % NQ;
    if (L < limit && is_lparked(p, s, L) && has_quad(p, L, q)) {
      t.post[pt] = Req{L, q, s.slot_of[L], SRC_LDS};
      s.nreq[L] = q + 1;
      ++s.busy;
    }
  }
  if ((!is_rparked(p, NB - 1) || is_resident(s, NB - 1)) && has_quad(p, NB - 1, NQ - 1)) --s.busy;
  for (int I = 0; I < NB; ++I) t.slot_of[I] = is_rparked(p, I) ? -1 : s.slot_of[I];
  t.slot0 = -1;
  // the same state seen from the next f-eval
  State x = s;
  x.resident = 0;
  for (int c = 0; c < MAXSLOT; ++c) {
    if (x.last[c] != NEVER) x.last[c] -= NB;
    if (x.prev[c] != NEVER) x.prev[c] -= NB;
  }
  for (int b = 0; b < NB; ++b) { x.slot_of[b] = s.slot_of[b + NB]; x.nreq[b] = s.nreq[b + NB]; }
  for (int b = NB; b < 2 * NB; ++b) { x.slot_of[b] = -1; x.nreq[b] = 0; }
  x.next_global = s.next_global - NB;
  t.exit = x;
  return t;
}

constexpr Table make_table(const Params& p, const State& in, int f) {
  return p.policy == EARLY ? early_table(p, in, f) : legacy_table(p, in);
}

// table of f-eval F (0 .. NFEVAL-1) of a launch: the exit state of one f-eval is the entry state of the next
constexpr Table launch_table(const Params& p, int F) {
  State s = entry_state(p);
  Table t{};
  for (int f = 0; f <= F; ++f) {
    t = make_table(p, s, f);
    s = t.exit;
  }
  return t;
}
// LEGACY table of an f-eval whose block 0 sits in slot slot0 (the kernels with one f-eval, and the chained form
// (QSB * (S - 2)) % QRING of the step kernels)
constexpr Table legacy_table_at(const Params& p, int slot0) {
  State s = entry_state(p);
  s.slot0 = slot0;
  return legacy_table(p, s);
}

// ---- the invariants, as a simulation of one launch: 0 = holds, otherwise the number of the first one that fails ----
// 1  a block's quad is multiplied without having been requested (exactly once, and earlier) into the slot the MFMAs read
// 2  a quad is requested twice, or for a block that needs no request
// 3  a slot quad is written while a block with MFMAs still to run on it owns it
// 4  global requests out of block (or quad) order
// 5  more than 63 requests in flight (`extra` = allowance for the loads and stores of the epilogues)
// 6  the last f-eval requests something past block 13
// 7  an LDS-parked quad is read from the wrong kind of source, or a register-parked block is requested
// 8  EARLY: more than cap[F] slot quads busy
constexpr int check_launch(const Params& p, int extra) {
  // owner[c][j]: absolute block (f * NB + b) whose quad j slot c holds or awaits, -1 = dead
  int owner[MAXSLOT][NQ] = {};
  for (int c = 0; c < MAXSLOT; ++c) for (int j = 0; j < NQ; ++j) owner[c][j] = -1;
  bool requested[(NFEVAL + 1) * NB][NQ] = {};
  bool global_src[(NFEVAL + 1) * NB][NQ] = {};
  for (int b = 0; b < 2; ++b) for (int j = 0; j < NQ; ++j) { owner[b][j] = b; requested[b][j] = true; global_src[b][j] = true; }
  int last_g = -1;  // last global request, as block * NQ + quad
  State s = entry_state(p);
  for (int f = 0; f < NFEVAL; ++f) {
    const bool lastf = f == NFEVAL - 1;
    const Table t = make_table(p, s, f);
    for (int pt = 0; pt < NP; ++pt) {
      const int I = pt / NQ, j = pt % NQ;
      for (int half = 0; half < 2; ++half) {
        if (half == 1) {  // the MFMAs of the point, between `pre` and `post`
          if (is_rparked(p, I)) {  // (what the head left of it in a slot is dead from here on)
            if (t.slot_of[I] != -1) return 1;
            if (f == 0 && I < 2 && owner[I][j] == I) owner[I][j] = -1;
          } else if (has_quad(p, I, j)) {
            const int c = t.slot_of[I];
            if (c < 0 || c >= p.nslot || owner[c][j] != f * NB + I || !requested[f * NB + I][j]) return 1;
            owner[c][j] = -1;
          }
        }
        const Req r = half == 0 ? t.pre[pt] : t.post[pt];
        if (r.src == SRC_NONE) continue;
        if (r.block < 0 || r.block >= 2 * NB || r.quad < 0 || r.quad >= NQ || r.slot < 0 || r.slot >= p.nslot) return 2;
        if (lastf && r.block >= NB && p.policy == EARLY) return 6;
        const int a = f * NB + r.block;
        if (is_rparked(p, r.block) || !has_quad(p, r.block, r.quad)) return 7;
        const bool lds = ((p.park >> (r.block % NB)) & 1u) != 0;
        if (lds != (r.src == SRC_LDS)) return 7;
        if (requested[a][r.quad]) return 2;
        if (a * NQ + r.quad < (f * NB) * NQ + pt + half) return 1;  // not ahead of its own MFMAs
        if (owner[r.slot][r.quad] != -1) return 3;
        owner[r.slot][r.quad] = a;
        requested[a][r.quad] = true;
        if (r.src == SRC_GLOBAL) {
          global_src[a][r.quad] = true;
          if (a * NQ + r.quad <= last_g) return 4;
          last_g = a * NQ + r.quad;
        }
        // in flight: every global quad requested and not yet multiplied, two loads each
        int fl = extra;
        for (int c = 0; c < p.nslot; ++c) for (int q = 0; q < NQ; ++q)
          if (owner[c][q] >= 0 && global_src[owner[c][q]][q]) fl += 2;
        if (fl > 63) return 5;
        int nbusy = 0;
        for (int c = 0; c < p.nslot; ++c) for (int q = 0; q < NQ; ++q) nbusy += owner[c][q] >= 0 ? 1 : 0;
        if (p.policy == EARLY && nbusy > p.cap[f]) return 8;
      }
    }
    if (p.policy == EARLY) {  // a block of this f-eval with a quad left in a slot was never multiplied from there
      for (int c = 0; c < p.nslot; ++c) for (int q = 0; q < NQ; ++q)
        if (owner[c][q] >= 0 && owner[c][q] < (f + 1) * NB) return 1;
      if (lastf) for (int c = 0; c < p.nslot; ++c) for (int q = 0; q < NQ; ++q) if (owner[c][q] >= 0) return 6;
    }
    s = t.exit;
  }
  return 0;
}

// LEGACY equals the closed form: point (I, j) requests quad j of block I + R - 1 into slot (slot0 + I + R - 1) % R
constexpr bool legacy_is_closed_form(const Params& p, int slot0) {
  const Table t = legacy_table_at(p, slot0);
  const int R = p.nslot;
  for (int pt = 0; pt < NP; ++pt) {
    const int I = pt / NQ, j = pt % NQ, b = I + R - 1;
    const bool none = ((p.rpark >> (b % NB)) & 1u) != 0 || ((b % NB) == NB - 1 && j >= p.kt);
    const Req r = t.pre[pt];
    if (t.post[pt].src != SRC_NONE) return false;
    if (none) { if (r.src != SRC_NONE) return false; continue; }
    if (r.block != b || r.quad != j || r.slot != (slot0 + I + R - 1) % R) return false;
    if (r.src != (((p.park >> (b % NB)) & 1u) ? SRC_LDS : SRC_GLOBAL)) return false;
  }
  for (int I = 0; I < NB; ++I)
    if (t.slot_of[I] != (((p.rpark >> I) & 1u) ? -1 : (slot0 + I) % R)) return false;
  return t.exit.slot0 == (slot0 + NB) % R;
}

// The default masks of the register form of k_step_q (LRNDE_QPARK, LRNDE_QRPARK in lrnde_qtile.hpp, where the choice is
// explained) and what the schedule promises for them; any other masks are checked where they are used (QSchedEarly)
constexpr unsigned DEFAULT_PARK = 0x1040u, DEFAULT_RPARK = 0x20u;
constexpr int EPI_INFLIGHT = 24;  // the stage epilogues' own loads and stores that can share the count (EpiFinalQ: 2 + 2 x 6)

// The default caps were derived with one compiler: uncapped, k_step_q<*, 1> needs 24 VGPRs more than the closed form and
// spills (profiles/qsched/resource_usage.txt).  They must be re-derived when tests/test_host_qstep_resources.py, which
// asserts no spill and no private segment on the built kernels, fails after a compiler update.
#define LRNDE_QSCHED_DEFAULT_CAP {12, 12, 12, 12, 11, 10}
constexpr Params default_params(int policy) { return Params{DEFAULT_PARK, DEFAULT_RPARK, 1, 3, policy, 2, 2, LRNDE_QSCHED_DEFAULT_CAP}; }
static_assert(check_launch(default_params(EARLY), EPI_INFLIGHT) == 0,
              "EARLY, default masks: every block of every f-eval requested exactly once and before its first MFMA, no "
              "slot quad written under a block with MFMAs to run, global requests in block order, at most 63 in flight, "
              "nothing past block 13 in the last f-eval");
static_assert(check_launch(default_params(LEGACY), EPI_INFLIGHT) == 0, "LEGACY, default masks");
static_assert(legacy_is_closed_form(default_params(LEGACY), 0) && legacy_is_closed_form(default_params(LEGACY), 1) &&
              legacy_is_closed_form(default_params(LEGACY), 2), "LEGACY is block B + 2 into slot (slot0 + B + 2) % 3 at block B");

}  // namespace qsched

#endif
