"""csrc/lrnde_qsched.hpp on the host: the compile-time issue schedule of the 4-column kernels' weight stream.  A small
stand-alone checker, compiled with the host compiler, walks the six chained f-evals of a step launch point by point with a
model of the three ring slots of its own (which quad of which f-eval's block a slot quad holds) and asserts, for every
LDS-park mask of at most two blocks, every register-park mask of at most one block disjoint from it, KT = 1 and 4 and
every lead of the parked reads, with the default caps on the busy slot quads and two blocks requested across a stage
epilogue, and with neither limit (all twelve quads, three blocks):

  * every quad of every block of every f-eval is requested exactly once, before its MFMAs, into the slot they read;
  * no slot quad is written while a block with MFMAs still to run owns it;
  * global requests are issued in block (and quad) order;
  * never more than 63 requests in flight per wave, the epilogues' own allowance included;
  * never more slot quads busy (requested, not yet multiplied) than the f-eval's cap;
  * the last f-eval requests nothing past block 13, and no f-eval leaves a quad of its own blocks behind;
  * the `legacy` policy is the closed form: block B + 2, quad j into slot (slot0 + B + 2) % 3 at point (B, j).

The slot model carries the f-eval a quad belongs to: every f-eval streams the same weights, so a block that is never
requested but still sits in its slot from the f-eval before computes the right bits on the GPU and only this sees it.
The checker is also run on schedules with one request removed, moved or doubled, which it has to refuse."""
import os
import subprocess
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = textwrap.dedent(r'''
    #include "lrnde_qsched.hpp"
    #include <cstdio>
    #include <cstring>
    #include <string>
    #include <vector>
    using namespace qsched;

    // the tables of a launch, chained through their exit states
    static std::vector<Table> tables(const Params& p) {
      std::vector<Table> v;
      State s = entry_state(p);
      for (int f = 0; f < NFEVAL; ++f) { v.push_back(make_table(p, s, f)); s = v.back().exit; }
      return v;
    }

    // "" = every invariant holds
    static std::string simulate(const Params& p, const std::vector<Table>& tabs) {
      const int NA = (NFEVAL + 1) * NB * NQ;           // absolute quads: (f * NB + block) * NQ + quad
      std::vector<int> nreq(NA, 0), done(NA, 0), glob(NA, 0);
      int occ[3][NQ];                                   // absolute quad a slot quad holds or awaits, -1 = dead
      for (auto& a : occ) for (int& x : a) x = -1;
      for (int b = 0; b < 2; ++b) for (int q = 0; q < NQ; ++q) { occ[b][q] = b * NQ + q; nreq[b * NQ + q] = 1; glob[b * NQ + q] = 1; }
      int last_global = -1;
      char msg[160];
      auto rparked = [&](int b) { return ((p.rpark >> (b % NB)) & 1u) != 0; };
      auto exists = [&](int b, int q) { return (b % NB) != NB - 1 || q < p.kt; };
      for (int f = 0; f < NFEVAL; ++f) {
        const Table& t = tabs[f];
        for (int pt = 0; pt < NP; ++pt) {
          const int I = pt / NQ, j = pt % NQ, now = f * NP + pt;
          for (int half = 0; half < 2; ++half) {
            if (half == 1) {   // the MFMAs of the point
              const int a = now;
              if (rparked(I)) {
                if (t.slot_of[I] != -1) return "register-parked block has a slot";
                if (f == 0 && I < 2 && occ[I][j] == a) occ[I][j] = -1;   // what the head left of it
              } else if (exists(I, j)) {
                const int c = t.slot_of[I];
                if (c < 0 || c > 2) { snprintf(msg, sizeof msg, "f%d block %d: no slot", f, I); return msg; }
                if (nreq[a] != 1 || occ[c][j] != a) {
                  snprintf(msg, sizeof msg, "f%d block %d quad %d: multiplied from slot %d, which holds %d (requested %d times)", f, I, j, c, occ[c][j], nreq[a]);
                  return msg;
                }
                occ[c][j] = -1; done[a] = 1;
              }
            }
            const Req r = half == 0 ? t.pre[pt] : t.post[pt];
            if (r.src == SRC_NONE) continue;
            if (r.block < 0 || r.block >= 2 * NB || r.quad < 0 || r.quad >= NQ || r.slot < 0 || r.slot > 2) return "request out of range";
            const int a = (f * NB + r.block) * NQ + r.quad;
            snprintf(msg, sizeof msg, "f%d point %d%s: block %d quad %d into slot %d: ", f, pt, half ? " (behind)" : "", r.block, r.quad, r.slot);
            const std::string at = msg;
            if (p.policy == EARLY && f == NFEVAL - 1 && r.block >= NB) return at + "the last f-eval requests past block 13";
            if (rparked(r.block)) return at + "a register-parked block is requested";
            if (!exists(r.block, r.quad)) return at + "a quad that does not exist";
            if ((((p.park >> (r.block % NB)) & 1u) != 0) != (r.src == SRC_LDS)) return at + "wrong source";
            if (nreq[a]++) return at + "requested twice";
            if (a < now + half) return at + "behind its own MFMAs";
            if (occ[r.slot][r.quad] != -1) return at + "the slot quad is owned by a block with MFMAs to run";
            occ[r.slot][r.quad] = a;
            if (r.src == SRC_GLOBAL) {
              glob[a] = 1;
              if (a <= last_global) return at + "global requests out of order";
              last_global = a;
            }
            int fl = EPI_INFLIGHT;
            for (auto& s : occ) for (int x : s) if (x >= 0 && glob[x]) fl += 2;
            if (fl > 63) return at + "more than 63 in flight";
            int nbusy = 0;
            for (auto& s : occ) for (int x : s) nbusy += x >= 0;
            if (p.policy == EARLY && nbusy > p.cap[f]) return at + "more slot quads busy than the f-eval's cap";
          }
        }
        for (int c = 0; c < 3; ++c) for (int q = 0; q < NQ; ++q) {
          if (occ[c][q] >= 0 && occ[c][q] < (f + 1) * NP) return "a quad of a finished f-eval was left in its slot";
          if (p.policy == EARLY && f == NFEVAL - 1 && occ[c][q] >= 0) return "the launch ends with a request nobody reads";
        }
      }
      return "";
    }

    static bool closed_form(const Params& p, const std::vector<Table>& tabs) {
      for (int f = 0; f < NFEVAL; ++f) {
        const int slot0 = (NB * f) % 3;
        for (int pt = 0; pt < NP; ++pt) {
          const int B = pt / NQ, j = pt % NQ, b = B + 2;
          const Req r = tabs[f].pre[pt];
          if (tabs[f].post[pt].src != SRC_NONE) return false;
          const bool none = ((p.rpark >> (b % NB)) & 1u) || ((b % NB) == NB - 1 && j >= p.kt);
          if (none) { if (r.src != SRC_NONE) return false; continue; }
          if (r.block != b || r.quad != j || r.slot != (slot0 + B + 2) % 3) return false;
          if (r.src != (((p.park >> (b % NB)) & 1u) ? SRC_LDS : SRC_GLOBAL)) return false;
        }
        for (int B = 0; B < NB; ++B) if (tabs[f].slot_of[B] != (((p.rpark >> B) & 1u) ? -1 : (slot0 + B) % 3)) return false;
        // the burst form (LRNDE_QBURST) loads block B + 2 whole at block B into slot (tab.slot0 + B + 2) % 3, whatever kind
        // of block B or B + 2 is: that has to be the slot the quad-wise requests name and the MFMAs of B + 2 read
        if (tabs[f].slot0 != slot0) return false;
        for (int B = 0; B < NB; ++B) {
          const int dst = (tabs[f].slot0 + B + 2) % 3;
          if (tabs[f].pre[B * NQ].src != SRC_NONE && tabs[f].pre[B * NQ].slot != dst) return false;
          if (B + 2 < NB && tabs[f].slot_of[B + 2] != -1 && tabs[f].slot_of[B + 2] != dst) return false;
        }
        const Table one = legacy_table_at(p, slot0);   // the form the single f-eval kernels and the LDS form use
        if (memcmp(one.pre, tabs[f].pre, sizeof one.pre) || memcmp(one.slot_of, tabs[f].slot_of, sizeof one.slot_of)) return false;
      }
      return true;
    }

    int main(int argc, char** argv) {
      const std::string mode = argc > 1 ? argv[1] : "all";
      if (mode == "all") {
        int n = 0, bad = 0;
        for (int kt : {1, 4})
          for (int a = -1; a < NB; ++a)
            for (int b = a; b < NB; ++b) {
              if (a >= 0 && b == a) continue;            // (a = -1: no or one block; a >= 0: the pairs a < b)
              const unsigned park = (a >= 0 ? 1u << a : 0u) | (b >= 0 ? 1u << b : 0u);
              for (int r = -1; r < NB - 1; ++r) {
                const unsigned rp = r >= 0 ? 1u << r : 0u;
                if (rp & park) continue;
                for (int lw = 0; lw < 2 * NQ; ++lw) {     // every lead, with two and with three blocks across the epilogue
                  const int lead = 1 + lw % NQ;
                  const Params e = lw < NQ ? Params{park, rp, kt, 3, EARLY, lead, 2, LRNDE_QSCHED_DEFAULT_CAP}
                                           : Params{park, rp, kt, 3, EARLY, lead, 3, {12, 12, 12, 12, 12, 12}};
                  const std::string m = simulate(e, tables(e));
                  const int own = check_launch(e, EPI_INFLIGHT);
                  ++n;
                  if (!m.empty() || own != 0) { ++bad; printf("EARLY park %#x rpark %#x kt %d lead %d wrap %d: %s (check_launch %d)\n", park, rp, kt, lead, e.wrap, m.c_str(), own); }
                  for (int f = 0; f < NFEVAL; ++f)       // launch_table(F) is the chain
                    if (memcmp(launch_table(e, f).pre, tables(e)[f].pre, sizeof(Table::pre))) { ++bad; printf("launch_table differs\n"); }
                }
                const Params l{park, rp, kt, 3, LEGACY, 0, 0, {}};
                const std::string m = simulate(l, tables(l));
                ++n;
                if (!m.empty() || !closed_form(l, tables(l)) || check_launch(l, EPI_INFLIGHT) != 0) { ++bad; printf("LEGACY park %#x rpark %#x kt %d: %s\n", park, rp, kt, m.c_str()); }
              }
            }
        printf("cases %d bad %d\n", n, bad);
        return bad != 0;
      }
      // broken schedules the checker has to refuse: the default masks' EARLY tables with one request changed
      const Params e = default_params(EARLY);
      std::vector<Table> v = tables(e);
      int pt9 = -1;                                      // where f-eval 1 requests quad 2 of block 9
      for (int pt = 0; pt < NP; ++pt) if (v[1].pre[pt].block == 9 && v[1].pre[pt].quad == 2) pt9 = pt;
      if (pt9 < 0) { printf("no such request\n"); return 2; }
      if (mode == "dropped") v[1].pre[pt9] = no_req();   // block 9 of f-eval 0 still lies in a slot: same bits on the GPU
      else if (mode == "doubled") v[1].post[pt9] = v[1].pre[pt9];
      else if (mode == "early") { v[1].pre[0] = v[1].pre[pt9]; v[1].pre[pt9] = no_req(); }   // over a quad not multiplied yet / out of order
      else if (mode == "wrap") { for (int pt = 0; pt < NP; ++pt) if (v[4].pre[pt].block >= NB) { v[5].pre[NP - 1] = v[4].pre[pt]; break; } }
      else if (mode == "slot") v[1].slot_of[9] = (v[1].slot_of[9] + 1) % 3;
      else return 2;
      const std::string m = simulate(e, v);
      printf("%s\n", m.c_str());
      return m.empty() ? 0 : 1;
    }
''')


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    d = tmp_path_factory.mktemp("qsched")
    src = d / "t.cpp"
    src.write_text(SRC)
    exe = d / "t"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "localregneuralde.jl_amd", "csrc"),
                    str(src), "-o", str(exe)], check=True)

    def run(mode):
        return subprocess.run([str(exe), mode], capture_output=True, text=True)
    return run


def test_every_mask_every_chain_holds_the_invariants(checker):
    """all park masks x KT x lead, EARLY and LEGACY, six chained f-evals; LEGACY against the closed form; the header's
    own check_launch agrees"""
    r = checker("all")
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr
    last = r.stdout.strip().split("\n")[-1].split()
    lds = [()] + [(a,) for a in range(14)] + [(a, b) for a in range(14) for b in range(a + 1, 14)]
    pairs = sum(1 for m in lds for rp in [None] + list(range(13)) if rp not in m)
    assert last[0] == "cases" and int(last[1]) == 2 * (8 + 1) * pairs and last[3] == "0", r.stdout[-400:]   # KT x (leads x wraps + legacy)


@pytest.mark.parametrize("mode", ["dropped", "doubled", "early", "wrap", "slot"])
def test_a_broken_schedule_is_refused(checker, mode):
    """`dropped`: block 9 of the second f-eval is never requested; its slot still holds the first f-eval's block 9"""
    r = checker(mode)
    assert r.returncode == 1 and r.stdout.strip(), (r.returncode, r.stdout, r.stderr)
