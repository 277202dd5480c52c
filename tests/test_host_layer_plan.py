"""csrc/lrnde_layer_plan.hpp on the host: the one statement of the layer forwards' bookkeeping (the solve's saveat for a
mode, the save slot of sol(t1), the "end slot known before the solve" rule, the slot count, the :biased pick, the
corrected-solution filter, the backward pass's stop list) against an independent restatement in plain Python lists,
sorted, bisect and np.float32; and the SDE layer's series plan on its accepted steps against the series rules of
tests/sde_adaptive_np.py (series_plan: the function that helper's forward calls).  Integers and float bit patterns are
compared exactly; no tolerances."""
import bisect, itertools, os, subprocess, textwrap
import numpy as np
import pytest

import sde_adaptive_np as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NONE, UNBIASED, BIASED = 0, 1, 2   # include/lrnde.h LRNDE_MODE_*

SRC = textwrap.dedent(r'''
    #include "lrnde_layer_plan.hpp"
    #include <cstdio>
    #include <cstring>
    #include <initializer_list>
    using namespace lrnde;
    static float rd() { unsigned u = 0; if (scanf("%x", &u) != 1) u = 0; float x; memcpy(&x, &u, 4); return x; }
    static unsigned bits(float x) { unsigned u; memcpy(&u, &x, 4); return u; }
    static void row(const std::vector<float>& v) { printf("%d", (int)v.size()); for (float x : v) printf(" %08x", bits(x)); printf("\n"); }
    int main() {
      static_assert(LRNDE_MODE_NONE == 0 && LRNDE_MODE_UNBIASED == 1 && LRNDE_MODE_BIASED == 2, "the test's mode numbers");
      char kind[4];
      while (scanf("%3s", kind) == 1) {
        if (kind[0] == 'B') {   // B r m -> the :biased index
          const float r = rd(); int m;
          if (scanf("%d", &m) != 1) return 2;
          printf("%d\n", biased_pick(r, m));
        } else if (kind[0] == 'K') {   // K needs_correction t1 t -> kept?
          int nc; if (scanf("%d", &nc) != 1) return 2;
          const float t1 = rd(), t = rd();
          printf("%d\n", series_keeps(nc != 0, t1, t) ? 1 : 0);
        } else if (kind[0] == 'S') {   // S t0 t2 n ts[n] -> the stop list
          const float t0 = rd(), t2 = rd(); int n;
          if (scanf("%d", &n) != 1) return 2;
          std::vector<float> ts(n);
          for (float& x : ts) x = rd();
          row(backward_stops(ts, t0, t2));
        } else if (kind[0] == 'E') {   // E t0 t2 nfine mode save_start t1_or_rand K (i m)[K] nuser user[nuser] -> the SDE layer's series plan
          struct Step { int x, y; };
          const float t0 = rd(), t2 = rd(); int nfine, mode, save_start, K, nuser;
          if (scanf("%d %d %d", &nfine, &mode, &save_start) != 3) return 2;
          const float r = rd();
          if (scanf("%d", &K) != 1) return 2;
          std::vector<Step> im(K);
          for (Step& e : im) if (scanf("%d %d", &e.x, &e.y) != 2) return 2;
          if (scanf("%d", &nuser) != 1) return 2;
          std::vector<float> user(nuser);
          for (float& x : user) x = rd();
          const SdeSeriesPlan p = sde_series_plan(t0, t2, nfine, im.data(), K, mode, r, save_start, user.data(), nuser);
          printf("%d", p.status);
          if (p.status == SERIES_OK) {
            printf(" %08x %08x %d %08x", bits(p.t1), bits(p.e1.t), p.e1.k, bits(p.e1.theta));
            for (const std::vector<SdeSeriesEntry>* v : {&p.sol, &p.series}) {
              printf(" %d", (int)v->size());
              for (const SdeSeriesEntry& e : *v) printf(" %08x %d %08x", bits(e.t), e.k, bits(e.theta));
            }
          }
          printf("\n");
        } else {   // P mode save_start maxiters t0 t1 t2 nuser user[nuser]
          int mode, save_start, maxiters, nuser;
          if (scanf("%d %d %d", &mode, &save_start, &maxiters) != 3) return 2;
          const float t0 = rd(), t1 = rd(), t2 = rd();
          if (scanf("%d", &nuser) != 1) return 2;
          std::vector<float> user(nuser);
          for (float& x : user) x = rd();
          const SolveSaveat p = solve_saveat(mode, t1, t2, user.data(), nuser);
          printf("%d %d\n", p.save_everystep, p.needs_correction ? 1 : 0);
          row(p.saveat);
          std::vector<float> other = user;   // the second form of vcat(saveat, t1): append, then sort stably
          other.push_back(t1); std::stable_sort(other.begin(), other.end());
          row(other);
          const int nsv = (int)p.saveat.size();
          printf("%d %d %zu\n", slot_of_t1(p.saveat.data(), nsv, t0, t1, save_start), end_slot_known(p.saveat.data(), nsv, t0, t2, save_start),
                 slots_needed(mode, nuser, maxiters));
          printf("%d", nsv);   // what the corrected solution keeps of a series saved at exactly these times
          for (float x : p.saveat) printf(" %d", series_keeps(p.needs_correction, t1, x) ? 1 : 0);
          printf("\n");
        }
      }
      return 0;
    }
''')


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("layer_plan")
    src = d / "t.cpp"
    src.write_text(SRC)
    exe = d / "t"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "localregneuralde.jl_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)

    def run(text):
        r = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout.split("\n")
    return run


def bits(x):
    return int(np.array([x], dtype=f32).view(np.uint32)[0])


def hx(x):
    return "%08x" % bits(f32(x))


def vec(xs):
    return " ".join([str(len(xs))] + [hx(x) for x in xs])


# ---- the restatement ----
def plan(mode, t1, t2, user):
    """(saveat of the solve, save_everystep, needs_correction): src/layers/neural_ode.jl:56-116"""
    user = [f32(x) for x in user]
    if mode == UNBIASED:
        if user:
            sv = list(user)
            sv.insert(bisect.bisect_right(sv, f32(t1)), f32(t1))
            return sv, 0, 1
        return [f32(t1), f32(t2)], 0, 0
    if user:
        return user, 0, 0
    return ([], 1, 0) if mode == BIASED else ([f32(t2)], 0, 0)


def slot_of_t1(sv, t0, t1, save_start):
    """the save slot of the last entry equal to t1: entries at or before t0 take none, a start slot comes first"""
    at = [k for k, s in enumerate(sv) if s == f32(t1)]
    if not at or not sv[at[-1]] > f32(t0):
        return -1
    return sum(1 for s in sv[:at[-1]] if s > f32(t0)) + (1 if save_start else 0)


def end_slot(sv, t0, t2, save_start):
    if save_start or not sv or not all(f32(t0) < s <= f32(t2) for s in sv):
        return -1
    return len(sv) - 1


def slots_needed(mode, nuser, maxiters):
    if nuser:
        return nuser + 3
    if mode == BIASED:
        return maxiters + 2 if maxiters < 510 else 512
    return 3


def pick(r, m):
    return min(max(int(f32(r) * f32(m)), 0), m - 1)   # (int() truncates towards zero, as the C cast does)


def stops(ts, t0, t2):
    return [-f32(t) for t in reversed(ts) if f32(t0) < f32(t) < f32(t2)]


T0, T2 = 0.0, 1.0
JUST_ABOVE = float(np.nextafter(f32(T0), f32(1)))
T1S = {"t0": T0, "just_above_t0": JUST_ABOVE, "middle": 0.375, "user_entry": None, "t2": T2}
USERS = {"none": [], "one": [0.5], "several": [0.25, 0.5, 1.0], "duplicates": [0.25, 0.5, 0.5, 1.0],
         "at_or_before_t0": [-0.5, 0.0, 0.5, 1.0], "contains_t1": None, "ends_before_t2": [0.25, 0.75]}


def plan_cases():
    for mode, save_start, (un, user), (tn, t1) in itertools.product((NONE, UNBIASED, BIASED), (0, 1), USERS.items(), T1S.items()):
        if t1 is None:
            t1 = user[len(user) // 2] if user else 0.5
        if user is None:
            user = sorted([0.25, t1, 1.0])
        for maxiters in ((100, 509, 510, 1000) if (un, tn, save_start) == ("none", "middle", 0) else (1000,)):
            yield mode, save_start, maxiters, un, user, tn, t1


def test_plan_enumeration(driver):
    cases = list(plan_cases())
    assert len(cases) == 3 * 2 * 7 * 5 + 3 * 3
    out = driver("".join("P %d %d %d %s %s %s %s\n" % (mode, ss, mi, hx(T0), hx(t1), hx(T2), vec(user))
                         for mode, ss, mi, _, user, _, t1 in cases))
    seen = set()
    for i, (mode, ss, mi, un, user, tn, t1) in enumerate(cases):
        ln = out[5 * i:5 * i + 5]
        what = (mode, ss, mi, un, tn)
        sv, everystep, nc = plan(mode, t1, T2, user)
        assert ln[0] == "%d %d" % (everystep, nc), (what, ln[0])
        assert ln[1] == vec(sv), (what, ln[1], vec(sv))
        # vcat(saveat, t1) sorted: insertion behind the equal entries and append + stable sort are the same vector
        appended = sorted([f32(x) for x in user] + [f32(t1)])
        assert ln[2] == vec(appended), (what, ln[2])
        if mode == UNBIASED and user:
            assert ln[1] == ln[2], (what, ln[1], ln[2])
        slot, end, need = slot_of_t1(sv, T0, t1, ss), end_slot(sv, T0, T2, ss), slots_needed(mode, len(user), mi)
        assert ln[3] == "%d %d %d" % (slot, end, need), (what, ln[3], slot, end, need)
        keep = [0 if (nc and s == f32(t1)) else 1 for s in sv]
        assert ln[4] == " ".join(str(v) for v in [len(sv)] + keep), (what, ln[4], keep)
        # every slot the plan names fits the slots it asks for (the solve may add a start slot and saves at most sv)
        assert everystep or (slot < need and end < need and len(sv) + ss <= need), what
        if mode == UNBIASED:
            seen.add(("slot", slot >= 0)), seen.add(("end", end >= 0)), seen.add(("dropped", len(sv) - sum(keep)))
            if slot >= 0:   # the slot is that of sol(t1) in the series the solve saves: [start value] + entries after t0
                saved = ([f32(T0)] if ss else []) + [s for s in sv if s > f32(T0)]
                assert saved[slot] == f32(t1) and (slot + 1 == len(saved) or saved[slot + 1] != f32(t1)), what
    assert seen >= {("slot", True), ("slot", False), ("end", True), ("end", False), ("dropped", 0), ("dropped", 1), ("dropped", 2),
                    ("dropped", 3)}, seen


def test_biased_pick(driver):
    ms = (1, 2, 3, 511, 512, 2 ** 24 + 1)
    rs = (0.0, 0.5, float(np.nextafter(f32(1), f32(0))), 1.0, -0.0)
    grid = list(itertools.product(ms, rs))
    out = driver("".join("B %s %d\n" % (hx(r), m) for m, r in grid))
    for (m, r), ln in zip(grid, out):
        got = int(ln)
        assert 0 <= got <= m - 1, (m, r, got)
        assert got == pick(r, m), (m, r, got, pick(r, m))
    assert pick(rs[2], 512) == 511 and pick(1.0, 512) == 511 and pick(0.5, 3) == 1 and pick(-0.0, 3) == 0


def test_corrected_solution_filter(driver):
    nan = float("nan")
    grid = [(nc, t1, t) for nc in (0, 1) for t1, t in ((0.5, 0.5), (0.5, 0.25), (0.0, -0.0), (nan, nan), (nan, 0.5), (0.5, nan))]
    out = driver("".join("K %d %s %s\n" % (nc, hx(t1), hx(t)) for nc, t1, t in grid))
    for (nc, t1, t), ln in zip(grid, out):
        assert int(ln) == (0 if (nc and f32(t) == f32(t1)) else 1), (nc, t1, t, ln)
    assert [int(ln) for ln in out[6:12]] == [0, 1, 0, 1, 1, 1]   # a NaN "no drop" never matches


def test_backward_stops(driver):
    cases = {
        "inside": [0.25, 0.5, 1.0],
        "at_t0_and_t2": [0.0, 0.25, 1.0, 1.0],
        "repeated": [0.25, 0.5, 0.5, 0.5, 0.75, 1.0],
        "start_slot_and_before": [-0.5, 0.0, 0.0, 0.5],
        "only_ends": [0.0, 1.0],
        "empty": [],
    }
    out = driver("".join("S %s %s %s\n" % (hx(T0), hx(T2), vec(ts)) for ts in cases.values()))
    for (name, ts), ln in zip(cases.items(), out):
        assert ln == vec(stops(ts, T0, T2)), (name, ln)
    assert stops(cases["at_t0_and_t2"], T0, T2) == [-0.25] and stops(cases["repeated"], T0, T2) == [-0.75, -0.5, -0.5, -0.5, -0.25]
    assert stops(cases["only_ends"], T0, T2) == []


# ---- the SDE layer's series on the accepted steps of its solve ----
ST0, ST2, NF = 0.25, 1.75, 24    # h = 1/16
SERIES_OK, T1_OUTSIDE, SAVES_NOTHING, BIASED_NEEDS_TWO, T1_AT_END = range(5)
REFUSALS = {"t1 outside tspan": T1_OUTSIDE, "the solve saves nothing": SAVES_NOTHING, ":biased needs at least two saved times": BIASED_NEEDS_TWO,
            "t1 must lie before the end of tspan": T1_AT_END}
MODES = {NONE: "none", UNBIASED: "unbiased", BIASED: "biased"}
STEPS = {"single": [(0, 24)], "uneven": [(0, 1), (1, 5), (6, 2), (8, 11), (19, 5)], "overshoot": [(0, 7), (7, 9), (16, 11)]}
T1 = 0.8125   # inside a step of every list, on a grid point of none's end


def series_saveats(steps):
    h = f32(f32(f32(ST2) - f32(ST0)) / f32(NF))
    i, m = steps[len(steps) // 2]
    inside = f32(f32(ST0) + f32(f32(i) + f32(0.5) * f32(m)) * h)      # strictly inside the middle step
    i0, m0 = steps[0]
    end0 = f32(ST2) if i0 + m0 >= NF else f32(f32(ST0) + f32(i0 + m0) * h)   # the first step's end as the plan computes it
    il, ml = steps[-1]
    behind = float(np.nextafter(f32(f32(ST0) + f32(min(il + ml, NF)) * h), f32(-1)))   # just behind the grid's end, where tk1 is t2 itself
    return {"none": [], "ends_and_mid": [ST0, 1.0, ST2], "equals_t1": [0.5, T1, 1.5], "inside_a_step": [float(inside)],
            "a_steps_end": sorted([float(end0), 1.5]), "behind_the_last_step": [behind, ST2]}


def series_line(t0, t2, nfine, mode, save_start, r, steps, user):
    return "E %s %s %d %d %d %s %d %s %s\n" % (hx(t0), hx(t2), nfine, mode, save_start, hx(r), len(steps), " ".join("%d %d" % s for s in steps), vec(user))


def series_want(t0, t2, nfine, mode, save_start, r, steps, user):
    try:
        sol, e1, t1, series = S.series_plan(t0, t2, nfine, steps, MODES[mode], r, save_start, user)
    except AssertionError as e:
        return str(REFUSALS[str(e)]), None
    if e1 is None:
        e1 = (f32(t2), len(steps) - 1, f32(1))   # (:none has no local step: the end of the solve)
    ent = lambda e: "%s %d %s" % (hx(e[0]), e[1], hx(e[2]))
    return " ".join([str(SERIES_OK), hx(t1), ent(e1)] + [" ".join([str(len(v))] + [ent(e) for e in v]) for v in (sol, series)]), (sol, e1, series)


def test_sde_series_plan(driver):
    cases = [(mode, ss, r, sn, un) for mode, ss, sn in itertools.product((NONE, UNBIASED, BIASED), (-1, 0, 1), STEPS)
             for un in series_saveats(STEPS[sn]) for r in ((T1,) if mode == UNBIASED else (0.0, 0.6) if mode == BIASED else (0.5,))]
    out = driver("".join(series_line(ST0, ST2, NF, mode, ss, r, STEPS[sn], series_saveats(STEPS[sn])[un]) for mode, ss, r, sn, un in cases))
    seen = set()
    for (mode, ss, r, sn, un), ln in zip(cases, out):
        want, parts = series_want(ST0, ST2, NF, mode, ss, r, STEPS[sn], series_saveats(STEPS[sn])[un])
        assert ln == want, ((mode, ss, r, sn, un), ln, want)
        if parts is None:
            seen.add(("refused", int(want)))
            continue
        sol, e1, series = parts
        seen.add(("start", sol[0][1] == -1)), seen.add(("dropped", len(sol) - len(series)))
        seen |= {("theta", "inside" if 0 < e[2] < 1 else "end") for e in sol if e[1] >= 0}
        seen |= {("e1", "inside" if 0 < e1[2] < 1 else "end" if e1[1] >= 0 else "start")}
        if un == "a_steps_end" and ss == 0:   # an entry equal to a step's end is that step's end state, not the next step's start
            assert [(e[1], e[2]) for e in sol if e[0] == series_saveats(STEPS[sn])[un][0 if sn != "single" else 1]] == [(0, 1)]
        if un == "behind_the_last_step" and mode == NONE and ss == 0:   # inside the last step, then t2 itself: theta < 1, then 1
            assert sol[0][1] == sol[1][1] == len(STEPS[sn]) - 1 and 0 < sol[0][2] < 1 and sol[1][2] == 1 and sol[1][0] == f32(ST2)
    assert seen >= {("start", True), ("start", False), ("dropped", 0), ("dropped", 1), ("dropped", 2), ("theta", "inside"), ("theta", "end"),
                    ("e1", "inside"), ("e1", "end"), ("e1", "start"), ("refused", BIASED_NEEDS_TWO)}, seen
    # the four refusals, each alone: t1 past the span; every step of a solve that took none; one saved time; t1 at the end
    refusals = [((UNBIASED, -1, 2.0, [(0, 24)], []), T1_OUTSIDE), ((UNBIASED, -1, float("nan"), [(0, 24)], []), T1_OUTSIDE),
                ((BIASED, 0, 0.5, [], []), SAVES_NOTHING), ((BIASED, 0, 0.5, [(0, 24)], [1.0]), BIASED_NEEDS_TWO),
                ((UNBIASED, -1, ST2, [(0, 24)], []), T1_AT_END), ((UNBIASED, 1, ST2, [(0, 24)], [0.5]), T1_AT_END)]
    out = driver("".join(series_line(ST0, ST2, NF, mode, ss, r, steps, user) for (mode, ss, r, steps, user), _ in refusals))
    for ((mode, ss, r, steps, user), code), ln in zip(refusals, out):
        assert ln == str(code) == series_want(ST0, ST2, NF, mode, ss, r, steps, user)[0], (mode, ss, r, steps, user, ln)
