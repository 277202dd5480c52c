"""csrc/lrnde_stepctl.hpp on the host: the one statement of the PI step-size controller, the accept snap, loopheader!'s
clamp and status, and ode_determine_initdt's dt0 rule and tail, against an independent restatement in numpy float32
(oracle/np_restatement.py's fastpow, _eps and f32; math.pow / math.log10 — the driver's libm — on the exact paths).
Bit for bit, NaN equal to NaN; no tolerances."""
import itertools, math, os, subprocess, textwrap
import numpy as np
import pytest

from np_restatement import fastpow, _eps, f32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OK, MAXITERS, DT_LESS_THAN_MIN, DT_NAN, DONE = 0, 1, 2, 3, 100   # include/lrnde.h; DONE: t reached t1

SRC = textwrap.dedent(r'''
    #include "lrnde_stepctl.hpp"
    #include <cstdio>
    #include <cstring>
    #include <cstdint>
    #include <vector>
    using namespace lrnde;
    static float rd() { unsigned u = 0; if (scanf("%x", &u) != 1) u = 0; float x; memcpy(&x, &u, 4); return x; }
    static unsigned bits(float x) { unsigned u; memcpy(&u, &x, 4); return u; }
    int main() {
      char kind[4];
      while (scanf("%3s", kind) == 1) {
        if (kind[0] == 'I') {   // I d0 d1 d2 dtmax order -> dt0, dt
          const float d0 = rd(), d1 = rd(), d2 = rd(), dtmax = rd(), order = rd();
          const float dt0 = initdt_dt0(d0, d1, dtmax);
          printf("%08x %08x\n", bits(dt0), bits(initdt_tail(dt0, d1, d2, order, dtmax)));
          continue;
        }
        if (kind[0] == 'S') {   // S n s0 s1 stops[n] m t[m] -> per t: the attempt's end time, the cursor's index
          int n, m;
          if (scanf("%d", &n) != 1) return 2;
          const float s0 = rd(), s1 = rd();
          std::vector<float> stops(n);
          for (float& x : stops) x = rd();
          if (scanf("%d", &m) != 1) return 2;
          TstopCursor c{stops.data(), stops.size(), 0};
          (void)s0;   // (the first t of a solve is s0: entries <= s0 are passed by that call)
          for (int i = 0; i < m; ++i) {
            const float e = tstop_next(c, rd(), s1);
            printf("%08x %d\n", bits(e), (int)c.i);
          }
          continue;
        }
        // C set exact_pow snap maxiters n t0 t1 dt_init eest[n]: one row per attempt, every attempt towards t1
        // T ... eest[n] tend[n + 1]: the same with attempt i towards tend[i] (a solve with tstops)
        int set, exact, snap, maxiters, n;
        if (scanf("%d %d %d %d %d", &set, &exact, &snap, &maxiters, &n) != 5) return 2;
        const float t0 = rd(), t1 = rd(), dt_init = rd();
        std::vector<float> ee(n), tend(n + 1, t1);
        for (float& e : ee) e = rd();
        if (kind[0] == 'T') for (float& e : tend) e = rd();
        AttemptLoop L = attempt_begin(set ? pi_order3() : pi_tsit5(), exact, maxiters, snap, t0, t1, dt_init);
        attempt_header(L, tend[0]);
        int status = L.status;
        printf("%d %08x\n", status, bits(L.dt));
        for (int i = 0; i < n && status == 0; ++i) {
          attempt_judge(L, ee[i]);
          status = L.status;
          if (status == 0) {
            if (!(L.t < t1)) status = 100;
            else { attempt_header(L, tend[i + 1]); status = L.status; }
          }
          printf("%08x %d %08x %08x %08x %d\n", bits(L.q11), L.accept, bits(L.t), bits(L.dtpropose), bits(L.dt), status);
        }
        printf("end\n");
      }
      return 0;
    }
''')


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("stepctl")
    src = d / "t.cpp"
    src.write_text(SRC)
    exe = d / "t"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "localregneuralde.jl_amd", "csrc"),
                    str(src), "-o", str(exe)], check=True)

    def run(text):
        r = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout.split("\n")
    return run


def bits(x):
    return int(np.array([x], dtype=f32).view(np.uint32)[0])


def hx(x):
    return "%08x" % bits(f32(x))


def same(a, b):
    """equal bits, or both NaN"""
    fa, fb = np.array([a], np.uint32).view(f32)[0], np.array([b], np.uint32).view(f32)[0]
    return a == b or (np.isnan(fa) and np.isnan(fb))


fmin, fmax = np.fmin, np.fmax   # C fminf / fmaxf: the operand that is not NaN
CONSTS = {0: (f32(0.9), f32(0.2), f32(10.0), f32(7.0 / 50.0), f32(2.0 / 25.0)),     # Tsit5
          1: (f32(0.9), f32(0.2), f32(10.0), f32(7.0 / 30.0), f32(2.0 / 15.0))}     # VCAB3 / VCABM3
ONE = f32(1)


def powf(exact, x, y):
    return f32(math.pow(float(x), float(y))) if exact else fastpow(x, y)


def clamp_status(dt, dtmax, dtmin, t, t1, it, maxiters):
    dt = fmax(fmin(dtmax, dt), dtmin)
    dt = fmin(f32(abs(dt)), f32(abs(f32(t1 - t))))
    if it > maxiters:
        return dt, MAXITERS
    if np.isnan(dt):
        return dt, DT_NAN
    if abs(dt) <= abs(dtmin):
        return dt, DT_LESS_THAN_MIN
    return dt, OK


def restate(cset, exact, snap, maxiters, t0, t1, dt, eests, tends=None):
    """the loops' recurrence: rows of (q11, accept, t, dtpropose, next dt, status).  tends: the end time
    of each attempt (a tstop or t1; one more than eests), every one t1 when not given"""
    gamma, qmin, qmax, beta1, beta2 = CONSTS[cset]
    t0, t1, dt = f32(t0), f32(t1), f32(dt)
    tends = [t1] * (len(eests) + 1) if tends is None else [f32(x) for x in tends]
    dtmax = f32(t1 - t0)
    dtmin = fmax(_eps(t1), _eps(t0))
    t, qold, q11, dtpropose, it = t0, f32(1e-4), ONE, dt, 1
    dt, status = clamp_status(dt, dtmax, dtmin, t, tends[0], it, maxiters)
    rows = [(status, bits(dt))]
    for i, eest in enumerate(eests):
        if status != OK:
            break
        tend = tends[i]
        eest = f32(eest)
        accept = False
        if np.isnan(eest):
            status = DT_NAN
        else:
            if eest == 0:
                q = f32(ONE / qmax)
            else:
                q11 = powf(exact, eest, beta1)
                q = f32(q11 / powf(exact, qold, beta2))
                q = fmax(f32(ONE / qmax), fmin(f32(ONE / qmin), f32(q / gamma)))
            accept = bool(eest <= 1)
            if accept:
                qold = fmax(eest, f32(1e-4))
                ttmp = f32(t + dt)
                ref = fmax(f32(abs(t)), f32(abs(tend))) if snap else fmax(t, tend)
                t = tend if abs(f32(ttmp - tend)) < f32(f32(100) * _eps(ref)) else ttmp
                dtpropose = fmax(fmin(dtmax, f32(dt / q)), fmax(_eps(t), dtmin))
            if not t < t1:
                status = DONE
            else:
                dt = dtpropose if accept else f32(dt / fmin(f32(ONE / qmin), f32(q11 / gamma)))
                it += 1
                dt, status = clamp_status(dt, dtmax, dtmin, t, tends[i + 1], it, maxiters)
        rows.append((bits(q11), int(accept), bits(t), bits(dtpropose), bits(dt), status))
    return rows


NEXT1 = np.nextafter(f32(1), f32(2))
NEAR = f32(1) - f32(2.0 ** -20)   # a step of this length from the start of a unit span ends 8 ulp(1) short of its end
# name: (t0, t1, dt_init, maxiters, eests[, tends])
SCRIPTS = {
    # zero, exactly one, just above one (a reject), both growth clamps, three rejects in a row, NaN last
    "mixed": (0.0, 1.0, 0.01, 1000, [0.0, 1.0, NEXT1, 1e-30, 1e30, 2.0, 1.5, 0.5, 0.25, float("nan")]),
    "snap": (0.0, 1.0, NEAR, 1000, [0.5, 0.5]),
    "reversed": (-1.0, 0.0, NEAR, 1000, [0.5, 0.5, 0.5, 0.5, float("nan")]),
    "dtmin": (0.0, 1.0, 0.01, 1000, [1e30] * 14),
    "maxiters": (0.0, 1.0, 0.01, 3, [0.5] * 6),
    # tstops at 1/4 and 1/2: a first step that ends 8 ulp short of 1/4, a reject and an accept on the way to 1/2, a step
    # cut at 1/2, one towards the end of the span
    "tstops": (0.0, 1.0, f32(0.25) * NEAR, 1000, [0.5, 2.0, 1e-30, 1e-30, 1e-30], [0.25, 0.5, 0.5, 0.5, 1.0, 1.0]),
}


def run_script(driver, name, cset, exact, snap):
    t0, t1, dt, maxiters, eests = SCRIPTS[name][:5]
    tends = SCRIPTS[name][5] if len(SCRIPTS[name]) > 5 else None
    text = "%s %d %d %d %d %d %s %s %s %s\n" % ("C" if tends is None else "T", cset, exact, snap, maxiters, len(eests), hx(t0),
                                                 hx(t1), hx(dt), " ".join(hx(e) for e in eests + (tends or [])))
    out = driver(text)
    end = out.index("end")
    got = [tuple(int(w, 16) if len(w) == 8 else int(w) for w in ln.split()) for ln in out[:end]]
    want = restate(cset, exact, snap, maxiters, t0, t1, dt, eests, tends)
    assert len(got) == len(want), (name, got, want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w) and all(same(a, b) for a, b in zip(g, w)), (name, cset, exact, snap, i, g, w)
    return want


@pytest.mark.parametrize("cset,exact,snap", list(itertools.product((0, 1), (0, 1), (0, 1))))
def test_controller_recurrence(driver, cset, exact, snap):
    rows = {name: run_script(driver, name, cset, exact, snap) for name in SCRIPTS}
    gamma, qmin, qmax, beta1, beta2 = CONSTS[cset]
    # the scripts reach what they were written for
    m = rows["mixed"]
    assert m[-1][-1] == DT_NAN and len(m) == 1 + len(SCRIPTS["mixed"][4])
    acc = [r[1] for r in m[1:]]
    assert acc[:3] == [1, 1, 0] and acc[4:7] == [0, 0, 0]
    dts = [np.array([r[4] if len(r) == 6 else r[1]], np.uint32).view(f32)[0] for r in m]
    # (a tiny error estimate: q is held at 1/qmax, the cap of ten on a step's growth; a huge one: the shrink is held at 1/qmin)
    assert m[4][3] == bits(f32(dts[3] / f32(ONE / qmax))), "eest = 1e-30: q clamped at 1/qmax"   # (attempted at dts[3])
    assert m[5][0] == bits(powf(exact, f32(1e30), beta1)) and dts[5] == f32(dts[4] / f32(ONE / qmin)), "eest = 1e30: shrink capped at 1/qmin"
    s = rows["snap"]
    assert s[1][2] == bits(f32(1.0)) and s[1][5] == DONE and len(s) == 2, "t + dt within 100 eps of t1 lands on t1"
    assert rows["dtmin"][-1][-1] == DT_LESS_THAN_MIN
    assert rows["maxiters"][-1][-1] == MAXITERS and len(rows["maxiters"]) == 1 + 3
    ts = rows["tstops"]
    assert ts[1][2] == bits(f32(0.25)) and ts[1][5] == OK, "t + dt within 100 eps of the tstop lands on it, and the solve goes on"
    assert [r[1] for r in ts[1:]] == [1, 0, 1, 1, 1] and ts[4][2] == bits(f32(0.5)), "the step after the reject is cut at the second tstop"
    r = rows["reversed"]
    if snap:
        assert r[1][2] == bits(f32(0.0)) and r[1][5] == DONE
    else:   # eps at the signed maximum (0) is the smallest subnormal: no snap, the solve goes on
        assert r[1][2] == bits(f32(f32(-1.0) + NEAR)) and r[1][5] == OK and len(r) > 2


def next_stop(stops, t, s1):
    """the end time of an attempt that starts at t: the first tstop after t if it lies before s1, else s1; and how many
    of the (ascending) tstops lie at or before t"""
    later = [x for x in stops if x > t]
    return (later[0] if later and later[0] < s1 else s1), len(stops) - len(later)


def test_tstop_cursor(driver):
    s0, s1 = -1.0, 0.0
    # name: (tstops, the times attempts start at)
    cases = {
        # a stop at s0, two equal stops, a stop at s1 and one past it; t on a stop, between stops, past two stops at once
        "all": ([-1.0, -0.75, -0.75, -0.5, -0.25, 0.0, 0.5], [-1.0, -0.875, -0.75, -0.625, -0.125, -0.0625]),
        "empty": ([], [-1.0, -0.5]),
        "past_s1": ([0.5], [-1.0, -0.5]),
        "at_s1": ([0.0], [-1.0, -0.5]),
    }
    for name, (stops, ts) in cases.items():
        out = driver("S %d %s %s %s %d %s\n" % (len(stops), hx(s0), hx(s1), " ".join(hx(x) for x in stops), len(ts),
                                                " ".join(hx(t) for t in ts)))
        for t, ln in zip(ts, out):
            e, i = next_stop(stops, t, s1)
            assert ln.split() == [hx(e), str(i)], (name, t, ln, e, i)
    want = [next_stop(cases["all"][0], t, s1) for t in cases["all"][1]]
    assert want == [(-0.75, 1), (-0.75, 1), (-0.5, 3), (-0.5, 3), (0.0, 5), (0.0, 5)], want   # (a stop at s1 is not passed: s1 is returned as the end)


def restate_initdt(d0, d1, d2, dtmax, order):
    d0, d1, d2, dtmax, order = f32(d0), f32(d1), f32(d2), f32(dtmax), f32(order)
    dt0 = f32(1e-6) if (float(d0) < 1e-5 or float(d1) < 1e-5) else f32(f32(d0 / d1) / f32(100))
    dt0 = fmin(dt0, dtmax)
    maxd = fmax(d1, f32(d2 / dt0))
    if float(maxd) <= 1e-15:
        dt1 = fmax(f32(1e-6), f32(dt0 * f32(1e-3)))
    else:
        e = f32(f32(-f32(f32(2) + f32(math.log10(float(maxd))))) / order)
        dt1 = f32(math.pow(10.0, float(e)))
    hundred = f32(f32(100) * dt0)
    dt = fmin(fmin(hundred, dt1), dtmax)
    return dt0, dt, dict(small_d0=float(d0) < 1e-5, small_d1=float(d1) < 1e-5, flat=float(maxd) <= 1e-15,
                         dtmax_binds=dt == dtmax and dtmax < fmin(hundred, dt1), hundred_binds=dt == hundred and hundred < fmin(dt1, dtmax))


def test_dt0_and_initdt_tail(driver):
    grid = list(itertools.product((1e-6, 0.5, 3.0, 1234.5), (0.0, 1e-16, 1e-7, 0.02, 40.0), (0.0, 1e-20, 1e-3, 7.0),
                                  (1e-4, 1.0, 50.0), (5.0, 3.0, 1.5)))
    out = driver("".join("I %s %s %s %s %s\n" % tuple(hx(v) for v in g) for g in grid))
    seen = set()
    for g, ln in zip(grid, out):
        dt0, dt, why = restate_initdt(*g)
        got = [int(w, 16) for w in ln.split()]
        assert same(got[0], bits(dt0)) and same(got[1], bits(dt)), (g, got, bits(dt0), bits(dt))
        seen |= {k for k, v in why.items() if v}
    assert seen == {"small_d0", "small_d1", "flat", "dtmax_binds", "hundred_binds"}, seen
