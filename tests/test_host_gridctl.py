"""csrc/lrnde_stepctl.hpp on the host: the SDE loops' controller on the path's grid (sde_grid_begin: every
initialisation of a control block; sde_grid_update: the host loop's controller, the device loops' sde_ctl_update restated
with the writes left to the caller) against the controller lines of
tests/sde_adaptive_np.py (grid_begin, grid_update: the loop tests/test_host_sde_adaptive.py pins to the committed oracle), with
fastpow through the oracle library as that helper takes it.  The whole control block after every update, integers and float
bit patterns compared exactly (NaN equal to NaN)."""
import os, subprocess, textwrap
import numpy as np
import pytest

import sde_adaptive_np as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
RUNNING, MAXITERS, DT_LESS_THAN_MIN, DT_NAN, CAPACITY, DONE = 0, 1, 2, 3, 5, 100   # include/lrnde.h; DONE: the end of the grid
STATUS = {"running": RUNNING, "done": DONE, "DtNaN": DT_NAN, "DtLessThanMin": DT_LESS_THAN_MIN}

SRC = textwrap.dedent(r'''
    #include "lrnde_stepctl.hpp"
    #include <cstdio>
    #include <cstring>
    using namespace lrnde;
    static float rd() { unsigned u = 0; if (scanf("%x", &u) != 1) u = 0; float x; memcpy(&x, &u, 4); return x; }
    static unsigned bits(float x) { unsigned u; memcpy(&u, &x, 4); return u; }
    static void show(const SdeCtl& c, const SdeVerdict v) {
      printf("%d %d %d %d %d %d %d %d %08x %08x %08x %d %d %d\n", c.status, c.i, c.m, c.cur, c.naccept, c.nreject, c.iters, c.nf, bits(c.qold),
             bits(c.eest_last), bits(c.dtc), v.accepted, v.rec, v.trace);
    }
    int main() {
      // dt0 h nfine maxiters gamma qmin qmax beta1 beta2 rec_cap nfa n eest[n]: the fresh block, then the block after every update
      for (;;) {
        const float dt0 = rd(), h = rd();
        int nfine, maxiters, rec_cap, nfa, n;
        if (scanf("%d %d", &nfine, &maxiters) != 2) return 0;
        SdeGrid g;
        g.pi.gamma = rd(); g.pi.qmin = rd(); g.pi.qmax = rd(); g.pi.beta1 = rd(); g.pi.beta2 = rd();
        g.h = h; g.nfine = nfine; g.maxiters = maxiters;
        if (scanf("%d %d %d", &rec_cap, &nfa, &n) != 3) return 2;
        SdeCtl c = sde_grid_begin(dt0, h, nfine);
        show(c, SdeVerdict{0, -1, -1});
        for (int j = 0; j < n; ++j) {
          const float eest = rd();
          if (c.status != STEP_OK) continue;
          const float dt = (float)c.m * h;
          show(c, sde_grid_update(c, eest, dt, fastpow(c.qold, g.pi.beta2), nfa, g, rec_cap));
        }
        printf("end\n");
      }
    }
''')


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("gridctl")
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
    """equal integers / bits, or both NaN"""
    if a == b or a < 0 or b < 0:
        return a == b
    fa, fb = np.array([a], np.uint32).view(f32)[0], np.array([b], np.uint32).view(f32)[0]
    return a == b or (np.isnan(fa) and np.isnan(fb))


DEFAULT = (0.9, 0.2, 1.125, 7.0 / 50.0, 2.0 / 25.0)   # the layer's options: gamma, qmin, qmax, beta1, beta2
LOOSE = (2.0, 0.2, 1.125, 7.0 / 50.0, 2.0 / 25.0)     # gamma = 2: a rejected step's proposal is no shorter than the step


def expected(fp, dt0, h, nfine, maxiters, consts, rec_cap, nfa, eests):
    """rows (status, i, m, cur, naccept, nreject, iters, nf, qold, eest_last, dtc, accepted, rec, trace) of the fresh block and of
    every update while the solve runs.  The controller is sde_adaptive_np's; around it, what the control block keeps beside it:
    nf and eest_last of every attempt (a NaN one too), the buffer flip, maxiters as a status, and the record slot.
    rec_cap >= 0: an accepted step that finds the record full is the device loops' CAPACITY — written from the
    device form (sde_ctl_update, lrnde_sde_frame.hpp): the step is still counted (naccept, i, the buffer flip, m = the proposal's floor, NOT clamped to the rest of
    the grid), iters is not, and neither DONE nor MAXITERS replaces the status."""
    consts = tuple(f32(v) for v in consts)
    h = f32(h)
    c = S.grid_begin(dt0, h, nfine)
    rows = [(RUNNING, c["i"], c["m"], 0, 0, 0, c["iters"], 0, bits(c["qold"]), bits(f32(0)), bits(c["dtc"]), 0, -1, -1)]
    status, nf = RUNNING, 0
    for ee in eests:
        if status != RUNNING:
            break
        ee = f32(ee)
        before = dict(c)
        dt = f32(f32(c["m"]) * h)
        S.grid_update(c, ee, dt, h, nfine, consts, fp)
        nf += nfa
        status = STATUS[c["status"]]
        acc = int(bool(ee <= 1))
        rec, trace = -1, (-1 if np.isnan(ee) else before["naccept"] + before["nreject"])
        if acc and rec_cap >= 0:
            if before["naccept"] < rec_cap:
                rec = before["naccept"]
            else:
                status = CAPACITY
                c["m"], c["iters"] = max(int(f32(c["dtc"] / h)), 1), before["iters"]
        if status == RUNNING and c["iters"] > maxiters:
            status = MAXITERS
        rows.append((status, c["i"], c["m"], c["naccept"] & 1, c["naccept"], c["nreject"], c["iters"], nf, bits(c["qold"]), bits(ee),
                     bits(c["dtc"]), acc, rec, trace))
    return rows


H64 = 1.0 / 64
NAN = float("nan")
# name: (dt0, h, nfine, maxiters, constants, rec_cap, nfa, eests)
SCRIPTS = {
    # from one interval: the proposal grows by 1.125 per step in dtc, the step stays at m = 1 until dtc passes 2 h
    "growth": (H64, H64, 64, 1000, DEFAULT, -1, 3, [1e-3] * 12),
    # zero, exactly one, a reject whose proposal is shorter (mnew < m), accepts, NaN last
    "mixed": (0.25, H64, 64, 1000, DEFAULT, -1, 1, [0.0, 1.0, 30.0, 0.5, 1.0001, 0.25, NAN]),
    # gamma = 2: the rejected step's proposal is not shorter than the step: m - 1
    "fallback": (0.125, H64, 64, 1000, LOOSE, -1, 4, [1.0, 1.0001, 1.0001, 0.5]),
    "dtmin": (2 * H64, H64, 64, 1000, DEFAULT, -1, 3, [1e-3, 1e30, 1e30, 1e30]),
    "maxiters": (0.125, H64, 64, 4, DEFAULT, -1, 3, [0.5] * 6),
    # the last step is cut to what is left of the grid, and ends the solve
    "clamped_end": (0.4, H64, 64, 1000, DEFAULT, 64, 3, [1e-3] * 4),
    "dt0_past_the_span": (3.0, H64, 64, 1000, DEFAULT, -1, 3, [2.0, 0.5, 0.5, 0.5]),
    "capacity": (0.125, H64, 64, 1000, DEFAULT, 2, 3, [0.5, 2.0, 0.5, 0.5, 0.5]),
    # ... on the step that reaches the end of the grid: CAPACITY stays, DONE does not replace it
    "capacity_at_the_end": (0.5, H64, 64, 1000, DEFAULT, 1, 3, [1e-3] * 3),
}


def run_script(driver, fp, name):
    dt0, h, nfine, maxiters, consts, rec_cap, nfa, eests = SCRIPTS[name]
    out = driver("%s %s %d %d %s %d %d %d %s\n" % (hx(dt0), hx(h), nfine, maxiters, " ".join(hx(v) for v in consts), rec_cap, nfa, len(eests),
                                                  " ".join(hx(e) for e in eests)))
    got = [tuple(int(w, 16) if len(w) == 8 else int(w) for w in ln.split()) for ln in out[:out.index("end")]]
    want = expected(fp, dt0, h, nfine, maxiters, consts, rec_cap, nfa, eests)
    assert len(got) == len(want), (name, got, want)
    for j, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w) and all(same(a, b) for a, b in zip(g, w)), (name, j, g, w)
    return want


ST, I, M, CUR, NACC, NREJ, ITERS, NF, QOLD, EEST, DTC, ACC, REC, TRACE = range(14)


def test_grid_controller(driver, oracle):
    fp = lambda a, b: f32(oracle.lib().lro_fastpow(float(a), float(b)))
    rows = {name: run_script(driver, fp, name) for name in SCRIPTS}
    fl = lambda b: np.array([b], np.uint32).view(f32)[0]
    # the scripts reach what they were written for
    g = rows["growth"]
    ms = [r[M] for r in g]
    assert ms[0] == 1 and ms[:6] == [1] * 6 and ms[-1] >= 2 and ms == sorted(ms), ms
    k = ms.index(2)   # the first update that leaves m = 2: its proposal has just passed 2 h, the one before had not
    assert fl(g[k][DTC]) >= f32(2 * H64) > fl(g[k - 1][DTC]) > f32(H64) and all(fl(b[DTC]) > fl(a[DTC]) for a, b in zip(g[:k], g[1:k + 1]))
    m = rows["mixed"]
    assert [r[ACC] for r in m[1:]] == [1, 1, 0, 1, 0, 1, 0] and m[-1][ST] == DT_NAN and m[-1][TRACE] == -1 and m[-1][NF] == 7
    assert m[1][DTC] == bits(f32(f32(0.25) / f32(f32(1) / f32(1.125)))), "eest == 0: q = 1 / qmax"
    assert m[3][M] < m[2][M] - 1 and m[3][I] == m[2][I] and m[3][CUR] == m[2][CUR], "a reject with mnew < m"
    assert [r[TRACE] for r in m[1:-1]] == list(range(6)) and all(r[REC] == -1 for r in m)
    f = rows["fallback"]
    assert [r[ACC] for r in f[1:]] == [1, 0, 0, 1] and f[2][M] == f[1][M] - 1 and f[3][M] == f[2][M] - 1, "a reject that falls back to m - 1"
    d = rows["dtmin"]
    assert d[-1][ST] == DT_LESS_THAN_MIN and d[-2][M] == 1 and d[-1][NREJ] == 2 and d[-1][ITERS] == d[-2][ITERS]
    x = rows["maxiters"]
    assert x[-1][ST] == MAXITERS and x[-1][ITERS] == 5 and len(x) == 1 + 4
    e = rows["clamped_end"]
    assert e[-1][ST] == DONE and e[-1][I] == 64 and e[-2][M] == 64 - e[-2][I] and fl(e[-2][DTC]) > f32(e[-2][M] * H64)
    assert [r[REC] for r in e[1:]] == list(range(len(e) - 1)) and e[-1][ITERS] == e[-2][ITERS]
    p = rows["dt0_past_the_span"]
    assert p[0][M] == 64 and p[0][DTC] == bits(f32(3.0)) and p[0][ITERS] == 1
    c = rows["capacity"]
    assert [r[ST] for r in c] == [0, 0, 0, 0, CAPACITY] and [r[REC] for r in c[1:]] == [0, -1, 1, -1]
    assert c[-1][NACC] == 3 and c[-1][I] == c[-2][I] + c[-2][M] and c[-1][CUR] == 1 and c[-1][ITERS] == c[-2][ITERS] and c[-1][ACC] == 1
    ce = rows["capacity_at_the_end"]
    assert ce[-1][ST] == CAPACITY and ce[-1][I] == 64 and ce[-1][NACC] == 2 and ce[-1][M] > 0
