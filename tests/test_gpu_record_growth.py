"""The Dense-chain handles (small: csrc/lrnde_chain.hpp, wide: csrc/lrnde_wide_chain.hpp) past the first dense record, and
after failed solves.

A recorded forward keeps one record entry per accepted step.  The record starts at 64 entries; a solve that needs more is
stopped by the step kernel's footer with LRNDE_CAPACITY, node_forward_record_impl doubles the record and runs the whole
forward again.  Everything here records more than 64 (or 128) accepted steps, so it runs the LRNDE_CAPACITY branches of the
Tsit5 footer, of k_adams_chain and of the host Adams loop, the retry, adj_lookup over more than 64 knots, and the discrete
sweeps over more than 64 recorded steps — on the small chain, the wide chain and both Adams loops.  The third group stops
solves on purpose (floating-point overflow to a defined return code, MaxIters) and holds the handle afterwards to a fresh
twin, bit for bit.

Cases, selection conditions and the origin of every bar: tests/record_growth_cases.py; the conditions are re-derived on the
CPU by tests/test_host_record_growth.py.  Every test prints the naccept it reached and asserts it is above the line it is
about."""
import numpy as np
import pytest
import torch

import chain_adams_cases as K
import chain_discrete_np as CD
import record_growth_cases as G
import test_gpu_chain as TC
import wide_chain_adjoint_cases as WA
import wide_chain_discrete_cases as WD
from test_gpu_chain_adams import STAT_KEYS, cu, rhs_field, solve_equal

pytestmark = pytest.mark.gpu

f32 = np.float32
MODES = ("none", "unbiased", "biased")
BIG = 10000     # maxiters of every solve that is meant to finish


# ---- helpers ----------------------------------------------------------------------------------------------------------
def fresh(P, kind, name, loop="auto"):
    """(handle, model, p, x, tol, span) of a case on a new handle: kind "small" (test_gpu_chain.mk) or "wide"
    (wide_chain_adjoint_cases.handle_for); the case's solver is set on the handle.  loop: the wide handle's adjoint loop
    ("auto": the host loop, "device", "discrete"); "discrete" gives the small handle its discrete sweep too"""
    model, p, x, tol, span, solver = G.case(P, name)
    c = G.CASES[name]
    if kind == "small":
        h, p2, x2 = TC.mk(P, model, c["B"], scale=c["scale"])
        assert np.array_equal(p, p2) and np.array_equal(x, x2)
        if solver != "tsit5":
            h.set_solver(solver)
        if loop == "discrete":
            h.set_sensealg("discrete")
    else:
        assert solver == "tsit5"
        h = WA.handle_for(P, model, p, loop=loop)
    return h, model, p, x, tol, span


def draw(mode, span):
    """t1_or_rand of the layer: t1 = 0.43 x span in :unbiased, the index draw 0.43 in :biased"""
    return float(f32(span[0] + G.T1_FRACTION * (span[1] - span[0]))) if mode == "unbiased" else G.T1_FRACTION


def same(a, b, tag=""):
    """two result dicts of the handle's calls, bit for bit: tensors, the saved times, floats, counters, the stats dict"""
    assert set(a) == set(b), (tag, set(a) ^ set(b))
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert torch.equal(a[k], b[k]), (tag, k)
        elif isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k]), (tag, k, a[k], b[k])
        elif isinstance(a[k], (float, np.floating)):
            assert np.float32(a[k]).tobytes() == np.float32(b[k]).tobytes(), (tag, k, a[k], b[k])
        else:
            assert a[k] == b[k], (tag, k, a[k], b[k])


def above(stats, name, tag):
    n, line = stats["naccept"], G.CASES[name]["line"]
    print(f"{tag}: naccept {n} nreject {stats['nreject']} (line {line})")
    assert n > line, (tag, n, line)
    if G.CASES[name]["one_doubling"]:
        assert n <= G.SECOND_RECORD
    return n


@pytest.fixture
def option(gpu_pkg):
    """option(name, fn): fn() with the process-wide switch `name` on, switched off again afterwards"""
    used = set()

    def run(name, fn):
        used.add(name)
        try:
            gpu_pkg.set_option(name, 1)
            return fn()
        finally:
            gpu_pkg.set_option(name, 0)
    yield run
    for name in used:
        gpu_pkg.set_option(name, 0)


def with_loop(option, host, fn):
    """fn() on the device Adams loop, or under LRNDE_ADAMS_HOST=1"""
    return option("LRNDE_ADAMS_HOST", fn) if host else fn()


HANDLE_CASES = [("small", n) for n in G.TSIT5_SMALL] + [("wide", n) for n in G.TSIT5_WIDE]
ADAMS_CASES = [(n, host) for n in G.ADAMS for host in (0, 1)]


# ======================================================================================================================
# 1. the recorded forward past the record
# ======================================================================================================================
def forward_equals_plain(P, kind, name):
    """the recorded forward (end form and series form) on a fresh handle against the plain forward on the same handle, in
    all three modes"""
    for mode in MODES:
        h, _, _, x, tol, span = fresh(P, kind, name)
        xd, sv = cu(x), G.series_times(span)
        args = (xd, span[0], span[1], tol, tol)
        # (:biased draws t1 among the saved times, the start included as the layer's default has it, in every form)
        kw = dict(mode=mode, t1_or_rand=draw(mode, span), maxiters=BIG, save_start=mode == "biased")
        rec = h.node_forward_record(*args, **kw)
        plain = h.node_forward(*args, **kw)
        above(rec["stats"], name, f"{kind} {name} {mode} end form")
        same(rec, plain, (name, mode, "end form"))   # u_end, reg_val, nfe, t1, every key of stats: one solve's, not the retries' sum
        assert (rec["reg_val"] > 0) == (mode != "none")
        # the series form: the layer's saveat (none, unbiased) or every step (biased: more than 64 entries)
        h = fresh(P, kind, name)[0]
        if mode == "biased":
            rts = h.node_forward_record_ts(*args, [], **kw)
            sol = h.solve(*args, saveat=(), save_everystep=True, save_start=True, maxiters=BIG)
            keep = list(range(len(sol["t"])))
            assert len(rts["t"]) == rts["stats"]["naccept"] + 1 > G.FIRST_RECORD
        else:
            t1 = f32(kw["t1_or_rand"])
            rts = h.node_forward_record_ts(*args, sv, **kw)
            sol = h.solve(*args, saveat=sorted(sv + [float(t1)]) if mode == "unbiased" else sv, maxiters=BIG)
            keep = [i for i, t in enumerate(sol["t"]) if not (mode == "unbiased" and t == t1)]
            assert [float(t) for t in rts["t"]] == sv
        above(rts["stats"], name, f"{kind} {name} {mode} series form")
        assert np.array_equal(rts["t"], sol["t"][keep]), (mode, rts["t"], sol["t"])
        assert torch.equal(rts["u"], sol["u"][keep]), mode
        assert rts["stats"] == sol["stats"], (mode, rts["stats"], sol["stats"])
        assert rts["nfe"] == sol["stats"]["nf"] + (9 if mode != "none" else 0) == rec["nfe"]
        assert torch.equal(rts["u_end"], rec["u_end"]) and rts["reg_val"] == rec["reg_val"] and rts["t1"] == rec["t1"]


@pytest.mark.parametrize("kind,name", HANDLE_CASES)
def test_recorded_forward_equals_the_plain_forward(gpu_pkg, kind, name):
    forward_equals_plain(gpu_pkg, kind, name)


@pytest.mark.parametrize("name,host", ADAMS_CASES)
def test_adams_recorded_forward_equals_the_plain_forward(gpu_pkg, option, name, host):
    with_loop(option, host, lambda: forward_equals_plain(gpu_pkg, "small", name))


def pairs(h, x, span, tol):
    """(end form, series form): mode -> (recorded forward, its backward at w_reg = 2.5) on handle h"""
    xd, sv = cu(x), G.series_times(span)
    du = cu(G.cotangents(1, x, seed=5)[0])
    gs = cu(G.cotangents(len(sv), x, seed=6))

    def end_pair(mode):
        fw = h.node_forward_record(xd, span[0], span[1], tol, tol, mode=mode, t1_or_rand=draw(mode, span), maxiters=BIG)
        return fw, h.node_backward_recorded(du, w_reg=G.W_REG)

    def series_pair(mode):
        fw = h.node_forward_record_ts(xd, span[0], span[1], tol, tol, sv, mode=mode, t1_or_rand=draw(mode, span), maxiters=BIG)
        return fw, h.node_backward_recorded_ts(gs, w_reg=G.W_REG)
    return dict(end=end_pair, series=series_pair)


def retry_leaves_nothing(P, kind, name, form, mode, loop="auto"):
    """the first recorded forward on a fresh handle (one or two retries) against a second, identical one (no retry: the
    capacity stays grown) and against a second fresh handle's first, with the backwards from each"""
    h, _, _, x, tol, span = fresh(P, kind, name, loop=loop)
    pair = pairs(h, x, span, tol)[form]
    (f1, b1), (f2, b2) = pair(mode), pair(mode)
    above(f1["stats"], name, f"{kind} {name} {form} {mode} {loop}")
    f3, b3 = pairs(fresh(P, kind, name, loop=loop)[0], x, span, tol)[form](mode)
    for tag, f, b in (("second call", f2, b2), ("fresh twin", f3, b3)):
        same(f1, f, tag)
        assert torch.equal(b1["dx"], b["dx"]) and torch.equal(b1["dp"], b["dp"]) and b1["stats_bwd"] == b["stats_bwd"], tag
    assert bool(torch.isfinite(b1["dp"]).all()) and f1["reg_val"] > 0
    return h


# The backward of the hygiene tests: the continuous adjoint (the handle's default routing), but for phys_196, whose reversed
# solve at tolerance 1e-7 is rounding all the way (more than 10000 steps on the MI355X, 4852 in the float32 restatement on
# the CPU): there, and once more on phys_74, the discrete sweep.  With the discrete adjoint the forward keeps its stage
# record through the step kernel's dense_direct path, whose LRNDE_CAPACITY branch is the one at c.naccept >= a.dense_cap.
HYGIENE_CASES = [(k, n, "auto") for k, n in HANDLE_CASES if n != "phys_196"] + \
    [(k, n, "discrete") for k in ("small", "wide") for n in ("phys_74", "phys_196")]


@pytest.mark.parametrize("form,mode", [("end", "unbiased"), ("series", "unbiased"), ("end", "biased")])
@pytest.mark.parametrize("kind,name,loop", HYGIENE_CASES)
def test_retry_leaves_nothing_behind(gpu_pkg, kind, name, loop, form, mode):
    """what a stopped attempt could leave: its regulariser sweep in R.gr, a save index, a series plan; w_reg = 2.5 brings the
    regulariser's gradient into dp"""
    h = retry_leaves_nothing(gpu_pkg, kind, name, form, mode, loop)
    assert h.last_adjoint_info()["kind"] == {("small", "auto"): 2, ("wide", "auto"): 0, ("small", "discrete"): 4, ("wide", "discrete"): 5}[(kind, loop)]


@pytest.mark.parametrize("form", ["end", "series"])
@pytest.mark.parametrize("name,host", ADAMS_CASES)
def test_adams_retry_leaves_nothing_behind(gpu_pkg, option, name, host, form):
    """as above, with the Adams history hh of the stopped attempt"""
    with_loop(option, host, lambda: retry_leaves_nothing(gpu_pkg, "small", name, form, "unbiased"))


@pytest.mark.parametrize("kind,name,loop", [("small", "phys_74", "auto"), ("small", "phys_196", "discrete"), ("wide", "phys_74", "auto"),
                                            ("wide", "phys_196", "discrete"), ("wide", "odd130_87", "auto"),
                                            ("small", "phys_vcab3_1e-4", "auto"), ("small", "phys_vcabm3_1e-4", "auto")])
def test_another_batch_and_back(gpu_pkg, kind, name, loop):
    """B' = 5 between two identical calls: dense_n changes, the record is reallocated at the grown capacity, and again on
    the way back"""
    P = gpu_pkg
    h, _, _, x, tol, span = fresh(P, kind, name, loop=loop)
    xo = G.other_batch(P, name)
    end_pair = pairs(h, x, span, tol)["end"]
    f1, b1 = end_pair("unbiased")
    above(f1["stats"], name, f"{kind} {name}")
    fo, bo = pairs(h, xo, span, tol)["end"]("unbiased")
    ft, bt = pairs(fresh(P, kind, name, loop=loop)[0], xo, span, tol)["end"]("unbiased")
    same(fo, ft, "the other batch against a fresh handle")
    assert torch.equal(bo["dx"], bt["dx"]) and torch.equal(bo["dp"], bt["dp"])
    f2, b2 = end_pair("unbiased")
    same(f1, f2, "back")
    assert torch.equal(b1["dx"], b2["dx"]) and torch.equal(b1["dp"], b2["dp"])


@pytest.mark.parametrize("kind,name", HANDLE_CASES)
def test_solution_against_float64_restatement(gpu_pkg, kind, name):
    """sol.u[end] of the recorded forward against np_restatement.solve over Chain64, at
    max(1e-5, 0.5 tol, 4 x the distance of the same solve over Chain32).  Twin distances on the CPU -> bar: phys_74 6.2e-5 ->
    2.5e-4, phys_119 2.8e-4 -> 1.1e-3, phys_196 3.5e-3 -> 1.4e-2, small3_176 1.2e-6 -> 1e-5, odd130_87 7.5e-6 -> 3.0e-5.
    Measured on an MI355X: record_growth_cases.SOLUTION_GPU."""
    P = gpu_pkg
    h, _, _, x, tol, span = fresh(P, kind, name)
    fw = h.node_forward_record(cu(x), span[0], span[1], tol, tol, mode="none", maxiters=BIG)
    above(fw["stats"], name, f"{kind} {name}")
    bar, d = G.solution_bar(name)
    e = TC.err(fw["u_end"].cpu().numpy(), G.solution_twins(name)[0]["u"])
    print(f"{kind} {name}: gpu from the float64 restatement {e:.2e}; float32 twin {d:.2e}; bar {bar:.2e}")
    assert e <= bar, (e, bar)


@pytest.mark.parametrize("name,host", ADAMS_CASES)
def test_adams_recorded_solve_equals_the_oracle(oracle, gpu_pkg, option, name, host):
    """the plain solve with its trace and the recorded forward's solve, both == oracle.solve(..., solver=...) around
    Handle.rhs (tests/test_gpu_chain_adams.py's convention); the device-loop record and the host-loop record give the same
    dx / dp"""
    P = gpu_pkg
    h, _, _, x, tol, span = fresh(P, "small", name)
    solver = G.CASES[name]["solver"]
    sv = G.series_times(span)
    xd = cu(x)
    ref = oracle.solve(rhs_field(oracle, h, x.shape[1]), x, span[0], span[1], tol, tol, saveat=sv, solver=solver, maxiters=BIG)
    assert ref["retcode"] == 0
    got = with_loop(option, host, lambda: h.solve(xd, span[0], span[1], tol, tol, saveat=sv, trace=True, maxiters=BIG))
    above(got["stats"], name, f"{name} host={host} plain solve")
    solve_equal(got, ref)
    gs = cu(G.cotangents(len(sv), x, seed=6))

    def pair():
        hh = fresh(P, "small", name)[0]
        fw = hh.node_forward_record_ts(xd, span[0], span[1], tol, tol, sv, mode="none", maxiters=BIG)
        return fw, hh.node_backward_recorded_ts(gs)
    fw, bw = with_loop(option, host, pair)
    for k in STAT_KEYS:
        assert fw["stats"][k] == ref["stats"][k], (k, fw["stats"], ref["stats"])
    assert np.array_equal(fw["t"], ref["t"]) and np.array_equal(fw["u"].cpu().numpy(), ref["u"])
    fo, bo = with_loop(option, 1 - host, pair)
    same(fw, fo, "the other loop's forward")
    assert torch.equal(bw["dx"], bo["dx"]) and torch.equal(bw["dp"], bo["dp"])
    assert bool(torch.isfinite(bw["dp"]).all()) and float(bw["dp"].abs().max()) > 0


# ======================================================================================================================
# 2. pullbacks from a record of more than 64 steps
# ======================================================================================================================
def run_ts(h, x, span, times, cots, tol, mode="none", t1_or_rand=0.43, w_reg=0.0, save_start=False):
    """wide_chain_adjoint_cases.run_ts with a span: recorded forward + pullback, with the trace of the reversed solve"""
    xd = cu(x)
    fw = h.node_forward_record_ts(xd, span[0], span[1], tol, tol, times, mode=mode, t1_or_rand=t1_or_rand, maxiters=BIG,
                                  save_start=save_start)
    h.set_adjoint_trace(16384)
    try:
        bw = h.node_backward_recorded_ts(cu(cots), w_reg=w_reg)
        rows = h.adjoint_trace()
    finally:
        h.set_adjoint_trace(0)
    sb = bw["stats_bwd"]
    return dict(dx=bw["dx"].cpu().numpy(), dp=bw["dp"].cpu().numpy(), counts=(sb["naccept"], sb["nreject"], sb["nf"]), rows=rows,
                ai=h.last_adjoint_info(), stats=sb, fwd=fw["stats"], t=fw["t"])


def both_loops(P, option, kind, name, mode):
    """[(tag, result)] of the continuous pullback on the device-controlled loop and on the host loop of the same kind of
    handle: LRNDE_ADJ_HOST=1 for the small chain, set_adjoint_loop("auto") for the wide one"""
    model, p, x, tol, span, times, cots = G.pullback_inputs(P, name)
    if mode == "biased":       # every step is saved: every impulse lies on a knot dense_t[lo], most of them with lo >= 64
        hp = fresh(P, kind, name, loop="device")[0]
        n = hp.node_forward_record_ts(cu(x), span[0], span[1], tol, tol, [], mode="biased", t1_or_rand=0.43, maxiters=BIG,
                                      save_start=False)["u"].shape[0]
        times, cots = [], G.cotangents(int(n), x)
    kw = dict(mode=mode, t1_or_rand=draw(mode, span))
    hd = fresh(P, kind, name, loop="device")[0]
    dev = run_ts(hd, x, span, times, cots, tol, **kw)
    if kind == "small":
        host = option("LRNDE_ADJ_HOST", lambda: run_ts(hd, x, span, times, cots, tol, **kw))
    else:
        host = run_ts(fresh(P, kind, name, loop="auto")[0], x, span, times, cots, tol, **kw)
    assert dev["ai"]["kind"] == (2 if kind == "small" else 3) and dev["ai"]["host_waits"] == 0, dev["ai"]
    assert host["ai"]["kind"] == 0, host["ai"]
    return dev, host


@pytest.mark.parametrize("kind,name,mode", [("small", "phys_119", "none"), ("small", "phys_119", "biased"), ("small", "small3_176", "none"),
                                            ("wide", "phys_119", "none"), ("wide", "odd130_87", "none"), ("wide", "odd130_87", "biased")])
def test_continuous_pullback_device_loop_equals_host_loop(gpu_pkg, option, kind, name, mode):
    """device loop == host loop, bit for bit, with more than 64 (small3_176: 128) knots in the record: the series times
    [0.1, 0.5, 0.93, 1.0] x span, and every step's end in :biased (each impulse lookup lands on a knot dense_t[lo])"""
    dev, host = both_loops(gpu_pkg, option, kind, name, mode)
    above(dev["fwd"], name, f"{kind} {name} {mode}")
    first = next((i for i, (a, b) in enumerate(zip(dev["rows"], host["rows"])) if a != b), None)
    print(f"{kind} {name} {mode}: {len(dev['t'])} saved times; reversed solve {dev['counts']} / {host['counts']}; launches "
          f"{dev['ai']['launches']} / {host['ai']['launches']}; rel dx {TC.rel(dev['dx'], host['dx']):.2e} dp {TC.rel(dev['dp'], host['dp']):.2e}"
          + ("" if first is None else f"; first differing row {first}: {dev['rows'][first]} / {host['rows'][first]}"))
    if mode == "biased":
        assert len(dev["t"]) == dev["fwd"]["naccept"] > G.FIRST_RECORD
    assert dev["fwd"] == host["fwd"]
    assert dev["counts"] == host["counts"] and dev["rows"] == host["rows"]
    assert np.array_equal(dev["dx"], host["dx"]) and np.array_equal(dev["dp"], host["dp"])
    assert np.isfinite(dev["dp"]).all() and np.abs(dev["dp"]).max() > 0


@pytest.mark.parametrize("kind,name", [("small", "phys_119"), ("small", "small3_176"), ("wide", "phys_119"), ("wide", "odd130_87"),
                                       ("wide", "small3_176")])
def test_continuous_pullback_against_float64_autograd(gpu_pkg, kind, name):
    """Against float64 torch autograd through RK4 (record_growth_cases.reference; its step count is held on the CPU) at
    max(3e-4, 4 x the distance of chain_adjoint_np.pullback in float32 from the same in float64).  On the CPU: phys_119 twins
    1.6e-2 apart in dx and in dp -> bars 6.4e-2 (the float64 restatement itself is 5.8e-4 from the reference: 3e-4 does not
    hold for a correct implementation at these inputs); odd130_87 5.3e-5 / 5.5e-5 and small3_176 2.7e-5 / 1.8e-5 -> 3e-4, the
    project's bar.  Measured on an MI355X: record_growth_cases.PULLBACK_GPU."""
    P = gpu_pkg
    model, p, x, tol, span, times, cots = G.pullback_inputs(P, name)
    got = run_ts(fresh(P, kind, name, loop="device")[0], x, span, times, cots, tol)
    above(got["fwd"], name, f"{kind} {name}")
    assert got["ai"]["kind"] == (2 if kind == "small" else 3)
    ref = dict(zip(("dx", "dp"), G.reference(name)))
    bars = G.pullback_bars(name)
    for k in ("dx", "dp"):
        e = TC.rel(got[k], ref[k])
        print(f"{kind} {name} {k}: rel to float64 autograd {e:.2e}; float32 restatement from float64 {bars[k][1]:.2e}; bar {bars[k][0]:.2e}")
    for k in ("dx", "dp"):
        assert TC.rel(got[k], ref[k]) <= bars[k][0], (k, TC.rel(got[k], ref[k]), bars[k])


_YARD = {}


def frozen_yardstick(name, model, p, x, grid, span, times, cots):
    k = (name, tuple(grid))
    if k not in _YARD:
        _YARD[k] = (CD.frozen_grads(model, p, x, grid, span[0], span[1], times, cots)[:2],
                    CD.frozen_grads(model, p, x, grid, span[0], span[1], times, cots, dtype=torch.float32)[:2])
    return _YARD[k]


@pytest.mark.parametrize("kind,name", [("small", "phys_74"), ("small", "phys_196"), ("small", "small3_176"), ("wide", "phys_74"),
                                       ("wide", "phys_196")])
def test_discrete_pullback_over_a_long_record(gpu_pkg, kind, name):
    """The discrete sweeps over more than 64 / 128 recorded steps (phys_74: with rejected attempts in the forward) against
    float64 autograd on the GPU forward's own grid, at the bars of tests/test_gpu_chain_discrete.py and
    tests/test_gpu_wide_chain_discrete.py: max(1e-5, 4 x the float32 twin).  record_growth_cases's docstring says what that
    bar is worth per case; the step counts of stats_bwd and the second call's bits hold for every one."""
    P = gpu_pkg
    model, p, x, tol, span, _ = G.case(P, name)
    times = G.series_times(span, G.DISCRETE_FRACTIONS)
    cots = G.cotangents(len(times), x, seed=12)
    if kind == "small":
        node = WD.make_node(P, model, tol, times, loop="auto", field="dense_chain", sensealg="TrackerAdjoint", tspan=span)
    else:
        node = WD.make_node(P, model, tol, times, tspan=span)
    got, again = WD.run(node, x, p, cots), WD.run(node, x, p, cots)
    h = node._bind(WD.dev(p), WD.dev(x))
    r = h.solve(WD.dev(x), span[0], span[1], tol, tol, saveat=[span[1]], save_everystep=False, maxiters=BIG, trace=True)
    grid = CD.grid_of_trace(r["trace"])
    N = len(grid)
    sf, sb = got["info"]["stats_fwd"], got["info"]["stats_bwd"]
    above(sf, name, f"{kind} {name}")
    assert (sf["naccept"], sf["nreject"]) == (r["stats"]["naccept"], r["stats"]["nreject"]) and sf["naccept"] == N
    if name == "phys_74":
        assert sf["nreject"] >= 1
    assert got["ai"]["kind"] == (4 if kind == "small" else 5) and got["ai"]["host_waits"] == 0, got["ai"]
    assert got["info"]["adjoint_loop"] == ("chain_discrete" if kind == "small" else "wide_discrete")
    assert (sb["naccept"], sb["nreject"], sb["iters"], sb["nf"], sb["retcode"]) == (N, 0, N, 6 * N + 1, 0), sb
    assert np.array_equal(got["dx"], again["dx"]) and np.array_equal(got["dp"], again["dp"])
    y64, y32 = frozen_yardstick(name, model, p, x, grid, span, times, cots)
    for k, key in enumerate(("dx", "dp")):
        e, b = TC.rel(got[key], y64[k]), CD.bound(y32[k], y64[k])
        print(f"{kind} {name}: {N} steps, {key} rel {e:.2e} bound {b:.2e}")
        assert e <= b, (key, e, b)


@pytest.mark.parametrize("name,shared", G.ADAMS_PULLBACK)
def test_adams_series_pullback_over_a_long_hermite_record(gpu_pkg, name, shared):
    """The series pullback over a Hermite record of more than 128 steps against float64 autograd, by the rule of
    test_gpu_chain_adams.test_pullback_against_float64_autograd: 3e-4, or twice the Tsit5 pullback's error measured here at
    the same inputs and tolerance.  phys_vcab3 at 1e-4 (149 steps): measured on an MI355X VCAB3 0.96 / 0.89 of the norm of
    dx / dp, Tsit5 0.96 / 0.88 — at that tolerance the chain at weights x3 has lost its gradient with either solver, and the
    rule holds nothing.  small3 at 1e-7 (1340 steps, the record grown five times) is held to the rule where it means
    something; record_growth_cases.ADAMS_PULLBACK says where its tolerance comes from."""
    P = gpu_pkg
    model, p, x, tol, span, _ = G.case(P, name)
    _, _, xs, _, _, times, cots = G.pullback_inputs(P, shared)
    assert np.array_equal(x, xs)
    ref = dict(zip(("dx", "dp"), G.reference(shared)))
    solver = G.CASES[name]["solver"]
    errs = {}
    for s in ("tsit5", solver):
        h = TC.mk(P, model, x.shape[0], scale=G.CASES[name]["scale"])[0]
        h.set_solver(s)
        got = run_ts(h, x, span, times, cots, tol)
        errs[s] = (TC.rel(got["dx"], ref["dx"]), TC.rel(got["dp"], ref["dp"]))
        assert got["ai"]["kind"] == 2
        if s == solver:
            above(got["fwd"], name, name)
    print(f"{name}: {solver} dx, dp rel: %.2e %.2e; Tsit5 at the same inputs: %.2e %.2e" % (errs[solver] + errs["tsit5"]))
    for got, t5 in zip(errs[solver], errs["tsit5"]):
        assert got < 3e-4 or got <= 2 * t5


@pytest.mark.parametrize("field", ["dense_chain", "wide_chain"])
def test_layer_object_forward_and_pullback_equal_the_handle_calls(gpu_pkg, field):
    P = gpu_pkg
    name = "phys_119"
    model, p, x, tol, span, sv, cots = G.pullback_inputs(P, name)
    node = P.NeuralODE(model, field=field, saveat=sv, save_start=False, regularize="none", abstol=tol, reltol=tol, maxiters=BIG,
                       tspan=span)
    st = node.initialstates(np.random.default_rng(0))
    xd, ps, gs = cu(x), cu(p), cu(cots)
    sol, st2 = node(xd, ps, st)
    dx, dp, info = node.pullback(xd, ps, st, gs)
    above(info["stats_fwd"], name, f"{field} layer")
    assert [float(t) for t in sol.t] == sv
    h = fresh(P, "small" if field == "dense_chain" else "wide", name)[0]
    plain = h.solve(xd, span[0], span[1], tol, tol, saveat=sv, maxiters=BIG)
    assert torch.equal(torch.stack(list(sol.u)), plain["u"]) and st2["nfe"] == plain["stats"]["nf"]
    fw = h.node_forward_record_ts(xd, span[0], span[1], tol, tol, sv, mode="none", maxiters=BIG)
    bw = h.node_backward_recorded_ts(gs)
    assert torch.equal(fw["u"], plain["u"]) and torch.equal(info["sol_u"], fw["u"]) and fw["stats"] == info["stats_fwd"]
    assert torch.equal(dx, bw["dx"]) and torch.equal(dp, bw["dp"])


def test_latent_training_step_past_the_record(gpu_pkg):
    """one Latent-ODE training step whose node solve records more than 128 steps: finite, and the same bits twice"""
    P = gpu_pkg
    dims, make, flat, node, batch = G.latent_inputs(P)
    ps = dict(latent=cu(flat), neural_ode=cu(node))
    dev_batch = tuple(cu(a) for a in batch)
    out = []
    for _ in range(2):
        model = make()
        st = model.initialstates(np.random.default_rng(5))
        hn = model.neural_ode.handle()
        seen, inner = [], hn.node_forward_record_ts

        def spy(*a, _inner=inner, _seen=seen, **kw):
            r = _inner(*a, **kw)
            _seen.append(r["stats"])
            return r
        hn.node_forward_record_ts = spy
        loss, _st, stats, grads, _tm = P.run_latent_training_step(model, ps, st, dev_batch, (2.0, 0.5))
        assert len(seen) == 1
        print(f"latent step: recorded forward naccept {seen[0]['naccept']} nreject {seen[0]['nreject']}; loss {float(loss):.6g}")
        assert seen[0]["naccept"] > G.LATENT["line"]
        assert np.isfinite(float(loss)) and stats["reg_val"] > 0
        assert all(bool(torch.isfinite(v).all()) for v in grads.values()) and float(grads["neural_ode"].abs().max()) > 0
        out.append((np.float32(loss), grads["latent"].clone(), grads["neural_ode"].clone(), stats["nfe"], np.float32(stats["reg_val"])))
    a, b = out
    assert a[0].tobytes() == b[0].tobytes() and a[3] == b[3] and a[4].tobytes() == b[4].tobytes()
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


# ======================================================================================================================
# 3. failed solves on chain handles
# ======================================================================================================================
def lin8_handle(P, kind, scale, solver="tsit5"):
    model, p, x = G.lin8(P, scale)
    if kind == "small":
        h, p2, x2 = TC.mk(P, model, G.LIN8["B"], scale=scale)
        assert np.array_equal(p, p2) and np.array_equal(x, x2)
        h.set_solver(solver)
    else:
        h = WA.handle_for(P, model, p, loop="auto")
    return h, model, p, x


def stop_equal(got, ref):
    """trace rows, nf, naccept, nreject, iters and t_final of a stopped solve, held with == (a NaN estimate equal to a NaN)"""
    assert len(got["trace"]) == len(ref["trace"]), (len(got["trace"]), len(ref["trace"]))
    for k in ("t", "dt", "accepted"):
        assert np.array_equal(got["trace"][k], ref["trace"][k]), k
    assert np.array_equal(got["trace"]["eest"], ref["trace"]["eest"], equal_nan=True)
    for k in ("nf", "naccept", "nreject", "iters", "t_final"):
        assert got["stats"][k] == ref["stats"][k], (k, got["stats"], ref["stats"])


def leave_a_record(h, xd, t0=0.0, t2=1.0, tol=1e-5):
    """a recorded forward that finishes: the failing call that follows finds a valid record on the handle, which it has to
    take away (a backward over a half-overwritten record would otherwise run)"""
    h.node_forward_record(xd, t0, t2, tol, tol, mode="unbiased", t1_or_rand=t0 + 0.43 * (t2 - t0), maxiters=BIG)
    assert h.record_generation() != 0


def usable_as_fresh(P, kind, scale, solver, h, x):
    """after the stop: a solve that finishes and a recorded forward / backward pair on the stopped handle == a fresh one's"""
    fr = lin8_handle(P, kind, scale, solver)[0]
    xd = cu(x)
    du = cu(G.cotangents(1, x, seed=5)[0])
    res = [(hh.solve(xd, 0.0, 1.0, 1e-5, 1e-5, saveat=[0.5, 1.0], maxiters=BIG),
            hh.node_forward_record(xd, 0.0, 1.0, 1e-5, 1e-5, mode="unbiased", t1_or_rand=0.43, maxiters=BIG),
            hh.node_backward_recorded(du, w_reg=G.W_REG)) for hh in (h, fr)]
    for a, b in zip(*res):
        same(a, b, "after the stop")


@pytest.mark.parametrize("kind", ["small", "wide"])
def test_tsit5_stops_deep_in_the_feed_loop(oracle, gpu_pkg, kind):
    """lin8 x3: DtNaN after more than 100 accepted steps, speculative launches queued behind the stop; then the recorded
    forward, which finds its record full first, retries, and stops the same way with a half-written record"""
    P = gpu_pkg
    from localregneuralde_jl_amd import _lib as L
    h, _, _, x = lin8_handle(P, kind, 3.0)
    c = G.LIN8
    xd = cu(x)
    ref = oracle.solve(rhs_field(oracle, h, 8), x, c["span"][0], c["span"][1], c["tol"], c["tol"], saveat=[c["span"][1]])
    got = h.solve(xd, c["span"][0], c["span"][1], c["tol"], c["tol"], saveat=[c["span"][1]], trace=True, raise_on_retcode=False)
    print(f"{kind} lin8 x3 Tsit5: retcode {got['retcode']} naccept {got['stats']['naccept']} nreject {got['stats']['nreject']} "
          f"t {got['stats']['t_final']:.4g}; oracle {G.stop_of(ref)}")
    assert got["retcode"] == G.RET_DT_NAN == ref["retcode"]
    assert (got["stats"]["naccept"], got["stats"]["nreject"]) == (ref["stats"]["naccept"], ref["stats"]["nreject"])
    assert got["stats"]["naccept"] > 100
    leave_a_record(h, xd)
    with pytest.raises(L.LrndeError) as e:
        h.node_forward_record(xd, c["span"][0], c["span"][1], c["tol"], c["tol"], mode="unbiased", t1_or_rand=10.0)
    assert e.value.code == G.RET_DT_NAN, e.value
    assert h.record_generation() == 0
    with pytest.raises(L.LrndeError):
        h.node_backward_recorded(xd, w_reg=G.W_REG)
    usable_as_fresh(P, kind, 3.0, "tsit5", h, x)


@pytest.mark.parametrize("host", [0, 1])
@pytest.mark.parametrize("solver,scale", [("vcab3", 3.0), ("vcabm3", 3.0), ("vcab3", 12.0)])
def test_adams_stops_equal_the_oracle(oracle, gpu_pkg, option, solver, scale, host):
    """the retcode, the trace and the counters of oracle.solve(..., solver=...) around Handle.rhs: DtNaN at x3, DtLessThanMin
    for VCAB3 at x12 (record_growth_cases says how x12 was looked at)"""
    P = gpu_pkg
    from localregneuralde_jl_amd import _lib as L
    h, _, _, x = lin8_handle(P, "small", scale, solver)
    c = G.LIN8
    xd = cu(x)
    want = G.LIN8_STOPS[(solver, scale)][0]
    ref = oracle.solve(rhs_field(oracle, h, 8), x, c["span"][0], c["span"][1], c["tol"], c["tol"], saveat=[c["span"][1]], solver=solver)
    got = with_loop(option, host, lambda: h.solve(xd, c["span"][0], c["span"][1], c["tol"], c["tol"], saveat=[c["span"][1]],
                                                  trace=True, raise_on_retcode=False))
    print(f"lin8 x{scale:g} {solver} host={host}: retcode {got['retcode']} naccept {got['stats']['naccept']} nreject "
          f"{got['stats']['nreject']} t {got['stats']['t_final']:.4g}; oracle around Handle.rhs {G.stop_of(ref)}")
    assert ref["retcode"] == want, "the oracle around Handle.rhs stops as the oracle over the float32 numpy field does"
    assert got["retcode"] == ref["retcode"]
    assert got["stats"]["naccept"] > G.SECOND_RECORD and got["stats"]["naccept"] + got["stats"]["nreject"] < G.MAX_ATTEMPTS
    stop_equal(got, ref)
    # the recorded forward grows its record past the stop's step count and stops the same way
    def rec():
        return h.node_forward_record(xd, c["span"][0], c["span"][1], c["tol"], c["tol"], mode="unbiased", t1_or_rand=5.0)
    with_loop(option, host, lambda: leave_a_record(h, xd))
    with pytest.raises(L.LrndeError) as e:
        with_loop(option, host, rec)
    assert e.value.code == want, e.value
    assert h.record_generation() == 0
    with_loop(option, host, lambda: usable_as_fresh(P, "small", scale, solver, h, x))


@pytest.mark.parametrize("kind", ["small", "wide"])
def test_maxiters_past_the_first_record(gpu_pkg, kind):
    """phys_74 with maxiters = 70: the record is full at step 65, the forward is retried, and stops at iteration 71 — status
    MaxIters (1), not Capacity (5)"""
    P = gpu_pkg
    from localregneuralde_jl_amd import _lib as L
    h, _, _, x, tol, span = fresh(P, kind, "phys_74")
    xd = cu(x)
    got = h.solve(xd, span[0], span[1], tol, tol, saveat=[span[1]], maxiters=G.MAXITERS_PAST, raise_on_retcode=False)
    print(f"{kind} phys_74 maxiters {G.MAXITERS_PAST}: retcode {got['retcode']} naccept {got['stats']['naccept']} nreject {got['stats']['nreject']}")
    assert got["retcode"] == G.RET_MAXITERS and got["stats"]["naccept"] > G.FIRST_RECORD
    for mode in MODES:
        leave_a_record(h, xd, span[0], span[1], tol)
        with pytest.raises(L.LrndeError) as e:
            h.node_forward_record(xd, span[0], span[1], tol, tol, mode=mode, t1_or_rand=draw(mode, span), maxiters=G.MAXITERS_PAST)
        assert e.value.code == G.RET_MAXITERS, e.value
        assert h.record_generation() == 0


@pytest.mark.parametrize("kind,name", [("small", "phys_74"), ("small", "phys_vcabm3_1e-5"), ("wide", "phys_74")])
def test_forward_and_backward_after_failures(gpu_pkg, kind, name):
    """tests/test_gpu_recovery.py's shape on the chain handles: after each failure the backward is refused, and forward,
    recorded forward and backward equal a fresh twin's bit for bit"""
    P = gpu_pkg
    from localregneuralde_jl_amd import _lib as L
    h, _, _, x, tol, span = fresh(P, kind, name)
    twin = fresh(P, kind, name)[0]
    xd = cu(x)
    du = cu(G.cotangents(1, x, seed=5)[0])
    kw = dict(mode="unbiased", t1_or_rand=draw("unbiased", span))
    args = (xd, span[0], span[1], tol, tol)
    want_f = twin.node_forward(*args, maxiters=BIG, **kw)
    want_r = twin.node_forward_record(*args, maxiters=BIG, **kw)
    want_b = twin.node_backward_recorded(du, w_reg=G.W_REG)
    above(want_r["stats"], name, f"{kind} {name}")
    xn = xd.clone(); xn[3, 5] = float("nan")
    failures = [("MaxIters in the plain forward", lambda: h.node_forward(*args, maxiters=4, **kw), G.RET_MAXITERS),
                ("MaxIters past the first record", lambda: h.node_forward_record(*args, maxiters=G.MAXITERS_PAST, **kw), G.RET_MAXITERS),
                ("DtNaN in the recorded forward", lambda: h.node_forward_record(xn, *args[1:], maxiters=BIG, **kw), G.RET_DT_NAN)]
    for tag, fail, code in failures:
        leave_a_record(h, xd, span[0], span[1], tol)
        with pytest.raises(L.LrndeError) as e:
            fail()
        assert e.value.code == code, (tag, e.value)
        assert h.record_generation() == 0, tag
        with pytest.raises(L.LrndeError):
            h.node_backward_recorded(du, w_reg=G.W_REG)
        same(h.node_forward(*args, maxiters=BIG, **kw), want_f, tag)
        same(h.node_forward_record(*args, maxiters=BIG, **kw), want_r, tag)
        same(h.node_backward_recorded(du, w_reg=G.W_REG), want_b, tag)
        with pytest.raises(L.LrndeError):                      # the record is consumed by its backward
            h.node_backward_recorded(du, w_reg=G.W_REG)
    # a NaN cotangent: the backward errors or hands back non-finite gradients; the next pair is clean
    h.node_forward_record(*args, maxiters=BIG, **kw)
    dn = du.clone(); dn[0, 0] = float("nan")
    try:
        got = h.node_backward_recorded(dn, w_reg=G.W_REG)
        assert not torch.isfinite(got["dx"]).all()
    except L.LrndeError:
        pass
    same(h.node_forward_record(*args, maxiters=BIG, **kw), want_r, "after a NaN cotangent")
    same(h.node_backward_recorded(du, w_reg=G.W_REG), want_b, "after a NaN cotangent")
    same(h.node_forward(*args, maxiters=BIG, **kw), want_f, "after a NaN cotangent")
