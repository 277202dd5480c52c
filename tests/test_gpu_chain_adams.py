"""VCAB3 / VCABM3 on the small Dense-chain handle: the one-launch-per-attempt device loop (csrc/lrnde_chain_adams.hpp,
k_adams_chain) and, under LRNDE_ADAMS_HOST=1, the host-driven loop (csrc/lrnde_adams.hpp).

The reference for bits is the C oracle's adams_solve (start-up, recurrences, controller, Hermite saves, counters) run around
the handle's own f-evals: oracle.PyField over Handle.rhs (k_rhs_chain, parent-commit code that tests/test_gpu_chain.py
pins to float64).  Everything this change adds is therefore held
with == to an independent statement of it.  Independent of both restatements: scipy DOP853 in float64 and float64 torch
autograd through a fine RK4.  Cases and their reasons: tests/chain_adams_cases.py."""
import numpy as np
import pytest
import torch

import chain_adams_cases as K

pytestmark = pytest.mark.gpu

SOLVERS = K.SOLVERS


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def mk_handle(model, p):
    from localregneuralde_jl_amd.layers import Handle, _chain_desc
    h = Handle(_chain_desc(model))
    h.set_params(torch.from_numpy(p))
    return h


def rhs_field(O, h, D):
    """the oracle's view of the handle's field: upload, the handle's rhs kernel, download"""
    return O.PyField(D, lambda u, t: h.rhs(cu(u), float(t)).cpu().numpy())


def trace_equal(got, ref):
    assert len(got) == len(ref), (len(got), len(ref))
    for i, (a, b) in enumerate(zip(got, ref)):
        assert tuple(a) == tuple(b), (i, tuple(a), tuple(b))


STAT_KEYS = ("nf", "naccept", "nreject", "iters", "nsaved", "t_final", "eest_last", "dt_init")


def solve_equal(got, ref):
    trace_equal(got["trace"], ref["trace"])
    for k in STAT_KEYS:
        assert got["stats"][k] == ref["stats"][k], (k, got["stats"], ref["stats"])
    assert np.array_equal(got["t"], ref["t"])
    assert np.array_equal(got["u"].cpu().numpy(), ref["u"])


# the reference traces of test 1, kept for the coverage test that follows it
_COVER = {}


# ---- 1. solve == oracle, attempt by attempt ----
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("name", list(K.CASES))
def test_solve_equals_the_oracle_attempt_by_attempt(oracle, gpu_pkg, name, solver):
    model, p, x, tol = K.case(gpu_pkg, name)
    h = mk_handle(model, p)
    fld = rhs_field(oracle, h, x.shape[1])
    ref = oracle.solve(fld, x, 0.0, 1.0, tol, tol, saveat=K.SAVEAT, save_start=True, solver=solver)
    h.set_solver(solver)
    got = h.solve(cu(x), 0.0, 1.0, tol, tol, saveat=K.SAVEAT, save_start=True, trace=True)
    assert ref["retcode"] == 0 and got["retcode"] == 0
    cov = K.coverage(ref["trace"])
    _COVER[(name, solver)] = cov
    print(name, solver, cov)
    assert cov["attempts"] <= K.MAX_ATTEMPTS
    solve_equal(got, ref)
    assert list(ref["t"]) == [np.float32(s) for s in K.SAVEAT]
    per = 2 if solver == "vcabm3" else 1
    nstart = acc = 0
    for r in ref["trace"]:
        nstart += acc < 2
        acc += int(r["accepted"])
    assert got["stats"]["nf"] == 3 + 3 * nstart + per * (len(ref["trace"]) - nstart)


@pytest.mark.parametrize("solver", SOLVERS)
def test_the_cases_reach_every_branch(oracle, gpu_pkg, solver):
    """from the reference traces of the test above (recomputed when this test runs alone): a rejected multistep attempt, a
    rejected start-up attempt, an accepted step without a saveat point directly after one that has two"""
    for name in K.CASES:
        if (name, solver) not in _COVER:
            model, p, x, tol = K.case(gpu_pkg, name)
            h = mk_handle(model, p)
            ref = oracle.solve(rhs_field(oracle, h, x.shape[1]), x, 0.0, 1.0, tol, tol, saveat=K.SAVEAT, save_start=True, solver=solver)
            _COVER[(name, solver)] = K.coverage(ref["trace"])
    cov = [_COVER[(name, solver)] for name in K.CASES]
    assert sum(c["multistep_rejects"] for c in cov) >= 1
    assert sum(c["startup_rejects"] for c in cov) >= 1
    assert any(c["two_then_none"] for c in cov)


# ---- 2. save_everystep ----
@pytest.mark.parametrize("solver", SOLVERS)
def test_every_step_series_equals_the_oracle(oracle, gpu_pkg, solver):
    model, p, x, tol = K.case(gpu_pkg, "td3")
    h = mk_handle(model, p)
    ref = oracle.solve(rhs_field(oracle, h, x.shape[1]), x, 0.0, 1.0, tol, tol, solver=solver)
    h.set_solver(solver)
    got = h.solve(cu(x), 0.0, 1.0, tol, tol)
    assert np.array_equal(got["t"], ref["t"]) and np.array_equal(got["u"].cpu().numpy(), ref["u"])
    assert len(ref["t"]) == ref["stats"]["naccept"] > 10


# ---- 3. layer forward ----
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("mode", ["none", "unbiased", "biased"])
def test_layer_forward_equals_the_oracle(oracle, gpu_pkg, solver, mode):
    """the global solve by the Adams method, sol(t1) from its Hermite interpolant, the local regularisation step by Tsit5"""
    model, p, x, tol = K.case(gpu_pkg, "physionet_b17")
    tol = 1e-4
    h = mk_handle(model, p)
    ref = oracle.node_forward(rhs_field(oracle, h, x.shape[1]), x, 0.0, 1.0, tol, tol, mode=mode, t1_or_rand=0.37, solver=solver)
    h.set_solver(solver)
    got = h.node_forward(cu(x), 0.0, 1.0, tol, tol, mode=mode, t1_or_rand=0.37)
    assert ref["retcode"] == 0
    assert np.array_equal(got["u_end"].cpu().numpy(), ref["u_end"])
    assert got["nfe"] == ref["nfe"] and got["t1"] == ref["t1"]
    assert np.float32(got["reg_val"]) == np.float32(ref["reg_val"])
    for k in ("nf", "naccept", "nreject"):
        assert got["stats"][k] == ref["stats"][k], (k, got["stats"], ref["stats"])
    if mode != "none":
        assert got["nfe"] == ref["stats"]["nf"] + 9 and got["reg_val"] > 0


# ---- 4. device loop == host loop ----
@pytest.fixture
def adams_host(gpu_pkg):
    """switches LRNDE_ADAMS_HOST on for the calls made through it, and off again afterwards"""
    def run(fn):
        try:
            gpu_pkg.set_option("LRNDE_ADAMS_HOST", 1)
            return fn()
        finally:
            gpu_pkg.set_option("LRNDE_ADAMS_HOST", 0)
    yield run
    gpu_pkg.set_option("LRNDE_ADAMS_HOST", 0)


@pytest.mark.parametrize("solver", SOLVERS)
def test_device_loop_equals_the_host_loop(gpu_pkg, adams_host, solver):
    model, p, x, tol = K.case(gpu_pkg, "physionet_b17")
    tol = 1e-4
    xd = cu(x)
    h = mk_handle(model, p)
    h.last_solve_kernel_ms()   # solves count their step launches from here on
    # the speculative-launch slack of the feed loop at these inputs: what the Tsit5 solve enqueues beyond its attempts
    t5 = h.solve(xd, 0.0, 1.0, tol, tol, saveat=K.SAVEAT, save_start=True, trace=True)
    slack = h.last_solve_kernel_ms()[1] - len(t5["trace"])
    assert slack >= 0
    h.set_solver(solver)
    dev = h.solve(xd, 0.0, 1.0, tol, tol, saveat=K.SAVEAT, save_start=True, trace=True)
    n_dev = h.last_solve_kernel_ms()[1]
    host = adams_host(lambda: h.solve(xd, 0.0, 1.0, tol, tol, saveat=K.SAVEAT, save_start=True, trace=True))
    n_host = h.last_solve_kernel_ms()[1]
    attempts = len(dev["trace"])
    print(solver, "attempts", attempts, "launches: device loop", n_dev, "host loop", n_host, "Tsit5 slack", slack)
    trace_equal(dev["trace"], host["trace"])
    assert np.array_equal(dev["t"], host["t"]) and torch.equal(dev["u"], host["u"])
    for k in STAT_KEYS:
        assert dev["stats"][k] == host["stats"][k], k
    assert n_dev <= attempts + slack
    assert n_host >= 3 * attempts
    # the dense record's consequences: end-state and series pullbacks from either loop's record
    g = cu(np.random.default_rng(4).standard_normal(x.shape).astype(np.float32))
    gs = cu(np.random.default_rng(5).standard_normal((4,) + x.shape).astype(np.float32))
    sv4 = [0.25, 0.5, 0.8, 1.0]

    def end_pair():
        fw = h.node_forward_record(xd, 0.0, 1.0, tol, tol, mode="unbiased", t1_or_rand=0.43)
        return fw, h.node_backward_recorded(g, w_reg=1.5)

    def series_pair():
        fw = h.node_forward_record_ts(xd, 0.0, 1.0, tol, tol, sv4, mode="none")
        return fw, h.node_backward_recorded_ts(gs)
    for pair in (end_pair, series_pair):
        (fd, bd), (fh, bh) = pair(), adams_host(pair)
        assert torch.equal(fd["u_end"], fh["u_end"]) and fd["nfe"] == fh["nfe"] and fd["reg_val"] == fh["reg_val"]
        assert torch.equal(bd["dx"], bh["dx"]) and torch.equal(bd["dp"], bh["dp"])
        assert bool(torch.isfinite(bd["dp"]).all()) and float(bd["dp"].abs().max()) > 0


# ---- 5. independent of both restatements ----
@pytest.mark.parametrize("solver", SOLVERS)
def test_solution_against_float64(gpu_pkg, solver):
    """the same field integrated in float64 by scipy's DOP853 at 1e-12; tests/test_gpu_adams.py's bars"""
    from scipy.integrate import solve_ivp
    import test_gpu_chain as TC
    P = gpu_pkg
    model = K.models(P)["small3"]
    B = 5
    p, x = K.inputs(P, model, B, 3.0)
    f64 = TC.Chain64(model, p).f64
    ex = solve_ivp(lambda t, y: f64(y.reshape(B, 12), t).reshape(-1), (0.0, 1.0), x.astype(np.float64).reshape(-1), method="DOP853",
                   rtol=1e-12, atol=1e-12).y[:, -1].reshape(B, 12)
    h = mk_handle(model, p)
    h.set_solver(solver)
    errs = []
    for tol in (1e-3, 1e-4, 1e-5):
        got = h.solve(cu(x), 0.0, 1.0, tol, tol, saveat=[1.0])
        errs.append(np.abs(got["u"][-1].cpu().numpy() - ex).max() / np.abs(ex).max())
    print(solver, "rel err vs float64 at tol 1e-3, 1e-4, 1e-5:", ["%.2e" % e for e in errs])
    assert errs[0] < 5e-2 and errs[1] < 1e-2 and errs[2] < 2e-3 and errs[2] < errs[0]


@pytest.mark.parametrize("solver", SOLVERS)
def test_pullback_against_float64_autograd(gpu_pkg, solver):
    """The series pullback over the Adams forward's Hermite record against float64 torch autograd through a fine RK4
    (tests/test_gpu_chain.py's reference_grads and inputs).  The bar is that file's for the Tsit5 chain at these inputs,
    3e-4 of each gradient's norm; where the Adams forward's coarser solution exceeds it, twice the Tsit5 pullback's own
    error measured here on the same inputs (the reversed solve is the same Tsit5; only the interpolant differs).
    Measured on an MI355X: VCAB3 dx 1.8e-5, dp 1.7e-5; VCABM3 2.4e-5, 2.3e-5; Tsit5 1.5e-6, 1.4e-6 — the 3e-4 bar holds."""
    import test_gpu_chain as TC
    P = gpu_pkg
    model = TC.physionet(P)
    _, p, x = TC.mk(P, model, 12, scale=1.5)
    times = [0.25, 0.5, 1.0]
    xd, ps = cu(x), cu(p)
    cots = np.random.default_rng(11).standard_normal((3, 12, 20)).astype(np.float32)
    gx, gp = TC.reference_grads(model, p, x, times, cots)
    errs = {}
    for s in ("tsit5", solver):
        node = P.NeuralODE(model, regularize="none", abstol=1e-6, reltol=1e-6, saveat=times, save_start=False, maxiters=10000,
                           field="dense_chain")
        node.handle().set_solver(s)
        st = node.initialstates(np.random.default_rng(3))
        dx, dp, info = node.pullback(xd, ps, st, cu(cots))
        errs[s] = (TC.rel(dx.cpu().numpy(), gx), TC.rel(dp.cpu().numpy(), gp))
        assert info["adjoint_loop"] == "chain_device"
    print(solver, "dx, dp rel: %.2e %.2e; Tsit5 at the same inputs: %.2e %.2e" % (errs[solver] + errs["tsit5"]))
    for got, t5 in zip(errs[solver], errs["tsit5"]):
        assert got < 3e-4 or got <= 2 * t5


# ---- 6. Python surface ----
@pytest.mark.parametrize("solver", SOLVERS)
def test_layer_object_forward_and_pullback_equal_the_handle_calls(gpu_pkg, solver):
    """the layer object's `solver` keyword stays closed for the chain fields (tests/test_host_chain.py pins that); the
    layer runs with the solver its handle was given"""
    P = gpu_pkg
    model, p, x, _ = K.case(P, "physionet_b8")
    tol, sv = 1e-4, [0.25, 0.5, 0.8, 1.0]
    node = P.NeuralODE(model, field="dense_chain", saveat=sv, save_start=False, regularize="none", abstol=tol, reltol=tol)
    node.handle().set_solver(solver)
    st = node.initialstates(np.random.default_rng(0))
    xd, ps = cu(x), cu(p)
    sol, st2 = node(xd, ps, st)
    assert [float(t) for t in sol.t] == [float(np.float32(t)) for t in sv]
    gs = cu(np.random.default_rng(7).standard_normal((4,) + x.shape).astype(np.float32))
    dx, dp, info = node.pullback(xd, ps, st, gs)
    h = mk_handle(model, p)
    h.set_solver(solver)
    plain = h.solve(xd, 0.0, 1.0, tol, tol, saveat=sv)
    assert torch.equal(torch.stack(list(sol.u)), plain["u"]) and st2["nfe"] == plain["stats"]["nf"]
    fw = h.node_forward_record_ts(xd, 0.0, 1.0, tol, tol, sv, mode="none")
    bw = h.node_backward_recorded_ts(gs)
    assert torch.equal(fw["u"], plain["u"]) and torch.equal(info["sol_u"], fw["u"])
    assert torch.equal(dx, bw["dx"]) and torch.equal(dp, bw["dp"])
    t5 = P.NeuralODE(model, field="dense_chain", saveat=sv, save_start=False, regularize="none", abstol=tol, reltol=tol)
    s5, _ = t5(xd, ps, st)
    assert not torch.equal(s5.u[-1], sol.u[-1]) and float((s5.u[-1] - sol.u[-1]).abs().max()) < 1e-2


def test_latent_training_step_with_an_adams_solver(gpu_pkg):
    import latent_cases as LC
    P = gpu_pkg
    dims, T, B = LC.TINY, 4, 9
    times = [0.25, 0.5, 0.75, 1.0]
    model = P.construct_time_series(*dims, saveat=times, regularize="unbiased", abstol=1e-5, reltol=1e-5, maxiters=10000)
    model.neural_ode.handle().set_solver("vcabm3")
    t5 = P.construct_time_series(*dims, saveat=times, regularize="unbiased", abstol=1e-5, reltol=1e-5, maxiters=10000)
    flat, node = LC.make_params(dims, seed=11), LC.make_node_params(dims, seed=12)
    data, mask, dt = LC.make_batch(dims, B, T, seed=13, unobserved_column=False)
    mask[:, 0, 0] = 1
    ps = dict(latent=cu(flat), neural_ode=cu(node))
    st = model.initialstates(np.random.default_rng(5))
    loss, st_, stats, grads, _ = P.run_latent_training_step(model, ps, st, (cu(data), cu(mask), cu(dt)), (2.0, 0.5))
    assert np.isfinite(float(loss)) and stats["reg_val"] > 0 and stats["nfe"] > 9
    assert tuple(grads["latent"].shape) == (flat.size,) and tuple(grads["neural_ode"].shape) == (node.size,)
    assert all(bool(torch.isfinite(v).all()) for v in grads.values()) and float(grads["neural_ode"].abs().max()) > 0
    # the Adams solve really ran: other evaluation counts than the Tsit5 model's, the same loss to the solvers' accuracy
    # (the solution bar of test_solution_against_float64 at tol 1e-5, 2e-3 of the state's scale, with a factor 5 for the loss)
    loss5, _, stats5, _, _ = P.run_latent_training_step(t5, ps, st, (cu(data), cu(mask), cu(dt)), (2.0, 0.5))
    assert stats["nfe"] != stats5["nfe"] and abs(float(loss) - float(loss5)) <= 1e-2 * abs(float(loss5))


# ---- 8. refusals ----
def test_adams_and_the_discrete_adjoint_refuse_each_other(gpu_pkg):
    """in both orders, LRNDE_UNSUPPORTED with a message, the handle usable afterwards; the wide handle stays Tsit5 only
    (tests/test_gpu_wide_chain.py pins its refusal)"""
    from localregneuralde_jl_amd import _lib as L
    P = gpu_pkg
    model, p, x, tol = K.case(P, "one_layer")
    for solver in SOLVERS:
        h = mk_handle(model, p)
        before = h.rhs(cu(x), 0.2)
        h.set_solver(solver)
        with pytest.raises(L.LrndeError) as e:
            h.set_sensealg("discrete")
        assert e.value.code == 8 and "Tsit5" in str(e.value)
        adams = h.solve(cu(x), 0.0, 1.0, tol, tol, saveat=[1.0])       # still the Adams solve
        h.set_solver("tsit5")
        h.set_sensealg("discrete")
        with pytest.raises(L.LrndeError) as e:
            h.set_solver(solver)
        assert e.value.code == 8 and "Tsit5" in str(e.value)
        assert torch.equal(h.rhs(cu(x), 0.2), before)
        t5 = h.solve(cu(x), 0.0, 1.0, tol, tol, saveat=[1.0])          # and still the Tsit5 one
        assert adams["retcode"] == 0 and t5["retcode"] == 0 and adams["stats"]["nf"] != t5["stats"]["nf"]
        h.set_sensealg("interpolating")
        h.set_solver(solver)
        # the layer object's keyword stays closed for the chain fields, with a message that names the handle's setter
        with pytest.raises(NotImplementedError, match="set_solver"):
            P.NeuralODE(model, field="dense_chain", solver=solver)


# ---- 9. robustness of the loop ----
@pytest.mark.parametrize("solver", SOLVERS)
def test_maxiters_reports_and_a_second_solve(oracle, gpu_pkg, solver):
    P = gpu_pkg
    model, p, x, tol = K.case(P, "physionet_b1")
    xd = cu(x)
    h = mk_handle(model, p)
    fld = rhs_field(oracle, h, x.shape[1])
    h.set_solver(solver)
    # maxiters = 5: the MAXITERS retcode and the oracle's counters
    ref5 = oracle.solve(fld, x, 0.0, 1.0, tol, tol, saveat=K.SAVEAT, save_start=True, solver=solver, maxiters=5)
    got5 = h.solve(xd, 0.0, 1.0, tol, tol, saveat=K.SAVEAT, save_start=True, trace=True, maxiters=5, raise_on_retcode=False)
    assert ref5["retcode"] == 1 and got5["retcode"] == 1
    trace_equal(got5["trace"], ref5["trace"])
    for k in ("nf", "naccept", "nreject", "iters", "nsaved", "t_final", "dt_init"):
        assert got5["stats"][k] == ref5["stats"][k], (k, got5["stats"], ref5["stats"])
    # the copy-polled fall-back gives the bits of the report-driven feed
    a = h.solve(xd, 0.0, 1.0, tol, tol, saveat=K.SAVEAT, save_start=True, trace=True)
    h.set_reports(False)
    try:
        b = h.solve(xd, 0.0, 1.0, tol, tol, saveat=K.SAVEAT, save_start=True, trace=True)
    finally:
        h.set_reports(True)
    trace_equal(a["trace"], b["trace"])
    assert torch.equal(a["u"], b["u"]) and np.array_equal(a["t"], b["t"]) and a["stats"] == b["stats"]
    # no Adams state survives a solve: new parameters on this handle == a fresh handle
    p2 = (p * np.float32(0.5)).astype(np.float32)
    h.set_params(torch.from_numpy(p2))
    again = h.solve(xd, 0.0, 1.0, tol, tol, saveat=K.SAVEAT, save_start=True, trace=True)
    fresh_h = mk_handle(model, p2)
    fresh_h.set_solver(solver)
    fresh = fresh_h.solve(xd, 0.0, 1.0, tol, tol, saveat=K.SAVEAT, save_start=True, trace=True)
    trace_equal(again["trace"], fresh["trace"])
    assert torch.equal(again["u"], fresh["u"]) and again["stats"] == fresh["stats"]
    assert not torch.equal(again["u"], a["u"])
