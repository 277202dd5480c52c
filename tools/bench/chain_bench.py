"""Dense-chain field bench: the PhysioNet latent ODE's gen_dynamics (Chain(tanh.(u), 8 Dense 20 <-> 40, tanh);
experiments/src/construct.jl:236-244, physionet.yml) at B = 512, abstol = reltol = 1.4e-8, :unbiased, a saveat series.

Prints one JSON line: attempted steps, step-kernel launches per attempted step and the solve's kernel time per attempt,
the layer forward and forward + pullback in ms per batch (median of --reps), and the same adaptive Tsit5 solve written in
eager torch fp32 on the same GPU (host-side controller, one EEst read-back per attempted step) as a baseline.

The pullback legs (4-time series and the experiment's 49-time series): node.pullback alone (recorded forward + backward)
and the backward alone from a record, ms per batch (median of --bwd-reps after warm-up) with the run's min / max, the
reversed solve's attempted steps, us per attempt of the backward alone, which loop ran it (adjoint_loop), its launches per
attempt and host waits.  LRNDE_ADJ_HOST=1 in the environment selects the host-controlled loop: the comparison path.
--sensealg TrackerAdjoint (or ReverseDiffAdjoint / discrete) builds the layers with the discrete adjoint (one launch over
the record); the default is the continuous adjoint.

--solver vcab3 | vcabm3 runs every leg with that global solver (one launch per attempted step, csrc/lrnde_chain_adams.hpp);
--adams-host adds LRNDE_ADAMS_HOST=1, the host-driven loop.  --solver-sweep prints the table of DESIGN.md 4.8.1 instead:
Tsit5, VCAB3 and VCABM3 on the device loop and both Adams methods under the switch, at tolerance 1e-3 with the 49-point
series and at 1.4e-8 with the 4-point one (profiles/chain_adams/).

    python tools/bench/chain_bench.py [--reps 5] [--B 512] [--bwd-reps 30] [--sensealg TrackerAdjoint] [--solver vcab3] [--adams-host]
    python tools/bench/chain_bench.py --solver-sweep [--reps 5]
    rocprofv3 --kernel-trace --stats -- python tools/bench/chain_bench.py      (us per k_step_chain launch)
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import lrnde_amd as P  # noqa: E402

TOL = 1.4e-8
MAXITERS = 20000   # of the --solver-sweep legs: a leg that does not finish within it is reported with its retcode, not timed
SAVEAT = [0.25, 0.5, 0.75, 1.0]
C = [0.161, 0.327, 0.9, 0.9800255409045097, 1.0, 1.0]
A = [[0.161], [-0.008480655492356989, 0.335480655492357], [2.8971530571054935, -6.359448489975075, 4.3622954328695815],
     [5.325864828439257, -11.748883564062828, 7.4955393428898365, -0.09249506636175525],
     [5.86145544294642, -12.92096931784711, 8.159367898576159, -0.071584973281401, -0.028269050394068383],
     [0.09646076681806523, 0.01, 0.4798896504144996, 1.379008574103742, -3.290069515436081, 2.324710524099774]]
BT = [-0.00178001105222577714, -0.0008164344596567469, 0.007880878010261995, -0.1447110071732629,
      0.5823571654525552, -0.45808210592918697, 0.015151515151515152]


def physionet():
    return P.Chain(P.Activation("tanh"), *[P.Dense(20, 40, "tanh") if i % 2 == 0 else P.Dense(40, 20, "tanh") for i in range(8)])


def eager_solve(Ws, x, t0, t1, tol, maxiters=100000):
    """adaptive Tsit5 (initdt, PI controller with the same constants) in eager torch fp32: the baseline"""
    def f(u):
        h = torch.tanh(u)
        for W, b in Ws:
            h = torch.tanh(torch.addmm(b, h, W.t()))
        return h

    def sc(a, b=None):
        m = a.abs() if b is None else torch.maximum(a.abs(), b.abs())
        return tol + m * tol
    rms = lambda v: float(torch.sqrt((v * v).mean()))
    u, t = x, t0
    k1 = f(u)
    d0, d1 = rms(u / sc(u)), rms(k1 / sc(u))
    dt0 = 1e-6 if d0 < 1e-5 or d1 < 1e-5 else 0.01 * d0 / d1
    d2 = rms((f(u + dt0 * k1) - k1) / sc(u)) / dt0
    dt = min(100 * dt0, 10 ** (-(2 + np.log10(max(d1, d2, 1e-15))) / 5), t1 - t0)
    qold, nacc, nrej = 1e-4, 0, 0
    for _ in range(maxiters):
        if t >= t1:
            break
        dt = min(dt, t1 - t)
        ks = [k1]
        for s in range(6):
            acc = ks[0] * A[s][0]
            for j in range(1, s + 1):
                acc = acc + ks[j] * A[s][j]
            y = u + dt * acc
            ks.append(f(y))
        utilde = dt * sum(b * k for b, k in zip(BT, ks))
        eest = rms(utilde / sc(u, y))
        q = max(0.1, min(5.0, eest ** 0.14 / qold ** 0.08 / 0.9)) if eest > 0 else 0.1
        if eest <= 1.0:
            u, k1, t, qold, nacc = y, ks[6], t + dt, max(eest, 1e-4), nacc + 1
            dt = dt / q
        else:
            nrej += 1
            dt = dt / min(5.0, eest ** 0.14 / 0.9)
    return u, nacc, nrej


def pullback_leg(node, h, xd, ps, st, times, B, reps):
    """node.pullback alone and the backward alone over a saveat series with a cotangent at every time"""
    cots = torch.from_numpy(np.random.default_rng(1).standard_normal((len(times), B, 20)).astype(np.float32)).cuda()
    full, bwd, info = [], [], None
    for i in range(reps + 3):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        _, _, info = node.pullback(xd, ps, st, cots, w_reg=10.0)
        torch.cuda.synchronize(); t1 = time.perf_counter()
        h.node_forward_record_ts(xd, 0.0, 1.0, TOL, TOL, times, mode="unbiased", t1_or_rand=0.37, maxiters=100000)
        torch.cuda.synchronize(); t2 = time.perf_counter()
        h.node_backward_recorded_ts(cots, w_reg=10.0)
        torch.cuda.synchronize(); t3 = time.perf_counter()
        if i >= 3:
            full.append((t1 - t0) * 1e3); bwd.append((t3 - t2) * 1e3)
    sb = info["stats_bwd"]
    attempts = sb["naccept"] + sb["nreject"]
    ai = h.last_adjoint_info() if hasattr(h, "last_adjoint_info") else None
    med = statistics.median
    return dict(ntimes=len(times), pullback_ms=round(med(full), 3), pullback_ms_min=round(min(full), 3), pullback_ms_max=round(max(full), 3),
                backward_ms=round(med(bwd), 3), backward_ms_min=round(min(bwd), 3), backward_ms_max=round(max(bwd), 3),
                adjoint_naccept=sb["naccept"], adjoint_nreject=sb["nreject"], adjoint_attempts=attempts,
                us_per_adjoint_attempt=round(1e3 * med(bwd) / max(attempts, 1), 2), adjoint_loop=info.get("adjoint_loop"),
                launches_per_attempt=round(ai["launches"] / max(attempts, 1), 3) if ai else None,
                host_waits=ai["host_waits"] if ai else None)


def solver_leg(model, xd, ps, B, solver, adams_host, tol, times, reps):
    """one solver on one (tolerance, series): attempts and f-evals per pass, us per attempted step from the solve's own
    event bracket (lrnde_last_solve_kernel_ms), the layer forward and forward + series pullback in ms (median, min, max)"""
    P.set_option("LRNDE_ADAMS_HOST", 1 if adams_host else 0)
    try:
        node = P.NeuralODE(model, regularize="unbiased", abstol=tol, reltol=tol, saveat=times, save_start=False,
                           maxiters=MAXITERS, field="dense_chain")
        node.handle().set_solver(solver)   # (the layer's solver keyword is closed for chain fields: the handle's setter)
        st = node.initialstates(np.random.default_rng(0))
        cots = torch.from_numpy(np.random.default_rng(1).standard_normal((len(times), B, 20)).astype(np.float32)).cuda()
        h = node._bind(ps)
        r = h.solve(xd, 0.0, 1.0, tol, tol, saveat=times, maxiters=MAXITERS, raise_on_retcode=False)
        if r["retcode"] != 0:   # (a float32 error estimate can stall an order-3 method far below its tolerance floor)
            return dict(solver=solver, loop="host" if adams_host else "device", tol=tol, ntimes=len(times), retcode=r["retcode"],
                        attempts=r["stats"]["naccept"] + r["stats"]["nreject"], t_final=float(r["stats"]["t_final"]))
        h.last_solve_kernel_ms()
        per, launches = [], 0
        for _ in range(reps):
            r = h.solve(xd, 0.0, 1.0, tol, tol, saveat=times, maxiters=MAXITERS)
            ms, launches = h.last_solve_kernel_ms()
            per.append(1e3 * ms / max(r["stats"]["naccept"] + r["stats"]["nreject"], 1))
        fwd, fb = [], []
        for i in range(reps + 2):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            node(xd, ps, st)
            torch.cuda.synchronize(); t1 = time.perf_counter()
            node.pullback(xd, ps, st, cots, w_reg=10.0)
            torch.cuda.synchronize(); t2 = time.perf_counter()
            if i >= 2:
                fwd.append((t1 - t0) * 1e3); fb.append((t2 - t1) * 1e3)
    finally:
        P.set_option("LRNDE_ADAMS_HOST", 0)
    mmm = lambda v, nd=3: dict(median=round(statistics.median(v), nd), min=round(min(v), nd), max=round(max(v), nd))
    attempts = r["stats"]["naccept"] + r["stats"]["nreject"]
    # (the host loop's solve is not bracketed by events: its us per attempt comes from the forward's wall time instead)
    return dict(solver=solver, loop="host" if adams_host else ("device" if solver != "tsit5" else "tsit5"), tol=tol, ntimes=len(times),
                attempts=attempts, naccept=r["stats"]["naccept"], nreject=r["stats"]["nreject"], nf=r["stats"]["nf"],
                step_launches=launches, us_per_attempt=None if adams_host else mmm(per, 2),
                layer_forward_ms=mmm(fwd), forward_us_per_attempt=round(1e3 * statistics.median(fwd) / max(attempts, 1), 2),
                forward_series_pullback_ms=mmm(fb))


def solver_sweep(args, model, xd, ps, B):
    """Tsit5 against VCAB3 / VCABM3 on the device loop and under LRNDE_ADAMS_HOST=1, at the experiment's tolerance with its
    49-point series and at 1.4e-8 with the 4-point series: one JSON line"""
    rows = []
    for tol, times in ((1e-3, [(i + 1) / 49.0 for i in range(49)]), (TOL, SAVEAT)):
        for solver, host in (("tsit5", False), ("vcab3", False), ("vcabm3", False), ("vcab3", True), ("vcabm3", True)):
            rows.append(solver_leg(model, xd, ps, B, solver, host, tol, times, args.reps))
    print(json.dumps(dict(workload="physionet_gen_dynamics_solvers", B=B, reps=args.reps, legs=rows)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bwd-reps", type=int, default=30)
    ap.add_argument("--B", type=int, default=512)
    ap.add_argument("--sensealg", default=None)
    ap.add_argument("--solver", default="tsit5", help="tsit5 | vcab3 | vcabm3: the layer's global solver in every leg")
    ap.add_argument("--adams-host", action="store_true", help="LRNDE_ADAMS_HOST=1: the host-driven Adams loop (the 'before' leg)")
    ap.add_argument("--solver-sweep", action="store_true", help="the Tsit5 / VCAB3 / VCABM3 table of DESIGN.md 4.8.1 instead")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    B = args.B
    model = physionet()
    p = P.glorot_chain_params(model, seed=0)
    x = (np.random.default_rng(2).random((B, 20), dtype=np.float32) - np.float32(0.5)) * np.float32(2)
    xd, ps = torch.from_numpy(x).cuda(), torch.from_numpy(p).cuda()
    if args.solver_sweep:
        return solver_sweep(args, model, xd, ps, B)
    if args.adams_host:
        P.set_option("LRNDE_ADAMS_HOST", 1)
    node = P.NeuralODE(model, regularize="unbiased", abstol=TOL, reltol=TOL, saveat=SAVEAT, save_start=False, maxiters=100000,
                       field="dense_chain", sensealg=args.sensealg)
    node.handle().set_solver(args.solver)
    st = node.initialstates(np.random.default_rng(0))
    cots = torch.from_numpy(np.random.default_rng(1).standard_normal((len(SAVEAT), B, 20)).astype(np.float32)).cuda()
    h = node._bind(ps)
    # the plain solve: kernel time and launches of its attempted steps
    h.solve(xd, 0.0, 1.0, TOL, TOL, saveat=SAVEAT, maxiters=100000)
    h.last_solve_kernel_ms()   # (the first call switches the solve's event bracket on)
    r = h.solve(xd, 0.0, 1.0, TOL, TOL, saveat=SAVEAT, maxiters=100000)
    solve_ms, launches = h.last_solve_kernel_ms()
    attempts = r["stats"]["naccept"] + r["stats"]["nreject"]
    fwd, fb = [], []
    for i in range(args.reps + 1):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        node(xd, ps, st)
        torch.cuda.synchronize(); t1 = time.perf_counter()
        node.pullback(xd, ps, st, cots, w_reg=10.0)
        torch.cuda.synchronize(); t2 = time.perf_counter()
        if i:
            fwd.append((t1 - t0) * 1e3); fb.append((t2 - t0) * 1e3)
    legs = []
    for times in (SAVEAT, [(i + 1) / 49.0 for i in range(49)]):
        nd = P.NeuralODE(model, regularize="unbiased", abstol=TOL, reltol=TOL, saveat=times, save_start=False, maxiters=100000,
                         field="dense_chain", sensealg=args.sensealg)
        nd.handle().set_solver(args.solver)
        legs.append(pullback_leg(nd, nd._bind(ps), xd, ps, st, times, B, args.bwd_reps))
    Ws, o = [], 0
    for l in model.layers[1:]:
        n, k = l.out_dims, l.in_dims
        Ws.append((torch.from_numpy(p[o:o + n * k].reshape(k, n).T.copy()).cuda(), torch.from_numpy(p[o + n * k:o + n * k + n]).cuda()))
        o += n * k + n
    eager_solve(Ws, xd, 0.0, 1.0, TOL, maxiters=5)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    ue, ena, enr = eager_solve(Ws, xd, 0.0, 1.0, TOL)
    torch.cuda.synchronize(); eager_ms = (time.perf_counter() - t0) * 1e3
    err = float((ue - r["u"][-1]).abs().max() / r["u"][-1].abs().max())
    print(json.dumps(dict(
        workload="physionet_gen_dynamics", B=B, tol=TOL, naccept=r["stats"]["naccept"], nreject=r["stats"]["nreject"],
        solve_kernel_ms=round(solve_ms, 3), step_launches=launches, launches_per_attempt=round(launches / max(attempts, 1), 3),
        us_per_attempt_solve=round(1e3 * solve_ms / max(attempts, 1), 2),
        layer_forward_ms=round(statistics.median(fwd), 3), layer_forward_pullback_ms=round(statistics.median(fb), 3),
        eager_torch_fp32_solve_ms=round(eager_ms, 2), eager_naccept=ena, eager_nreject=enr, eager_vs_hip_u_end=err,
        adj_host=bool(os.environ.get("LRNDE_ADJ_HOST")), sensealg=args.sensealg, pullback_series4=legs[0], pullback_series49=legs[1])))


if __name__ == "__main__":
    main()
