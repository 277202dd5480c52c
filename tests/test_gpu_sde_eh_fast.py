"""The one-launch Euler-Heun kernel (k_sde_eh_fast) at the edges of its workgroup frame: one column, D % 4 != 0 (scalar loads,
padded fragments), H = 128 (two 112-row segments), a partial last column tile.

* routes: `lrnde_sde_node_forward_record` == tests/sde_adaptive_np.py BIT FOR BIT on the persistent launch (the default), on a
  launch per attempted step (LRNDE_SDE_NO_PERSIST=1: the controller in the step's shared footer) and on the host-controlled
  loop (LRNDE_SDE_HOST_LOOP=1), for every in-gate case of test_host_sde_eh_fast.EH_CASES in all three modes; the three routes
  equal each other in u, reg_val and the solve's stats.  Outside the gate the host-controlled loop runs.
* trace: the plain solve's (t, dt, EEst, accepted) of every attempt is the same on the persistent launch and the launch per step.
* single steps and march mode: `euler_heun_step` == the oracle's step in u, EEst and reg_val; `solve_fixed` of 5 steps (one
  marching launch, and a launch per step under LRNDE_SDE_NO_MARCH=1) == the loop of single-step calls."""
import numpy as np
import pytest
import torch

import sde_adaptive_np as S
from test_gpu_sde_adaptive_alg import _check_forward, _forward, _handle
from test_host_sde_adaptive import MODES, case_id, case_reference
from test_host_sde_eh_fast import EH_CASES, EH_IN_GATE

pytestmark = pytest.mark.gpu
f32 = np.float32
STAT_KEYS = ("retcode", "naccept", "nreject", "nf", "iters")
ROUTES = ((None, 2), ("LRNDE_SDE_NO_PERSIST", 1), ("LRNDE_SDE_HOST_LOOP", 0))     # (option, last_solve_info()["kind"])


def _dev(a):
    return torch.from_numpy(a).cuda()


def _with_option(P, name, fn):
    if name is None:
        return fn()
    P.set_option(name, 1)
    try:
        return fn()
    finally:
        P.set_option(name, 0)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", EH_IN_GATE, ids=case_id)
def test_euler_heun_same_bits_on_all_three_routes(oracle, gpu_pkg, c, mode):
    inp, T, ref = case_reference(oracle, c, mode)
    h = _handle(gpu_pkg, c, inp)
    got = []
    for opt, kind in ROUTES:
        r, info = _with_option(gpu_pkg, opt, lambda: (_forward(h, c, inp, T, mode), h.last_solve_info()))
        assert info["kind"] == kind, (opt, info)
        _check_forward(r, ref, f"{case_id(c)} {mode} {opt}")
        assert r["stats"]["nf"] == 3 * (ref["naccept"] + ref["nreject"])      # three drift evaluations per attempted step
        got.append(r)
    for r in got[1:]:
        assert torch.equal(got[0]["u"], r["u"]) and got[0]["reg_val"] == r["reg_val"]
        assert all(got[0]["stats"][k] == r["stats"][k] for k in STAT_KEYS), (got[0]["stats"], r["stats"])
    print(f"{case_id(c)} {mode}: accepted {ref['naccept']}, rejected {ref['nreject']}, series {len(ref['t'])}, reg_val {ref['reg_val']:.4g}")


def test_euler_heun_outside_the_gate_takes_the_host_loop(oracle, gpu_pkg):
    c = EH_CASES[-1]
    assert c["shape"] == (72, 32, 6, 32)
    inp, T, ref = case_reference(oracle, c, "unbiased")
    h = _handle(gpu_pkg, c, inp)
    got = _forward(h, c, inp, T, "unbiased")
    assert h.last_solve_info()["kind"] == 0
    _check_forward(got, ref, case_id(c))


@pytest.mark.parametrize("c", [EH_CASES[1], EH_CASES[3]], ids=case_id)
def test_euler_heun_trace_is_the_same_on_the_persistent_launch_and_the_launch_per_step(oracle, gpu_pkg, c):
    assert c["shape"] in ((33, 100, 9, 32), (64, 128, 17, 32)) and c["dt0"] == 0.4
    inp, _, ref = case_reference(oracle, c, "none")
    h = _handle(gpu_pkg, c, inp)
    solve = lambda: (h.solve_adaptive(_dev(inp["x"]), _dev(inp["W"]), 0.0, 1.0, c["tol"], c["tol"], dt0=c["dt0"]), h.last_solve_info())
    a, ia = solve()
    b, ib = _with_option(gpu_pkg, "LRNDE_SDE_NO_PERSIST", solve)
    assert ia["kind"] == 2 and ib["kind"] == 1, (ia, ib)
    assert len(a["trace"]) == ref["naccept"] + ref["nreject"] and int(a["trace"]["accepted"].sum()) == ref["naccept"]
    for k in ("t", "dt", "eest", "accepted"):
        assert np.array_equal(a["trace"][k], b["trace"][k]), (k, a["trace"][k], b["trace"][k])
    assert torch.equal(a["u_end"], b["u_end"]) and np.array_equal(a["u_end"].cpu().numpy(), ref["u"][-1])
    assert all(a["stats"][k] == b["stats"][k] for k in STAT_KEYS), (a["stats"], b["stats"])


@pytest.mark.parametrize("D,H,B", [(33, 100, 9), (64, 128, 17)])
def test_euler_heun_single_steps_and_march_mode(oracle, gpu_pkg, D, H, B):
    n, tol, delta = 5, 0.14, 1.0 / 6.0
    inp = S.case_inputs(D, H, B, n, 7)
    drift, diff = S.oracle_fields(oracle, D, H, inp["pd"], inp["pg"])
    h = _handle(gpu_pkg, dict(shape=(D, H, B, n)), inp)
    t0, dt = f32(0.1), f32(0.05)
    dW = (np.random.default_rng(13).standard_normal((n, B, D)) * np.sqrt(dt)).astype(f32)
    ud, dWd = _dev(inp["x"]), _dev(dW)
    march = h.solve_fixed(ud, dWd, t0, dt, tol, tol, delta)
    loop = _with_option(gpu_pkg, "LRNDE_SDE_NO_MARCH", lambda: h.solve_fixed(ud, dWd, t0, dt, tol, tol, delta))
    u, uo = ud, inp["x"]
    for i in range(n):
        t = f32(t0 + f32(i) * dt)
        r = h.euler_heun_step(u, dWd[i].contiguous(), t, dt, tol, tol, delta)
        ro = oracle.euler_heun_step(drift, diff, uo, dW[i], t, dt, tol, tol, delta)
        assert np.array_equal(r["u"].cpu().numpy(), ro["u"]), i
        assert r["eest"] == ro["eest"] and r["reg_val"] == ro["reg_val"], (i, r["eest"], ro["eest"])
        for tr in (march, loop):
            assert torch.equal(tr["u"][i], r["u"]), i
            assert tr["eest"][i] == r["eest"] and tr["reg_val"][i] == r["reg_val"], i
        u, uo = r["u"], ro["u"]
