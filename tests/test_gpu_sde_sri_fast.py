"""The adaptive SRI solve as one launch per attempted step with the controller on the device (k_sde_sri_fast,
csrc/lrnde_sde_sri_fast.hip), through the C ABI.

* the same bits on three routes: the fused kernel under the device controller (default), the host-controlled loop on
  lrnde_sde_sri_step (LRNDE_SDE_HOST_LOOP=1, the route every SRI solve took before), and lrnde_sde_sri_step fed the recorded
  (i, m) steps one by one — every accepted state, reg_val, the counters, and the plain solve's trace row by row;
* forward == tests/sde_adaptive_np.py (the oracle's loop) bit for bit at the kernel's edges (tests/test_host_sde_sri_fast.py
  pins the cases): one column, odd widths with padded fragments and scalar loads, the gate's corner;
* `SdeHandle.last_solve_info()` says which loop ran, how many step launches it enqueued and how often the host waited;
* the main solve's automatic initial dt on the device (Milstein: order 1, SRI: order 3/2) == the host form;
* the pullback from a record the fused kernel wrote == the pullback from the host loop's record."""
import numpy as np
import pytest
import torch

import sde_adaptive_np as S
from test_gpu_sde_adaptive_alg import MIL, SRI, S_FIELDS, _check_forward, _forward, _handle
from test_host_sde_adaptive import MODES, case_id, case_reference
from test_host_sde_sri_fast import IN_GATE, NEW_SRI

pytestmark = pytest.mark.gpu
f32 = np.float32
CORNER = next(c for c in NEW_SRI if c["shape"] == (64, 128, 17, 32))
OUTSIDE = next(c for c in NEW_SRI if c["shape"] == (72, 32, 6, 32))
STAT_KEYS = ("retcode", "naccept", "nreject", "nf", "iters")


def _dev(a):
    return None if a is None else torch.from_numpy(a).cuda()


def _with_option(P, name, fn):
    P.set_option(name, 1)
    try:
        return fn()
    finally:
        P.set_option(name, 0)


def _plain(h, c, inp, T, dt0, solver=None):
    solver = solver or c["kind"]
    kw = dict(tableau=[T[k] for k in S_FIELDS()], path_z=_dev(inp["Z"])) if solver == "SRI" else {}
    return h.solve_adaptive(_dev(inp["x"]), _dev(inp["W"]), 0.0, 1.0, c["tol"], c["tol"], dt0=dt0, solver=solver, **kw)


@pytest.mark.parametrize("c", [SRI[2], CORNER], ids=case_id)
def test_sri_same_bits_on_all_three_routes(oracle, gpu_pkg, c):
    assert c["shape"] in ((32, 64, 24, 64), (64, 128, 17, 32)) and c["dt0"]
    inp, T, ref = case_reference(oracle, c, "biased")      # :biased with saveat = (): the series is every accepted step's end state
    assert ref["nreject"] >= 1
    h = _handle(gpu_pkg, c, inp)
    fused = _forward(h, c, inp, T, "biased")
    assert h.last_solve_info()["kind"] == 1
    host = _with_option(gpu_pkg, "LRNDE_SDE_HOST_LOOP", lambda: (_forward(h, c, inp, T, "biased"), h.last_solve_info()))
    assert host[1]["kind"] == 0
    host = host[0]
    _check_forward(fused, ref, "fused")
    _check_forward(host, ref, "host loop")
    assert torch.equal(fused["u"], host["u"]) and fused["reg_val"] == host["reg_val"]
    assert all(fused["stats"][k] == host["stats"][k] for k in STAT_KEYS), (fused["stats"], host["stats"])
    nfine = c["shape"][3]
    hh = f32(f32(1.0) / f32(nfine))
    W, Z = _dev(inp["W"]), _dev(inp["Z"])
    u = _dev(inp["x"])
    tab = [T[k] for k in S_FIELDS()]
    assert len(ref["steps"]) + 1 == fused["u"].shape[0]
    for k, (i, m) in enumerate(ref["steps"]):
        r = h.sri_step(tab, u, (W[i + m] - W[i]).contiguous(), (Z[i + m] - Z[i]).contiguous(), f32(f32(i) * hh), f32(f32(m) * hh),
                       c["tol"], c["tol"], 1.0 / 6.0)
        u = r["u"]
        assert torch.equal(u, fused["u"][k + 1]), k
    # the plain solve's trace: (t, dt, EEst, accepted) of every attempt.  EEst is an fp64 sum of fp32 squares rounded once to
    # fp32; the two routes add the same squares in different orders, which moves the fp32 result only if the sum lies within
    # about n 2^-53 (relative) of a rounding boundary
    a = _plain(h, c, inp, T, c["dt0"])
    b = _with_option(gpu_pkg, "LRNDE_SDE_HOST_LOOP", lambda: _plain(h, c, inp, T, c["dt0"]))
    assert len(a["trace"]) == ref["naccept"] + ref["nreject"]
    for k in ("t", "dt", "eest", "accepted"):
        assert np.array_equal(a["trace"][k], b["trace"][k]), (k, a["trace"][k], b["trace"][k])
    assert torch.equal(a["u_end"], b["u_end"]) and torch.equal(a["u_end"], fused["u"][-1])
    assert all(a["stats"][k] == b["stats"][k] for k in STAT_KEYS)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", IN_GATE, ids=case_id)
def test_sri_forward_equals_the_helper_at_the_kernels_edges(oracle, gpu_pkg, c, mode):
    inp, T, ref = case_reference(oracle, c, mode)
    h = _handle(gpu_pkg, c, inp)
    got = _forward(h, c, inp, T, mode)
    _check_forward(got, ref, f"{case_id(c)} {mode}")
    assert got["stats"]["nf"] == 4 * (ref["naccept"] + ref["nreject"])
    assert h.last_solve_info()["kind"] == 1
    print(f"{case_id(c)} {mode}: accepted {ref['naccept']}, rejected {ref['nreject']}, series {len(ref['t'])}, reg_val {ref['reg_val']:.4g}")


def test_last_solve_info_says_what_ran(oracle, gpu_pkg):
    c = SRI[2]
    inp, T, ref = case_reference(oracle, c, "none")
    att = ref["naccept"] + ref["nreject"]
    h = _handle(gpu_pkg, c, inp)
    r = _plain(h, c, inp, T, c["dt0"])
    assert r["stats"]["naccept"] == ref["naccept"] and r["stats"]["nreject"] == ref["nreject"]
    info = h.last_solve_info()
    assert info["kind"] == 1 and info["host_waits"] == 1 and info["launches"] >= att, info
    _with_option(gpu_pkg, "LRNDE_SDE_HOST_LOOP", lambda: _plain(h, c, inp, T, c["dt0"]))
    info = h.last_solve_info()
    assert info["kind"] == 0 and info["host_waits"] >= att and info["launches"] == att, info
    # outside the gate: the host-controlled loop
    inp, T, ref = case_reference(oracle, OUTSIDE, "none")
    ho = _handle(gpu_pkg, OUTSIDE, inp)
    r = _plain(ho, OUTSIDE, inp, T, OUTSIDE["dt0"])
    assert np.array_equal(r["u_end"].cpu().numpy(), ref["u"][-1])
    info = ho.last_solve_info()
    assert info["kind"] == 0 and info["host_waits"] >= ref["naccept"] + ref["nreject"], info
    # Euler-Heun at config-5 widths (persistent launch, or a launch per attempt), Milstein (a launch per attempt)
    inp = S.case_inputs(32, 64, 40, 256, 7)
    he = _handle(gpu_pkg, dict(shape=(32, 64, 40, 256)), inp)
    r = he.solve_adaptive(_dev(inp["x"]), _dev(inp["W"]), 0.0, 1.0, 0.02, 0.02)
    info = he.last_solve_info()
    assert info["kind"] in (1, 2) and info["host_waits"] == 1 and info["launches"] >= 1, info
    inp, T, ref = case_reference(oracle, MIL[0], "none")
    hm = _handle(gpu_pkg, MIL[0], inp)
    r = _plain(hm, MIL[0], inp, None, float(ref["dt0"]))
    info = hm.last_solve_info()
    assert info["kind"] == 1 and info["host_waits"] == 1 and info["launches"] >= r["stats"]["naccept"] + r["stats"]["nreject"], info


@pytest.mark.parametrize("c", [MIL[0], SRI[0]], ids=case_id)
def test_main_solve_initial_dt_on_the_device_equals_the_host_form(oracle, gpu_pkg, c):
    assert c["dt0"] == 0.0 and c["shape"][:2] == (32, 64)
    inp, T, ref = case_reference(oracle, c, "unbiased")
    h = _handle(gpu_pkg, c, inp)
    dev = _forward(h, c, inp, T, "unbiased")
    info = h.last_solve_info()
    assert info["kind"] == 1 and info["host_waits"] == 1, info      # no wait for the initial dt: the solve's closing one alone
    host, hinfo = _with_option(gpu_pkg, "LRNDE_SDE_HOST_INITDT", lambda: (_forward(h, c, inp, T, "unbiased"), h.last_solve_info()))
    assert hinfo["kind"] == 1 and hinfo["host_waits"] == 3, hinfo   # the host form's two synchronisations
    assert np.array_equal(dev["t"], host["t"]) and torch.equal(dev["u"], host["u"]) and dev["reg_val"] == host["reg_val"]
    assert dev["stats"] == host["stats"], (dev["stats"], host["stats"])
    assert dev["nfe_drift"] == host["nfe_drift"] and dev["nfe_diffusion"] == host["nfe_diffusion"] and dev["t1"] == host["t1"]
    _check_forward(dev, ref, case_id(c))


@pytest.mark.parametrize("saveat", [(0.3, 0.77, 1.0), ()], ids=["saveat", "default"])
def test_pullback_from_a_fused_kernel_record(oracle, gpu_pkg, saveat):
    """the record is the same bits on both routes, so the reverse sweep over it is too"""
    c = SRI[1]
    inp, T, ref = case_reference(oracle, c, "unbiased", saveat=saveat, t1_or_rand=0.37)
    D, H, B, nfine = c["shape"]
    du = _dev(np.random.default_rng(5).standard_normal((len(ref["t"]), B, D)).astype(f32))
    h = _handle(gpu_pkg, c, inp)
    fwd = lambda: _forward(h, c, inp, T, "unbiased", saveat=saveat, t1_or_rand=0.37)
    got = fwd()
    assert h.last_solve_info()["kind"] == 1
    _check_forward(got, ref, f"{case_id(c)} {saveat}")
    a = h.node_backward_recorded(du, w_reg=2.0)
    hh = _handle(gpu_pkg, c, inp)
    fwd = lambda: _forward(hh, c, inp, T, "unbiased", saveat=saveat, t1_or_rand=0.37)
    host = _with_option(gpu_pkg, "LRNDE_SDE_HOST_LOOP", fwd)
    assert hh.last_solve_info()["kind"] == 0
    assert torch.equal(got["u"], host["u"]) and got["reg_val"] == host["reg_val"]
    b = hh.node_backward_recorded(du, w_reg=2.0)
    for k in ("dx", "dp_drift", "dp_diff"):
        assert torch.isfinite(a[k]).all() and (a[k] != 0).any(), k
        assert torch.equal(a[k], b[k]), (k, float((a[k] - b[k]).abs().max()))
