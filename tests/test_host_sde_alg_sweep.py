"""The one-launch reverse sweep of Milstein / SRI records — CPU side (the GPU side: tests/test_gpu_sde_alg_sweep.py).

* the cases the GPU suite adds (the diffusion without a bias at 12 x 20) are pinned like tests/test_host_sde_adaptive.py::CASES:
  every form ends OK with at least three accepted steps; the forms with `saveat` do produce interpolated entries and a saved
  start value;
* the float64 reference the GPU gradients are held to REACTS to what the sweep must get right — a wrong (i, m) for one step,
  dZ swapped for dW, a series cotangent put wholly on one step end — by far more than the GPU suite's bound of 5e-6 of each
  gradient's norm (the factors are printed): those bounds cannot pass vacuously;
* the sweep's gate restated in Python says what the issue's shapes need; the new hook is a hook."""
import os
import re

import numpy as np
import pytest

import sde_alg_sweep_cases as AC
from sde_alg_sweep_cases import FORMS, GATE_CORNER, MIL, NOBIAS, SRI, SWEEP_CASES, cid

BOUND = 5e-6
FAR = 100.0          # "far more": at least a hundred times the bound
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("c", NOBIAS, ids=cid)
def test_the_cases_without_a_diffusion_bias_end_ok_with_three_accepted_steps_in_every_form(oracle, c):
    D = c["shape"][0]
    for form in FORMS:
        inp, T, r = AC.reference(oracle, c, form)       # (raises on MaxIters / DtLessThanMin / DtNaN)
        assert inp["pg"].size == D * D
        assert r["naccept"] >= 3 and np.isfinite(r["u"]).all() and (r["reg_val"] > 0) == (FORMS[form]["mode"] != "none")
        print(f"{cid(c)} {form}: accepted {r['naccept']}, rejected {r['nreject']}, series {len(r['t'])}, reg_val {r['reg_val']:.4g}")


@pytest.mark.parametrize("c", [MIL[0], SRI[1]], ids=cid)
def test_the_saveat_forms_have_interpolated_entries_and_a_saved_start(oracle, c):
    _, _, r = AC.reference(oracle, c, "saveat-interpolated")
    assert any(0.0 < float(th) < 1.0 for (_, k, th) in r["series"])
    _, _, r = AC.reference(oracle, c, "saveat-with-start")
    assert r["series"][0][1] < 0 and any(k >= 0 for (_, k, th) in r["series"])


def _moved(steps):
    """the recorded steps with the boundary between two neighbouring steps moved by one grid interval: one wrong (i, m) pair
    on each side, the grid still tiled"""
    s = list(steps)
    for j in range(len(s) - 1):
        (i0, m0), (i1, m1) = s[j], s[j + 1]
        if m1 > 1:
            s[j], s[j + 1] = (i0, m0 + 1), (i1 + 1, m1 - 1)
            return s
        if m0 > 1:
            s[j], s[j + 1] = (i0, m0 - 1), (i1 - 1, m1 + 1)
            return s
    raise AssertionError("every recorded step is one grid interval long")


def _factors(base, other):
    return {k: AC._rel(o, b) / BOUND for k, b, o in zip(("dx", "dp_drift", "dp_diff"), base, other)}


@pytest.mark.parametrize("c", SWEEP_CASES + [GATE_CORNER] + NOBIAS, ids=cid)
def test_a_wrong_step_moves_every_gradient_far_beyond_the_bound(oracle, c):
    form = "unbiased-w2"
    inp, T, ref = AC.reference(oracle, c, form)
    du = AC.cotangents(c, ref, form)
    base = AC.autograd64(c, inp, T, ref, du, 2.0)
    fac = _factors(base, AC.autograd64(c, inp, T, ref, du, 2.0, steps=_moved(ref["steps"])))
    print(f"{cid(c)}: one step boundary moved by a grid interval: " + ", ".join(f"{k} x{v:.3g} of the bound" for k, v in fac.items()))
    assert all(v > FAR for v in fac.values()), fac


@pytest.mark.parametrize("c", SRI + [NOBIAS[1]], ids=cid)
def test_dz_swapped_for_dw_moves_every_gradient_far_beyond_the_bound(oracle, c):
    form = "unbiased-w2"
    inp, T, ref = AC.reference(oracle, c, form)
    du = AC.cotangents(c, ref, form)
    base = AC.autograd64(c, inp, T, ref, du, 2.0)
    fac = _factors(base, AC.autograd64(c, inp, T, ref, du, 2.0, swap_dz=True))
    print(f"{cid(c)}: dZ := dW: " + ", ".join(f"{k} x{v:.3g} of the bound" for k, v in fac.items()))
    assert all(v > FAR for v in fac.values()), fac


@pytest.mark.parametrize("end", [0, 1])
@pytest.mark.parametrize("c", [MIL[0], MIL[2], SRI[0], SRI[1]], ids=cid)
def test_a_series_cotangent_on_one_step_end_moves_every_gradient_far_beyond_the_bound(oracle, c, end):
    form = "saveat-interpolated"
    inp, T, ref = AC.reference(oracle, c, form)
    du = AC.cotangents(c, ref, form)
    base = AC.autograd64(c, inp, T, ref, du, 2.0)
    fac = _factors(base, AC.autograd64(c, inp, T, ref, du, 2.0, series_end=end))
    print(f"{cid(c)}: interpolated values taken wholly at the step's {'end' if end else 'start'}: " +
          ", ".join(f"{k} x{v:.3g} of the bound" for k, v in fac.items()))
    assert all(v > FAR for v in fac.values()), fac


def test_the_gate_on_the_cpu_side():
    for c in SWEEP_CASES + NOBIAS:
        assert AC.sweep_gate(*c["shape"][:2], c["kind"]), cid(c)
    assert not AC.sweep_gate(72, 32, "RKMil")                      # D > 64: outside the one-launch kernels' shape
    # (64, 128): the weights alone take 98 KB and the workgroup's cotangent 83 KB
    assert AC.sweep_lds_bytes(64, 128, "RKMil") > AC.LDS_LIMIT and not AC.sweep_gate(*GATE_CORNER["shape"][:2], "RKMil")
    assert AC.sweep_lds_bytes(32, 64, "RKMil") < AC.sweep_lds_bytes(32, 64, "SRI") < 64 * 1024
    assert not AC.sweep_gate(32, 64, "SRI", nseries=AC.SBF_MAXSER + 1)


def test_last_backward_info_is_a_hook_not_part_of_the_main_header():
    hooks = open(os.path.join(ROOT, "include", "lrnde_hooks.h")).read()
    main = open(os.path.join(ROOT, "include", "lrnde.h")).read()
    assert re.search(r"int\s+lrnde_sde_last_backward_info\s*\(\s*lrnde_sde\s*\*", hooks)
    assert "lrnde_sde_last_backward_info" not in main
    import lrnde_amd  # noqa: F401
    from localregneuralde_jl_amd import _lib as L
    assert "lrnde_sde_last_backward_info" in [s[0] for s in L.SYMBOLS]
