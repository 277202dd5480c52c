"""The one-launch Euler-Heun step with the controller on the device (k_sde_eh_fast) at the edges of its workgroup frame — CPU side.

* EH_CASES: the pinned Euler-Heun cases of tests/test_gpu_sde_eh_fast.py in the format of test_host_sde_adaptive.CASES, chosen
  here with the helper alone (tests/sde_adaptive_np.py on the C oracle).  The shapes are those at which the Milstein and SRI
  kernels are already held to equal bits: one column | odd widths (D % 4 != 0: scalar loads, padded fragments) | the gate's
  corner (H = 128: two 112-row segments; a partial last column tile) | outside the gate.  Every case ends with retcode OK (the
  helper raises otherwise), at least three accepted steps that tile the path's grid, in all three modes; the cases that start
  from a too long first step dt0 = 0.4 reject at least once, and (33, 100, 9, 32) at tol 0.3 keeps the automatic initial dt
  (its device form at odd widths)."""
import numpy as np
import pytest

from test_host_sde_adaptive import MODES, case_id, case_reference

# accepted / rejected steps are the same in all three modes
EH_CASES = [
    dict(kind="EulerHeun", shape=(2, 4, 1, 64), seed=7, tol=0.14, dt0=0.4),       # 10 accepted, 4 rejected
    dict(kind="EulerHeun", shape=(33, 100, 9, 32), seed=7, tol=0.05, dt0=0.4),    # 27 accepted, 1 rejected
    dict(kind="EulerHeun", shape=(33, 100, 9, 32), seed=7, tol=0.3, dt0=0.0),     # 23 accepted
    dict(kind="EulerHeun", shape=(64, 128, 17, 32), seed=7, tol=0.05, dt0=0.4),   # 32 accepted, 2 rejected
    dict(kind="EulerHeun", shape=(72, 32, 6, 32), seed=7, tol=0.05, dt0=0.4),     # 32 accepted, 2 rejected; outside the gate
]
EH_IN_GATE = [c for c in EH_CASES if c["shape"][0] <= 64 and c["shape"][1] <= 128]
COUNTS = [(10, 4), (27, 1), (23, 0), (32, 2), (32, 2)]


@pytest.mark.parametrize("c,counts", list(zip(EH_CASES, COUNTS)), ids=[case_id(c) for c in EH_CASES])
def test_euler_heun_cases_end_ok_with_three_accepted_steps_in_every_mode(oracle, c, counts):
    for mode in MODES:
        _, _, r = case_reference(oracle, c, mode)     # (raises on MaxIters / DtLessThanMin / DtNaN)
        assert r["naccept"] >= 3, (mode, r["naccept"])
        assert np.isfinite(r["u"]).all() and (r["reg_val"] > 0) == (mode != "none")
        assert sum(m for _, m in r["steps"]) == c["shape"][3]     # the accepted steps tile the path's grid
        if c["dt0"]:
            assert r["nreject"] >= 1
        assert (r["naccept"], r["nreject"]) == counts, (mode, r["naccept"], r["nreject"])
        print(f"{case_id(c)} {mode}: accepted {r['naccept']}, rejected {r['nreject']}, dt0 {r['dt0']:.4g}, reg_val {r['reg_val']:.4g}")


def test_the_gate_has_euler_heun_cases_on_each_side():
    assert len(EH_IN_GATE) == 4 and [c["shape"] for c in EH_CASES if c not in EH_IN_GATE] == [(72, 32, 6, 32)]
    assert any(c["shape"][0] % 4 for c in EH_IN_GATE) and any(c["shape"][1] == 128 for c in EH_IN_GATE) and any(c["shape"][2] == 1 for c in EH_IN_GATE)
