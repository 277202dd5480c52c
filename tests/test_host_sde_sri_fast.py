"""The one-launch SRI step with the controller on the device (k_sde_sri_fast) — CPU side.

* `lrnde_sde_last_solve_info` is a hook: declared in lrnde_hooks.h, absent from lrnde.h, bound in `_lib.SYMBOLS`.
* NEW_SRI: the pinned SRI cases at the kernel's edges that tests/test_gpu_sde_sri_fast.py adds to the three SRI entries of
  test_host_sde_adaptive.CASES, chosen here with the helper alone (tests/sde_adaptive_np.py on the C oracle) from a scan of
  tol in (0.05 .. 0.8) x dt0 in (0, 0.4).  Every case ends with retcode OK (the helper raises otherwise) and at least three
  accepted steps in all three modes.  As in test_host_sde_adaptive.py, no case of these sizes rejects with the automatic
  initial dt, so the rejecting ones start from a too long first step dt0 = 0.4; (33, 100, 9, 32) keeps the automatic initial dt
  (the device form of it with the SRI step's order 3/2, at odd widths)."""
import os
import re

import numpy as np
import pytest

from test_host_sde_adaptive import MODES, case_id, case_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (D, H, B, nfine): one column | odd widths, padded fragments, scalar loads | the gate's corner, two 112-row segments, partial
# last tile | outside the gate (host-controlled loop)
NEW_SRI = [
    dict(kind="SRI", shape=(2, 4, 1, 64), seed=7, tol=0.14, dt0=0.4, tab=(41, 0.1)),       # 14 accepted, 1 rejected
    dict(kind="SRI", shape=(33, 100, 9, 32), seed=7, tol=0.3, dt0=0.0, tab=(41, 0.1)),     # 27 accepted
    dict(kind="SRI", shape=(64, 128, 17, 32), seed=7, tol=0.2, dt0=0.4, tab=(41, 0.1)),    # 17 accepted, 1 rejected
    dict(kind="SRI", shape=(72, 32, 6, 32), seed=7, tol=0.14, dt0=0.4, tab=(41, 0.1)),     # 17 accepted, 1 rejected
]
IN_GATE = [c for c in NEW_SRI if c["shape"][0] <= 64 and c["shape"][1] <= 128]


def test_last_solve_info_is_a_hook_not_part_of_the_main_header():
    hooks = open(os.path.join(ROOT, "include", "lrnde_hooks.h")).read()
    main = open(os.path.join(ROOT, "include", "lrnde.h")).read()
    assert re.search(r"int\s+lrnde_sde_last_solve_info\s*\(\s*lrnde_sde\s*\*", hooks)
    assert "lrnde_sde_last_solve_info" not in main
    import lrnde_amd  # noqa: F401
    from localregneuralde_jl_amd import _lib as L
    assert "lrnde_sde_last_solve_info" in [s[0] for s in L.SYMBOLS]


@pytest.mark.parametrize("c", NEW_SRI, ids=case_id)
def test_new_sri_cases_end_ok_with_three_accepted_steps_in_every_mode(oracle, c):
    for mode in MODES:
        _, _, r = case_reference(oracle, c, mode)     # (raises on MaxIters / DtLessThanMin / DtNaN)
        assert r["naccept"] >= 3, (mode, r["naccept"])
        assert np.isfinite(r["u"]).all() and (r["reg_val"] > 0) == (mode != "none")
        att = r["naccept"] + r["nreject"]
        init = 0 if c["dt0"] else 2
        loc = 0 if mode == "none" else 1
        assert r["nfe_drift"] == r["nfe_diffusion"] == 4 * (att + loc) + init * (1 + loc)
        assert sum(m for _, m in r["steps"]) == c["shape"][3]     # the accepted steps tile the path's grid
        if c["dt0"]:
            assert r["nreject"] >= 1
        print(f"{case_id(c)} {mode}: accepted {r['naccept']}, rejected {r['nreject']}, dt0 {r['dt0']:.4g}, reg_val {r['reg_val']:.4g}")


def test_the_gate_has_a_case_on_each_side_and_one_that_rejects(oracle):
    assert len(IN_GATE) == 3 and [c["shape"] for c in NEW_SRI if c not in IN_GATE] == [(72, 32, 6, 32)]
    assert max(case_reference(oracle, c, "none")[2]["nreject"] for c in IN_GATE) >= 1
