"""Host side of the chain handle's device-controlled adjoint: the hook's declaration, the documented info key, and the
error of the float64 yardstick tests/test_gpu_chain_adjoint.py holds the 49-time series to.  No GPU needed."""
import inspect
import os
import re

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_last_adjoint_info_is_a_hook_not_part_of_the_main_header():
    hooks = open(os.path.join(ROOT, "include", "lrnde_hooks.h")).read()
    main = open(os.path.join(ROOT, "include", "lrnde.h")).read()
    assert re.search(r"int\s+lrnde_last_adjoint_info\s*\(\s*lrnde_ctx\s*\*", hooks)
    assert "lrnde_last_adjoint_info" not in main
    import lrnde_amd  # noqa: F401
    from localregneuralde_jl_amd import _lib as L
    assert "lrnde_last_adjoint_info" in [s[0] for s in L.SYMBOLS]


def test_pullback_documents_the_adjoint_loop_key():
    import lrnde_amd as P
    doc = inspect.getdoc(P.NeuralODE.pullback)
    assert "info['adjoint_loop']" in doc
    for name in ('"host"', '"device"', '"chain_device"'):
        assert name in doc
    from localregneuralde_jl_amd.layers import Handle
    assert Handle.ADJOINT_LOOPS == ("host", "device", "chain_device") and callable(Handle.last_adjoint_info)


def test_chain_adjoint_kernel_args_are_value_initialised():
    src = open(os.path.join(ROOT, "localregneuralde.jl_amd", "csrc", "lrnde_kernels.hip")).read()
    for decl in ("ChAdjArgs a{};", "ChAdjBegin b{};"):
        assert decl in src


def test_float64_yardstick_of_the_49_time_series_agrees_with_itself():
    """RK4 with 196 and with 245 steps (both divisible by 49): the two float64 gradients agree to well under the 3e-4 the
    GPU results are held to, so the yardstick's own error does not eat the bound"""
    import lrnde_amd as P
    ACT = torch.tanh
    model = P.Chain(P.Activation("tanh"), *[P.Dense(20, 40, "tanh") if i % 2 == 0 else P.Dense(40, 20, "tanh") for i in range(8)])
    B = 12
    p = P.glorot_chain_params(model, seed=0, scale=1.5)
    p = (p + np.random.default_rng(1).standard_normal(p.size).astype(np.float32) * np.float32(0.01)).astype(np.float32)
    x = (np.random.default_rng(2).random((B, 20), dtype=np.float32) - np.float32(0.5)) * np.float32(2)
    times = [(i + 1) / 49.0 for i in range(49)]
    cots = np.random.default_rng(13).standard_normal((49, B, 20)).astype(np.float32)

    def grads(nsteps):
        pt = torch.tensor(p, dtype=torch.float64, requires_grad=True)
        xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
        Wb, o = [], 0
        for l in model.layers[1:]:
            i, n = l.in_dims, l.out_dims
            Wb.append((pt[o:o + n * i].reshape(i, n).T, pt[o + n * i:o + n * i + n]))
            o += n * i + n

        def f(u):
            h = ACT(u)
            for W, b in Wb:
                h = ACT(h @ W.T + b)
            return h
        h, u, loss = 1.0 / nsteps, xt, 0.0
        marks = {int(round(t * nsteps)): i for i, t in enumerate(times)}
        assert len(marks) == 49
        for k in range(nsteps):
            k1 = f(u); k2 = f(u + 0.5 * h * k1); k3 = f(u + 0.5 * h * k2); k4 = f(u + h * k3)
            u = u + (h / 6.0) * (k1 + 2 * k2 + 2 * k3 + k4)
            if k + 1 in marks:
                loss = loss + (u * torch.tensor(cots[marks[k + 1]], dtype=torch.float64)).sum()
        loss.backward()
        return xt.grad.numpy(), pt.grad.numpy()

    (gx1, gp1), (gx2, gp2) = grads(196), grads(245)
    rel = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))
    print(f"RK4 196 vs 245 steps: dx {rel(gx1, gx2):.2e} dp {rel(gp1, gp2):.2e}")
    assert rel(gx1, gx2) < 3e-6 and rel(gp1, gp2) < 3e-6
