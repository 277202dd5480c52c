"""NeuralDSDE mirror (src/layers/neural_sde.jl) on the liblrnde SDE entry points.

The layer runs what the reference's runs (src/layers/neural_sde.jl:50-123): an ADAPTIVE solve — the step of the layer's solver
under a PI controller on its error estimate, on a Brownian path drawn up front on a uniform grid
(`lrnde_sde_node_forward_record_alg`) — the local step of the same kind at (sol(t1), t1) for reg_val, user `saveat` with the
`_CorrectedDESolution` filter, and the pullback as the reverse sweep over the recorded accepted steps
(`lrnde_sde_node_backward_recorded`).  The step is the Lamba Euler-Heun step (`_perform_step(::LambaEulerHeunConstantCache)`,
src/perform_step.jl:172-206; the default, adaptive unless told otherwise), the Milstein step (:108-170) or the four-stage SRI
step (:49-106); the last two are adaptive with `adaptive=True` and march the fixed grid of rounds 1-2 otherwise
(`adaptive=False` gives Euler-Heun that grid too).  The controller runs on the device for all three steps at the one-launch
kernels' shape (D <= 64, H <= 128, no time input, unsharded: one launch per attempted step, one stream sync per solve); outside
that shape Milstein and SRI are host-controlled (one stream sync per attempted step).  `SdeHandle.last_solve_info()` says
which loop ran.  The pullback sweeps the record newest-first in ONE launch for all three steps at that shape (Milstein and SRI:
csrc/lrnde_sde_bwd_alg_fused.hpp) and with launch sequences per recorded step outside it; `SdeHandle.last_backward_info()`
says which.  SOSRI's tableau and its RSWM noise process live in un-vendored StochasticDiffEq and are not restated:
`solver="SOSRI"` raises, `solver="SRI"` takes the tableau from the caller.
"""
import copy
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from .layers import (Chain, Dense, ODESolution, _check_valid_regularize, _dev_ptr, _mlp_desc, _sym)


WHICH = {"EulerHeun": 0, "RKMil": 1, "SRI": 2}   # the step kinds of the `_alg` entry points (include/lrnde.h)


def _which(solver):
    if solver in ("SRI", "FourStageSRI"):
        return 2
    if solver in ("EulerHeun", "LambaEulerHeun"):
        return 0
    if solver.startswith("RKMil"):
        return 1
    raise ValueError(f"solver {solver!r}: EulerHeun, RKMil or SRI")


def _sri_tab(tableau):
    if isinstance(tableau, L.SriTableau):
        return tableau
    return L.SriTableau(*[float(tableau[k]) for k in L.SRI_FIELDS]) if isinstance(tableau, dict) else L.SriTableau(*[float(v) for v in tableau])


class SdeHandle:
    def __init__(self, drift_desc, diffusion_bias=True, device=None, stream=None):
        if not torch.cuda.is_available():
            raise RuntimeError("liblrnde needs a GPU (gfx950); there is no CPU fallback")
        self.D = drift_desc.state_dim
        self.device = torch.cuda.current_device() if device is None else int(device)
        self._stream = torch.cuda.current_stream(self.device) if stream is None else stream
        self._h = C.c_void_p()
        rc = L.lib.lrnde_sde_create(C.byref(self._h), C.byref(drift_desc), int(bool(diffusion_bias)), self.device,
                                    C.c_void_p(self._stream.cuda_stream))
        if rc != 0:
            raise L.LrndeError(rc, "lrnde_sde_create failed")
        self._keep = None

    def close(self):
        if getattr(self, "_h", None):
            L.lib.lrnde_sde_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            msg = L.lib.lrnde_sde_last_error(self._h)
            raise L.LrndeError(rc, msg.decode() if msg else "")

    def set_params(self, p_drift, p_diffusion):
        dev = f"cuda:{self.device}"
        pd = torch.as_tensor(p_drift, dtype=torch.float32).to(dev).contiguous().reshape(-1)
        pg = torch.as_tensor(p_diffusion, dtype=torch.float32).to(dev).contiguous().reshape(-1)
        self._keep = (pd, pg)
        self._chk(L.lib.lrnde_sde_set_params(self._h, C.c_void_p(pd.data_ptr()), pd.numel(),
                                             C.c_void_p(pg.data_ptr()), pg.numel()))

    def euler_heun_step(self, uprev, dW, t, dt, abstol, reltol, delta):
        B = uprev.numel() // self.D
        u = torch.empty_like(uprev)
        ee, rv = C.c_float(), C.c_float()
        self._chk(L.lib.lrnde_sde_euler_heun_step(self._h, _dev_ptr(uprev, "uprev", self.D), _dev_ptr(dW, "dW", self.D),
                                                  B, float(t), float(dt), float(abstol), float(reltol), float(delta),
                                                  _dev_ptr(u, "u"), C.byref(ee), C.byref(rv)))
        return dict(u=u, eest=np.float32(ee.value), reg_val=np.float32(rv.value))

    def rkmil_step(self, uprev, dW, t, dt, abstol, reltol):
        """`_perform_step(integrator, ::RKMilCommuteConstantCache, p)` (src/perform_step.jl:108-170), diagonal noise, Ito."""
        B = uprev.numel() // self.D
        u = torch.empty_like(uprev)
        ee, rv = C.c_float(), C.c_float()
        self._chk(L.lib.lrnde_sde_rkmil_step(self._h, _dev_ptr(uprev, "uprev", self.D), _dev_ptr(dW, "dW", self.D), B,
                                             float(t), float(dt), float(abstol), float(reltol), _dev_ptr(u, "u"),
                                             C.byref(ee), C.byref(rv)))
        return dict(u=u, eest=np.float32(ee.value), reg_val=np.float32(rv.value))


    def sri_step(self, tableau, uprev, dW, dZ, t, dt, abstol, reltol, delta):
        """`_perform_step(integrator, ::FourStageSRIConstantCache, p)` (src/perform_step.jl:49-106), diagonal noise;
        tableau: dict / sequence with the 51 coefficients named as the reference unpacks them (L.SRI_FIELDS) — SOSRI's
        values live in StochasticDiffEq and are the caller's to supply."""
        tab = L.SriTableau(*[float(tableau[k]) for k in L.SRI_FIELDS]) if isinstance(tableau, dict) else L.SriTableau(*[float(v) for v in tableau])
        B = uprev.numel() // self.D
        u = torch.empty_like(uprev)
        ee, rv = C.c_float(), C.c_float()
        self._chk(L.lib.lrnde_sde_sri_step(self._h, C.byref(tab), _dev_ptr(uprev, "uprev", self.D), _dev_ptr(dW, "dW", self.D),
                                           _dev_ptr(dZ, "dZ", self.D), B, float(t), float(dt), float(abstol), float(reltol),
                                           float(delta), _dev_ptr(u, "u"), C.byref(ee), C.byref(rv)))
        return dict(u=u, eest=np.float32(ee.value), reg_val=np.float32(rv.value))

    def solve_fixed(self, u0, dW, t0, dt, abstol, reltol, delta=1.0 / 6.0, solver="EulerHeun"):
        """nsteps = dW.shape[0] steps on a fixed grid in one call (no host round trip per step): dict(u (nsteps,B,D),
        eest (nsteps,), reg_val (nsteps,)); step i equals the single-step call from t0 + i*dt"""
        nsteps = int(dW.shape[0])
        B = u0.numel() // self.D
        dW = dW.contiguous()
        u = torch.empty((nsteps,) + tuple(u0.shape), dtype=torch.float32, device=u0.device)
        ee = (C.c_float * nsteps)(); rv = (C.c_float * nsteps)()
        self._chk(L.lib.lrnde_sde_solve_fixed(self._h, 1 if solver.startswith("RKMil") else 0, _dev_ptr(u0, "u0", self.D),
                                              _dev_ptr(dW, "dW"), B, float(t0), float(dt), nsteps, float(abstol), float(reltol),
                                              float(delta), _dev_ptr(u, "u"), ee, rv))
        return dict(u=u, eest=np.frombuffer(ee, dtype=np.float32).copy(), reg_val=np.frombuffer(rv, dtype=np.float32).copy())


    def solve_adaptive(self, u0, W, t0, t1, abstol, reltol, delta=1.0 / 6.0, dt0=None, gamma=0.9, qmin=0.2, qmax=1.125,
                       beta1=7.0 / 50.0, beta2=2.0 / 25.0, maxiters=10000, solver="EulerHeun", tableau=None, path_z=None, nfine=None):
        """adaptive solve on the caller's Brownian path W ((nfine+1, B, D), W[0] = 0, uniform grid over (t0, t1)):
        dict(u_end, stats, trace) — steps are whole grid intervals, EEst drives a PI controller (lrnde.h).  solver: "EulerHeun",
        "RKMil" or "SRI" (with tableau= and the second path path_z=, same shape as W).  After `set_path_tree`: W=None with
        nfine= (a power of two), the path is the handle's virtual tree"""
        nfine = self._nfine_of(W, nfine)
        B = u0.numel() // self.D
        o = L.SdeAdaptOpts(float(abstol), float(reltol), float(delta), float((t1 - t0) / nfine if dt0 is None else dt0),
                           float(gamma), float(qmin), float(qmax), float(beta1), float(beta2), int(maxiters))
        u_end = torch.empty_like(u0)
        st = L.Stats()
        ntr = int(maxiters) + 4
        tr = (L.TraceRow * ntr)()
        which = _which(solver)
        if which == 0:
            self._chk(L.lib.lrnde_sde_solve_adaptive(self._h, _dev_ptr(u0, "u0", self.D), self._path_ptr(W, "W"), nfine, B,
                                                     float(t0), float(t1), C.byref(o), _dev_ptr(u_end, "u_end"), C.byref(st), tr, ntr))
        else:
            tab = None if tableau is None else C.byref(_sri_tab(tableau))
            Z = None if path_z is None else _dev_ptr(path_z.contiguous(), "path_z")
            self._chk(L.lib.lrnde_sde_solve_adaptive_alg(self._h, _dev_ptr(u0, "u0", self.D), self._path_ptr(W, "W"), nfine, B,
                                                         float(t0), float(t1), C.byref(o), _dev_ptr(u_end, "u_end"), C.byref(st), tr, ntr,
                                                         which, tab, Z))
        nt = st.naccept + st.nreject
        trace = np.array([(tr[i].t, tr[i].dt, tr[i].eest, tr[i].accepted) for i in range(nt)],
                         dtype=[("t", "f4"), ("dt", "f4"), ("eest", "f4"), ("accepted", "i4")])
        return dict(u_end=u_end, stats=st.asdict(), trace=trace)

    @staticmethod
    def _nfine_of(W, nfine):
        if W is not None:
            return int(W.shape[0]) - 1
        if nfine is None:
            raise ValueError("W=None (the path tree, after set_path_tree) needs nfine=")
        return int(nfine)

    @staticmethod
    def _series_cap(sv, nfine, maxiters, mode, tree):
        """states the series buffer of a recorded forward starts with.  :biased without a saveat saves every accepted step: at most
        min(nfine, maxiters) of them — never a grid-sized buffer.  On the path tree (a grid of up to 2^20 intervals, of which a solve
        takes few) the buffer starts at 64 steps; a forward whose series does not fit says how many states it has
        (LRNDE_CAPACITY) and is run again with exactly that many — the same path, the same bits"""
        every = min(int(nfine), max(int(maxiters), 1)) + 1 if (mode == "biased" and not sv.size) else 0
        return int(sv.size) + 3 + (min(every, 65) if tree else every)

    def _run_series(self, cap, shape, device, ns, call):
        """allocate the (cap,) + shape series and run call(us, ts, cap) -> status; a series that does not fit (LRNDE_CAPACITY, ns
        says how many states there are) is run once more with exactly ns states.  Returns (us, ts)"""
        for _ in range(2):
            us = torch.empty((cap,) + tuple(shape), dtype=torch.float32, device=device)
            ts = np.empty(cap, dtype=np.float32)
            rc = call(us, ts, cap)
            if rc == 5 and int(ns.value) > cap:   # LRNDE_CAPACITY
                cap = int(ns.value)
                continue
            break
        self._chk(rc)
        return us, ts

    @staticmethod
    def _path_ptr(W, name):
        return None if W is None else _dev_ptr(W.contiguous(), name)

    # ---- the virtual Brownian tree (lrnde_sde_set_path_tree / lrnde_sde_tree_path; csrc/lrnde_sde_tree.hpp) ----
    def set_path_tree(self, seed):
        """from now on the adaptive calls of this handle ignore W / path_z (pass None and nfine=, a power of two <= 2^20) and take
        the path from the tree of `seed`: W[k] is a function of (seed, column, k) — no (nfine+1, B, D) array exists"""
        self._chk(L.lib.lrnde_sde_set_path_tree(self._h, 1, int(seed) & (2 ** 64 - 1)))

    def clear_path_tree(self):
        """back to the caller's arrays (the default)"""
        self._chk(L.lib.lrnde_sde_set_path_tree(self._h, 0, 0))

    def tree_path(self, seed, stream, levels, B, t0, t2):
        """the tree's whole array (2^levels + 1, B, D) for the span (t0, t2): stream 6 is W, 7 the SRI solve's Z"""
        levels = int(levels)
        if not 0 <= levels <= 20:
            raise ValueError("levels must lie in 0..20")
        out = torch.empty(((1 << levels) + 1, int(B), self.D), dtype=torch.float32, device=f"cuda:{self.device}")
        self._chk(L.lib.lrnde_sde_tree_path(self._h, int(seed) & (2 ** 64 - 1), int(stream), levels, int(B), float(np.float32(t0)),
                                            float(np.float32(t2)), C.c_void_p(out.data_ptr())))
        return out

    SOLVE_LOOPS = ("host", "device", "device-persistent")

    def last_solve_info(self):
        """how the last adaptive solve of this handle ran (lrnde_sde_last_solve_info; for a layer call the main solve with its
        automatic initial dt, not the local step): kind 0 the host-controlled loop / 1 the device controller, one launch per
        attempted step / 2 the device controller in one persistent launch (Euler-Heun only); launches: step-kernel launches
        enqueued; host_waits: stream synchronisations plus waits for a report with nothing enqueued behind them"""
        k, n, w = C.c_int32(), C.c_int32(), C.c_int32()
        self._chk(L.lib.lrnde_sde_last_solve_info(self._h, C.byref(k), C.byref(n), C.byref(w)))
        return dict(kind=int(k.value), launches=int(n.value), host_waits=int(w.value))

    BACKWARD_ROUTES = ("per-step", "one-launch sweep")

    def last_backward_info(self):
        """how the last `node_backward_recorded` (or the model's pullback around it) of this handle ran
        (lrnde_sde_last_backward_info): kind 0 launch sequences per recorded step / 1 the one-launch sweep, for all three step
        kinds; launches: kernels the call enqueued (kind 1; -1 for kind 0); host_waits: stream synchronisations inside the
        call (kind 1: 1, or 0 when the model's pullback waits for it; -1 for kind 0)"""
        k, n, w = C.c_int32(), C.c_int32(), C.c_int32()
        self._chk(L.lib.lrnde_sde_last_backward_info(self._h, C.byref(k), C.byref(n), C.byref(w)))
        return dict(kind=int(k.value), launches=int(n.value), host_waits=int(w.value))

    def draw_noise(self, seed, stream, nsteps, B, scale, cumulative):
        """Gaussian noise drawn on the device (lrnde_sde_draw_noise, counter-based: sample b's noise does not depend on B or
        nsteps): cumulative -> the path (nsteps+1, B, D), row 0 zero, else the increments scale * z (nsteps, B, D)"""
        rows = int(nsteps) + (1 if cumulative else 0)
        out = torch.empty((max(rows, 0), int(B), self.D), dtype=torch.float32, device=f"cuda:{self.device}")
        if out.numel() == 0 and rows == 0 and int(B) > 0:   # nothing to write (an empty tensor has no data pointer)
            return out
        self._chk(L.lib.lrnde_sde_draw_noise(self._h, int(seed), int(stream), int(nsteps), int(B), float(np.float32(scale)),
                                             1 if cumulative else 0, C.c_void_p(out.data_ptr())))
        return out

    def _pcounts(self):
        return self._keep[0].numel(), self._keep[1].numel()

    # ---- the MNIST-SDE model around the layer (experiments/src/construct.jl:202-210; lrnde_sde_model.hpp) ----
    def dense_forward(self, x, pd):
        """`downsample = Dense(Din => D)`: x (B, Din), pd = [vec(W) (D x Din, column-major); b] -> u0 (B, D)"""
        B, Din = int(x.shape[0]), int(x.shape[1])
        if pd.numel() != self.D * (Din + 1):
            raise ValueError(f"downsample parameters must have {self.D * (Din + 1)} entries")
        u0 = torch.empty((B, self.D), dtype=torch.float32, device=x.device)
        self._chk(L.lib.lrnde_sde_dense_forward(self._h, _dev_ptr(x, "x"), B, Din, _dev_ptr(pd, "pd"), C.c_void_p(u0.data_ptr())))
        return u0

    def dense_backward(self, x, pd, du0, want_dx=False):
        """that layer's pullback: dict(dpd, dx) (dx None unless asked for: x is data in the experiment)"""
        B, Din = int(x.shape[0]), int(x.shape[1])
        if pd.numel() != self.D * (Din + 1):
            raise ValueError(f"downsample parameters must have {self.D * (Din + 1)} entries")
        dpd = torch.empty_like(pd)
        dx = torch.empty_like(x) if want_dx else None
        self._chk(L.lib.lrnde_sde_dense_backward(self._h, _dev_ptr(x, "x"), B, Din, _dev_ptr(pd, "pd"), _dev_ptr(du0, "du0", self.D),
                                                 C.c_void_p(dpd.data_ptr()), C.c_void_p(dx.data_ptr()) if want_dx else None))
        return dict(dpd=dpd, dx=dx)

    def _head_args(self, B, pc, K, labels):
        if pc.numel() != K * (self.D + 1):
            raise ValueError(f"classifier parameters must have {K * (self.D + 1)} entries")
        if not (labels.is_cuda and labels.dtype == torch.int32 and labels.numel() == B):
            raise ValueError("labels must be a CUDA int32 tensor of length B")

    def classifier_ce(self, u, pc, K, labels, want_grads=True):
        """`classifier = Dense(D => K)` + logitcrossentropy on the SDE handle: dict(loss, logits, du, dpc)"""
        B = u.numel() // self.D
        self._head_args(B, pc, K, labels)
        logits = torch.empty((B, K), dtype=torch.float32, device=u.device)
        du = torch.empty_like(u) if want_grads else None
        dpc = torch.empty_like(pc) if want_grads else None
        loss = C.c_float()
        self._chk(L.lib.lrnde_sde_classifier_ce(self._h, _dev_ptr(u, "u", self.D), B, _dev_ptr(pc, "pc"), int(K),
                                                C.c_void_p(labels.data_ptr()), C.byref(loss), C.c_void_p(logits.data_ptr()),
                                                C.c_void_p(du.data_ptr()) if want_grads else None,
                                                C.c_void_p(dpc.data_ptr()) if want_grads else None))
        return dict(loss=np.float32(loss.value), logits=logits, du=du, dpc=dpc)

    def record_generation(self):
        g = C.c_uint64()
        self._chk(L.lib.lrnde_sde_record_generation(self._h, C.byref(g)))
        return int(g.value)

    def model_forward_record_ce(self, x, pd, W, t0, t2, abstol, reltol, pc, K, labels, mode="unbiased", t1_or_rand=0.5, z_local=None,
                                saveat=(), save_start=-1, delta=1.0 / 6.0, dt0=0.0, gamma=0.9, qmin=0.2, qmax=1.125, beta1=7.0 / 50.0,
                                beta2=2.0 / 25.0, maxiters=10000, solver="EulerHeun", tableau=None, path_z=None, z_local2=None, nfine=None):
        """downsample -> `node_forward_record` -> head on sol.u[end] in one call with one wait (lrnde_sde_model_forward_record_ce):
        the layer's dict plus loss, logits, dpc; keeps the record for one `model_backward_recorded`"""
        B, Din = int(x.shape[0]), int(x.shape[1])
        if pd.numel() != self.D * (Din + 1):
            raise ValueError(f"downsample parameters must have {self.D * (Din + 1)} entries")
        self._head_args(B, pc, K, labels)
        nfine = self._nfine_of(W, nfine)   # (W=None with nfine=: the path tree, after set_path_tree)
        W = None if W is None else W.contiguous()
        sv = np.ascontiguousarray(saveat, dtype=np.float32)
        o = L.SdeAdaptOpts(float(abstol), float(reltol), float(delta), float(dt0), float(gamma), float(qmin), float(qmax),
                           float(beta1), float(beta2), int(maxiters))
        cap = self._series_cap(sv, nfine, maxiters, mode, W is None)
        ns, reg, nf, ng, st, t1u, loss = C.c_int32(), C.c_float(), C.c_int32(), C.c_int32(), L.Stats(), C.c_float(), C.c_float()
        logits = torch.empty((B, K), dtype=torch.float32, device=x.device)
        dpc = torch.empty_like(pc)
        z_local = None if z_local is None else z_local.contiguous()
        path_z = None if path_z is None else path_z.contiguous()
        z_local2 = None if z_local2 is None else z_local2.contiguous()
        which = _which(solver)
        us, ts = self._run_series(cap, (B, self.D), x.device, ns, lambda us, ts, cap: L.lib.lrnde_sde_model_forward_record_ce(
            self._h, _dev_ptr(x, "x"), Din, _dev_ptr(pd, "pd"), self._path_ptr(W, "W"), nfine, B, float(t0), float(t2), C.byref(o), L.MODE[mode],
            float(t1_or_rand), None if z_local is None else _dev_ptr(z_local, "z_local", self.D), int(save_start),
            sv.ctypes.data_as(C.POINTER(C.c_float)) if sv.size else None, int(sv.size), C.c_void_p(us.data_ptr()),
            ts.ctypes.data_as(C.POINTER(C.c_float)), cap, C.byref(ns), C.byref(reg), C.byref(nf), C.byref(ng), C.byref(st), C.byref(t1u),
            which, None if tableau is None or which != 2 else C.byref(_sri_tab(tableau)), None if path_z is None else _dev_ptr(path_z, "path_z"),
            None if z_local2 is None else _dev_ptr(z_local2, "z_local2", self.D), _dev_ptr(pc, "pc"), int(K), C.c_void_p(labels.data_ptr()),
            C.byref(loss), C.c_void_p(logits.data_ptr()), C.c_void_p(dpc.data_ptr())))
        self._node_keep = (W, x, path_z, pd)   # the record refers to them: alive until the backward
        self._model_shape = (B, Din)
        n = int(ns.value)
        return dict(u=us[:n], t=ts[:n].copy(), u_end=us[n - 1], reg_val=np.float32(reg.value), nfe_drift=int(nf.value),
                    nfe_diffusion=int(ng.value), stats=st.asdict(), t1=np.float32(t1u.value), loss=np.float32(loss.value),
                    logits=logits, dpc=dpc, generation=self.record_generation())

    def model_backward_recorded(self, w_reg=0.0, want_dx=False):
        """the pullback of  logitcrossentropy + w_reg * reg_val  from the record of `model_forward_record_ce`:
        dict(dpd, dp_drift, dp_diff, dx)"""
        B, Din = self._model_shape
        nf, ng = self._pcounts()
        dev = self._keep[0].device
        dpd = torch.empty(self.D * (Din + 1), dtype=torch.float32, device=dev)
        dpf = torch.empty(nf, dtype=torch.float32, device=dev)
        dpg = torch.empty(ng, dtype=torch.float32, device=dev)
        dx = torch.empty((B, Din), dtype=torch.float32, device=dev) if want_dx else None
        self._chk(L.lib.lrnde_sde_model_backward_recorded(self._h, B, float(w_reg), C.c_void_p(dpd.data_ptr()), C.c_void_p(dpf.data_ptr()),
                                                          C.c_void_p(dpg.data_ptr()), C.c_void_p(dx.data_ptr()) if want_dx else None))
        return dict(dpd=dpd, dp_drift=dpf, dp_diff=dpg, dx=dx)

    def node_forward_record(self, x, W, t0, t2, abstol, reltol, mode="unbiased", t1_or_rand=0.5, z_local=None, saveat=(),
                            save_start=-1, delta=1.0 / 6.0, dt0=0.0, gamma=0.9, qmin=0.2, qmax=1.125, beta1=7.0 / 50.0,
                            beta2=2.0 / 25.0, maxiters=10000, solver="EulerHeun", tableau=None, path_z=None, z_local2=None, nfine=None):
        """the NeuralDSDE layer forward (lrnde_sde_node_forward_record[_alg]): adaptive solve on the path W ((nfine+1, B, D),
        W[0] = 0), sol.u / sol.t as the layer's caller sees them, reg_val of the local step; keeps the record for one
        `node_backward_recorded`.  dt0 = 0: automatic initial dt.  solver: "EulerHeun", "RKMil" or "SRI" (with tableau=, the
        second path path_z= and the local step's second draw z_local2=).  After `set_path_tree`: W=None (and path_z=None) with nfine=."""
        nfine = self._nfine_of(W, nfine)
        B = x.numel() // self.D
        W = None if W is None else W.contiguous()
        sv = np.ascontiguousarray(saveat, dtype=np.float32)
        o = L.SdeAdaptOpts(float(abstol), float(reltol), float(delta), float(dt0), float(gamma), float(qmin), float(qmax),
                           float(beta1), float(beta2), int(maxiters))
        cap = self._series_cap(sv, nfine, maxiters, mode, W is None)
        ns, reg, nf, ng, st, t1u = C.c_int32(), C.c_float(), C.c_int32(), C.c_int32(), L.Stats(), C.c_float()
        if z_local is not None:
            z_local = z_local.contiguous()
        which = _which(solver)
        path_z = None if path_z is None else path_z.contiguous()
        z_local2 = None if z_local2 is None else z_local2.contiguous()

        def call(us, ts, cap):
            args = (self._h, _dev_ptr(x, "x", self.D), self._path_ptr(W, "W"), nfine, B, float(t0), float(t2), C.byref(o), L.MODE[mode],
                    float(t1_or_rand), None if z_local is None else _dev_ptr(z_local, "z_local", self.D), int(save_start),
                    sv.ctypes.data_as(C.POINTER(C.c_float)) if sv.size else None, int(sv.size), C.c_void_p(us.data_ptr()),
                    ts.ctypes.data_as(C.POINTER(C.c_float)), cap, C.byref(ns), C.byref(reg), C.byref(nf), C.byref(ng), C.byref(st), C.byref(t1u))
            if which == 0:
                return L.lib.lrnde_sde_node_forward_record(*args)
            return L.lib.lrnde_sde_node_forward_record_alg(
                *args, which, None if tableau is None else C.byref(_sri_tab(tableau)),
                None if path_z is None else _dev_ptr(path_z, "path_z"), None if z_local2 is None else _dev_ptr(z_local2, "z_local2", self.D))

        us, ts = self._run_series(cap, tuple(x.shape), x.device, ns, call)
        self._node_keep = (W, x, path_z)   # the record refers to the caller's path(s): keep them alive until the backward
        n = int(ns.value)
        return dict(u=us[:n], t=ts[:n].copy(), u_end=us[n - 1], reg_val=np.float32(reg.value), nfe_drift=int(nf.value),
                    nfe_diffusion=int(ng.value), stats=st.asdict(), t1=np.float32(t1u.value))

    def node_backward_recorded(self, du_series, w_reg=0.0):
        """pullback of sum_j <du_j, sol.u[j]> + w_reg * reg_val from the record of `node_forward_record`"""
        du_series = du_series.contiguous()
        nser = int(du_series.shape[0])
        B = du_series[0].numel() // self.D
        nf, ng = self._pcounts()
        dx = torch.empty_like(du_series[0])
        dpf = torch.empty(nf, dtype=torch.float32, device=dx.device)
        dpg = torch.empty(ng, dtype=torch.float32, device=dx.device)
        self._chk(L.lib.lrnde_sde_node_backward_recorded(self._h, B, _dev_ptr(du_series, "du_series", self.D), nser, float(w_reg),
                                                         _dev_ptr(dx, "dx"), C.c_void_p(dpf.data_ptr()), C.c_void_p(dpg.data_ptr())))
        return dict(dx=dx, dp_drift=dpf, dp_diff=dpg)

    def solve_fixed_backward(self, u0, u_traj, dW, t0, dt, du_end, solver="EulerHeun"):
        """pullback of solve_fixed (Euler-Heun, or solver="RKMil": the Milstein step) for <du_end, u_traj[-1]>:
        dict(dx, dp_drift, dp_diff)"""
        nsteps = int(dW.shape[0])
        B = u0.numel() // self.D
        nf, ng = self._pcounts()
        dx = torch.empty_like(u0)
        dpf = torch.empty(nf, dtype=torch.float32, device=u0.device)
        dpg = torch.empty(ng, dtype=torch.float32, device=u0.device)
        fn = L.lib.lrnde_sde_solve_fixed_backward_rkmil if solver.startswith("RKMil") else L.lib.lrnde_sde_solve_fixed_backward
        self._chk(fn(self._h, _dev_ptr(u0, "u0", self.D), _dev_ptr(u_traj.contiguous(), "u_traj"),
                                                       _dev_ptr(dW.contiguous(), "dW"), B, float(t0), float(dt), nsteps,
                                                       _dev_ptr(du_end, "du_end", self.D), _dev_ptr(dx, "dx"),
                                                       C.c_void_p(dpf.data_ptr()), C.c_void_p(dpg.data_ptr())))
        return dict(dx=dx, dp_drift=dpf, dp_diff=dpg)

    def sri_step_backward(self, tableau, uprev, dW, dZ, t, dt, abstol, reltol, delta, du_new=None, w_reg=0.0, want_dx=True,
                          dp_drift=None, dp_diff=None):
        """reverse sweep of one four-stage SRI step (lrnde_sde_sri_step_backward) for <du_new, u'> + w_reg * EEst*dt:
        dict(dx, dp_drift, dp_diff, reg_val); dp_* are accumulated into the given tensors (fresh zeros by default)"""
        B = uprev.numel() // self.D
        tab = tableau if isinstance(tableau, L.SriTableau) else L.SriTableau(*[float(v) for v in tableau])
        nf, ng = self._pcounts()
        dpf = torch.zeros(nf, dtype=torch.float32, device=uprev.device) if dp_drift is None else dp_drift
        dpg = torch.zeros(ng, dtype=torch.float32, device=uprev.device) if dp_diff is None else dp_diff
        dx = torch.empty_like(uprev) if want_dx else None
        rv = C.c_float()
        self._chk(L.lib.lrnde_sde_sri_step_backward(
            self._h, C.byref(tab), _dev_ptr(uprev, "uprev", self.D), _dev_ptr(dW, "dW", self.D), _dev_ptr(dZ, "dZ", self.D), B, float(t),
            float(dt), float(abstol), float(reltol), float(delta), None if du_new is None else _dev_ptr(du_new.contiguous(), "du_new", self.D),
            float(w_reg), None if dx is None else _dev_ptr(dx, "dx"), C.c_void_p(dpf.data_ptr()), C.c_void_p(dpg.data_ptr()), C.byref(rv)))
        return dict(dx=dx, dp_drift=dpf, dp_diff=dpg, reg_val=np.float32(rv.value))

    def rkmil_reg_grad(self, uprev, dW, t, dt, abstol, reltol):
        """d (EEst*dt) / d (p_drift, p_diffusion) of one local Milstein step (src/perform_step.jl:108-170), uprev / dW / dt constant"""
        B = uprev.numel() // self.D
        nf, ng = self._pcounts()
        dpf = torch.empty(nf, dtype=torch.float32, device=uprev.device)
        dpg = torch.empty(ng, dtype=torch.float32, device=uprev.device)
        rv = C.c_float()
        self._chk(L.lib.lrnde_sde_rkmil_reg_grad(self._h, _dev_ptr(uprev, "uprev", self.D), _dev_ptr(dW, "dW", self.D), B, float(t), float(dt),
                                                 float(abstol), float(reltol), C.c_void_p(dpf.data_ptr()), C.c_void_p(dpg.data_ptr()), C.byref(rv)))
        return dict(dp_drift=dpf, dp_diff=dpg, reg_val=np.float32(rv.value))

    def euler_heun_reg_grad(self, uprev, dW, t, dt, abstol, reltol, delta):
        """d (EEst*dt) / d (p_drift, p_diffusion) of one local Euler-Heun step, uprev / dW / dt constant"""
        B = uprev.numel() // self.D
        nf, ng = self._pcounts()
        dpf = torch.empty(nf, dtype=torch.float32, device=uprev.device)
        dpg = torch.empty(ng, dtype=torch.float32, device=uprev.device)
        rv = C.c_float()
        self._chk(L.lib.lrnde_sde_euler_heun_reg_grad(self._h, _dev_ptr(uprev, "uprev", self.D), _dev_ptr(dW, "dW", self.D), B,
                                                      float(t), float(dt), float(abstol), float(reltol), float(delta),
                                                      C.c_void_p(dpf.data_ptr()), C.c_void_p(dpg.data_ptr()), C.byref(rv)))
        return dict(dp_drift=dpf, dp_diff=dpg, reg_val=np.float32(rv.value))


class NeuralDSDE:
    """`(sol, st) = nsde(x, ps, st)`; ps = dict(drift=flat, diffusion=[vec(Wg); bg]).
    src/layers/neural_sde.jl:1-123.  Default (solver="EulerHeun", adaptive=True): the ADAPTIVE solve on a Brownian path of
    `nfine` grid intervals drawn from st["rng"] (or given as `noise=` / `path=`), kwargs `abstol`, `reltol`, `saveat`, `save_start`
    as the reference's; `adaptive=False`: the fixed grid of `nsteps` steps.  solver="RKMil" / "SRI" (with tableau=): the fixed
    grid unless `adaptive=True`, which runs the same adaptive layer with that step (SRI: a second path Z and a second local
    draw z2, given as `path_z=` / `z_local2=` or drawn after W and z).
    noise_source="device": the noise is drawn on the device (SdeHandle.draw_noise) from one uint64 seed taken from st["rng"]
    before its other draws — streams 0 (path W), 1 (local-step z), 2 (fixed-grid dW), 3 (fixed-grid dZ), 4 (adaptive SRI: path
    Z), 5 (adaptive SRI: local-step z2); arrays given explicitly still win.
    noise_source="tree" (adaptive only, nfine a power of two <= 2^20): the same seed, but no path array at all — the solve queries
    the virtual Brownian tree of the seed (streams 6: W, 7: SRI's Z; SdeHandle.set_path_tree), the record keeps the accepted
    steps' increments for the pullback; z / z2 from streams 1 / 5 as with "device".  `path=` / `path_z=` still win."""

    def __init__(self, drift, diffusion, *, solver="EulerHeun", sensealg=None, tspan=(0.0, 1.0),
                 regularize="unbiased", maxiters=1000, nsteps=20, delta=1.0 / 6.0, tableau=None, adaptive=None, nfine=256,
                 dt0=0.0, noise_source="host", **kwargs):
        regularize = _sym(regularize)
        _check_valid_regularize(regularize)
        if noise_source not in ("host", "device", "tree"):
            raise ValueError("noise_source must be 'host' (numpy draws from st['rng']), 'device' (lrnde_sde_draw_noise from a "
                             "seed drawn from st['rng']) or 'tree' (the virtual Brownian tree of that seed: no path array)")
        self.noise_source = noise_source
        if solver in ("SRI", "FourStageSRI"):
            if tableau is None:
                raise ValueError("solver='SRI' (src/perform_step.jl:49-106) needs tableau=: the 51 coefficients of the "
                                 "FourStageSRIConstantCache (SOSRI's live in un-vendored StochasticDiffEq)")
        elif solver not in ("EulerHeun", "LambaEulerHeun", "RKMil", "RKMilCommute"):
            raise NotImplementedError("on the device: the Euler-Heun step (src/perform_step.jl:172-206), the Milstein step "
                                      "(:108-170) and the four-stage SRI step (:49-106, solver='SRI' with tableau=); SOSRI's own "
                                      "tableau and adaptive noise process live in un-vendored StochasticDiffEq")
        self.solver = "SRI" if solver in ("SRI", "FourStageSRI") else ("RKMil" if solver.startswith("RKMil") else "EulerHeun")
        self.tableau = tableau
        if not isinstance(diffusion, Dense) or diffusion.in_dims != diffusion.out_dims:
            raise NotImplementedError("diffusion must be Dense(D => D) (experiments/src/construct.jl:205)")
        self.drift, self.diffusion = drift, diffusion
        self.desc = _mlp_desc(drift if isinstance(drift, Chain) else drift)
        if self.desc.state_dim != diffusion.in_dims:
            raise ValueError("drift and diffusion state sizes differ")
        self.tspan = (np.float32(tspan[0]), np.float32(tspan[1]))
        self.regularize, self.maxiters, self.nsteps, self.delta = regularize, int(maxiters), int(nsteps), float(delta)
        self.adaptive = (self.solver == "EulerHeun") if adaptive is None else bool(adaptive)
        self.nfine, self.dt0 = int(nfine), float(dt0)
        if noise_source == "tree":
            if not self.adaptive:
                raise ValueError("noise_source='tree' is the adaptive solve's path source: adaptive must be true")
            if self.nfine < 1 or self.nfine > 2 ** 20 or self.nfine & (self.nfine - 1):
                raise ValueError(f"noise_source='tree' needs nfine = 2^L <= 2^20 (got {self.nfine})")
        self.kwargs = dict(kwargs)
        self._handle = None
        self._last_adaptive = None
        self._last_path_z = None   # adaptive SRI: the second path of the last forward

    def initialstates(self, rng):
        rng.standard_normal()  # :23
        return dict(drift={}, diffusion={}, nfe_drift=-1, nfe_diffusion=-1, reg_val=np.float32(0.0),
                    rng=copy.deepcopy(rng), training=True)

    def handle(self):
        if self._handle is None:
            self._handle = SdeHandle(self.desc)
        return self._handle

    def _draw_path(self, rng, shape, device):
        """W on the uniform grid (nfine + 1, B, D), W[0] = 0, and the local step's standard-normal draw, from the host stream"""
        t0, t2 = self.tspan
        h = np.float32((t2 - t0) / np.float32(self.nfine))
        inc = rng.standard_normal((self.nfine,) + tuple(shape)).astype(np.float32) * np.float32(np.sqrt(h))
        W = np.concatenate([np.zeros((1,) + tuple(shape), np.float32), np.cumsum(inc, axis=0, dtype=np.float32)], axis=0)
        z = rng.standard_normal(tuple(shape)).astype(np.float32)
        return torch.from_numpy(W).to(device), torch.from_numpy(z).to(device)

    def _draw_seed(self, rng):
        """the device streams' seed: one uint64 from the layer's host stream"""
        return int(rng.integers(0, 2 ** 64, dtype=np.uint64))

    def _adaptive_draws(self, h, shape, device, st, path=None, z_local=None, path_z=None, z_local2=None):
        """the adaptive layer's draws for an input of `shape` on `device`, from a copy of st["rng"]:
        (rng, path, z_local, path_z, z_local2, mode, t1_or_rand) — arrays given explicitly win"""
        shape = tuple(shape)
        t0, t2 = self.tspan
        rng = copy.deepcopy(st["rng"])
        if self.noise_source == "tree":   # the seed where "device" takes it; z / z2 from its streams 1 / 5; the path is not drawn
            seed = self._draw_seed(rng)
            B = int(np.prod(shape)) // h.D
            need_z = self.solver == "SRI"
            if path is None and (path_z is None or not need_z):
                h.set_path_tree(seed)          # no array: the solve queries the tree (node_forward_record: W=None, nfine=)
            else:                              # an explicit array wins; the other path of an SRI solve is then the tree's array
                h.clear_path_tree()
                L2 = self.nfine.bit_length() - 1
                if path is None:
                    path = h.tree_path(seed, 6, L2, B, t0, t2).view((self.nfine + 1,) + shape)
                if need_z and path_z is None:
                    path_z = h.tree_path(seed, 7, L2, B, t0, t2).view((self.nfine + 1,) + shape)
            if z_local is None:
                z_local = h.draw_noise(seed, 1, 1, B, 1.0, False)[0].view(shape)
            if need_z and z_local2 is None:
                z_local2 = h.draw_noise(seed, 5, 1, B, 1.0, False)[0].view(shape)
            if path is None:
                mode = self.regularize if st["training"] else "none"
                r01 = np.float32(rng.random(dtype=np.float32)) if mode != "none" else np.float32(0)
                t1_or_rand = np.float32(r01 * (t2 - t0) + t0) if mode == "unbiased" else r01     # :92 / :114
                self._last_path_z = None
                return rng, None, z_local, None, z_local2, mode, t1_or_rand
        if self.noise_source == "device":   # W (stream 0) and z (stream 1) on the device; node_forward_record keeps W alive
            seed = self._draw_seed(rng)
            B = int(np.prod(shape)) // h.D
            if path is None:
                hh = np.float32((t2 - t0) / np.float32(self.nfine))
                path = h.draw_noise(seed, 0, self.nfine, B, np.float32(np.sqrt(hh)), True).view((self.nfine + 1,) + shape)
            if z_local is None:
                z_local = h.draw_noise(seed, 1, 1, B, 1.0, False)[0].view(shape)
            if self.solver == "SRI":   # the second path (stream 4) and the local step's second draw (stream 5)
                if path_z is None:
                    hh = np.float32((t2 - t0) / np.float32(self.nfine))
                    path_z = h.draw_noise(seed, 4, self.nfine, B, np.float32(np.sqrt(hh)), True).view((self.nfine + 1,) + shape)
                if z_local2 is None:
                    z_local2 = h.draw_noise(seed, 5, 1, B, 1.0, False)[0].view(shape)
        if path is None:
            path, z_draw = self._draw_path(rng, shape, device)
            z_local = z_draw if z_local is None else z_local
        else:
            path = torch.as_tensor(path, dtype=torch.float32).to(device)
            if z_local is None:
                z_local = torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(device)
        if self.solver == "SRI":   # host draws of Z, then z2, AFTER W and z (the other solvers' draw sequences are unchanged)
            if path_z is None:
                path_z, z2_draw = self._draw_path(rng, shape, device)
                z_local2 = z2_draw if z_local2 is None else z_local2
            else:
                path_z = torch.as_tensor(path_z, dtype=torch.float32).to(device)
                if z_local2 is None:
                    z_local2 = torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(device)
            self._last_path_z = path_z
        mode = self.regularize if st["training"] else "none"
        r01 = np.float32(rng.random(dtype=np.float32)) if mode != "none" else np.float32(0)
        t1_or_rand = np.float32(r01 * (t2 - t0) + t0) if mode == "unbiased" else r01     # :92 / :114
        return rng, path, z_local, path_z, z_local2, mode, t1_or_rand

    def _call_adaptive(self, x, ps, st, path=None, z_local=None, path_z=None, z_local2=None):
        h = self.handle()
        h.set_params(ps["drift"], ps["diffusion"])
        t0, t2 = self.tspan
        abstol, reltol = self.kwargs.get("abstol", 1e-2), self.kwargs.get("reltol", 1e-2)
        rng, path, z_local, path_z, z_local2, mode, t1_or_rand = self._adaptive_draws(h, x.shape, x.device, st, path, z_local, path_z, z_local2)
        saveat = self.kwargs.get("saveat", ())
        r = h.node_forward_record(x, path, t0, t2, abstol, reltol, mode=mode, t1_or_rand=float(t1_or_rand), z_local=z_local,
                                  saveat=() if saveat is None else saveat, save_start=int(self.kwargs.get("save_start", -1)),
                                  delta=self.delta, dt0=self.dt0, maxiters=self.maxiters, solver=self.solver,
                                  tableau=self.tableau if self.solver == "SRI" else None, path_z=path_z, z_local2=z_local2,
                                  nfine=self.nfine)
        self._last_adaptive = dict(nseries=int(r["u"].shape[0]), mode=mode)
        sol = ODESolution([r["u"][i] for i in range(r["u"].shape[0])], [np.float32(t) for t in r["t"]], r["nfe_drift"])
        sol.stats = r["stats"]
        return sol, dict(drift=st["drift"], diffusion=st["diffusion"], nfe_drift=r["nfe_drift"], nfe_diffusion=r["nfe_diffusion"],
                         reg_val=r["reg_val"], rng=rng, training=st["training"])

    def __call__(self, x, ps, st, noise=None, path=None, z_local=None, path_z=None, z_local2=None):
        if self.adaptive:
            return self._call_adaptive(x, ps, st, path=path if path is not None else noise, z_local=z_local, path_z=path_z, z_local2=z_local2)
        h = self.handle()
        h.set_params(ps["drift"], ps["diffusion"])
        t0, t2 = self.tspan
        abstol, reltol = self.kwargs.get("abstol", 1e-2), self.kwargs.get("reltol", 1e-2)
        n = self.nsteps
        dt = np.float32((t2 - t0) / np.float32(n))
        rng = copy.deepcopy(st["rng"])
        seed = self._draw_seed(rng) if self.noise_source == "device" else None
        B = x.numel() // h.D
        if noise is None and seed is not None:   # dW (stream 2) on the device
            noise = h.draw_noise(seed, 2, n + 1, B, np.float32(np.sqrt(dt)), False).view((n + 1,) + tuple(x.shape))
        if noise is None:  # W.dW ~ sqrt(dt) N(0,1), drawn on the host stream
            noise = (rng.standard_normal((n + 1,) + tuple(x.shape)).astype(np.float32) * np.float32(np.sqrt(dt)))
        noise = torch.as_tensor(noise, dtype=torch.float32).to(x.device)
        # step(u, i, t): one step with the i-th increments of the noise process
        if self.solver == "SRI":  # second increment dZ (W.dZ): stream 3 on the device, or drawn after dW from the same host stream
            if seed is not None:
                dz = h.draw_noise(seed, 3, n + 1, B, np.float32(np.sqrt(dt)), False).view((n + 1,) + tuple(x.shape))
            else:
                dz = torch.as_tensor(rng.standard_normal((n + 1,) + tuple(x.shape)).astype(np.float32) * np.float32(np.sqrt(dt))).to(x.device)
            step = lambda uu, i, tt: h.sri_step(self.tableau, uu, noise[i].contiguous(), dz[i].contiguous(), tt, dt, abstol, reltol, self.delta)
            us, u = [], x
            for i in range(n):
                u = step(u, i, np.float32(t0 + np.float32(i) * dt))["u"]
                us.append(u)
            self._last_solve = dict(us=us, dW=noise, dZ=dz, t0=t0, dt=dt, abstol=abstol, reltol=reltol)
        else:
            if self.solver == "RKMil":
                step = lambda uu, i, tt: h.rkmil_step(uu, noise[i].contiguous(), tt, dt, abstol, reltol)
            else:
                step = lambda uu, i, tt: h.euler_heun_step(uu, noise[i].contiguous(), tt, dt, abstol, reltol, self.delta)
            traj = h.solve_fixed(x, noise[:n], t0, dt, abstol, reltol, self.delta, self.solver)  # the n steps, one host sync
            us = [traj["u"][i] for i in range(n)]
            self._last_solve = dict(u_traj=traj["u"], dW=noise[:n], t0=t0, dt=dt)
        ts = [np.float32(t0 + np.float32(i + 1) * dt) if i + 1 < n else t2 for i in range(n)]
        per_step = {"RKMil": (1, 2), "SRI": (4, 4)}.get(self.solver, (3, 3))  # (drift, diffusion) evaluations of one step
        nfe, nfe_g = per_step[0] * n, per_step[1] * n
        mode = self.regularize if st["training"] else "none"
        reg_val = np.float32(0.0)
        if mode != "none":
            if mode == "unbiased":  # :88-105: t1 uniform in (t0,t2); sol(t1) by linear interpolation
                t1 = np.float32(rng.random(dtype=np.float32) * (t2 - t0) + t0)
                j = min(int((t1 - t0) / dt), n - 1)
                ta = t0 if j == 0 else ts[j - 1]
                ua = x if j == 0 else us[j - 1]
                th = np.float32((t1 - ta) / (ts[j] - ta))
                u1 = (ua + th * (us[j] - ua)).contiguous()
            else:  # :109-123: rand(rng, sol.t[1:end-1]) — every saved time but the last, t0 included (the SDE solve saves
                # its start); one uniform draw, index floor(r * m) (layers.biased_index: the package's one convention)
                from .layers import biased_index
                j = biased_index(np.float32(rng.random(dtype=np.float32)), n)
                t1, u1 = (t0, x) if j == 0 else (ts[j - 1], us[j - 1])
            # the local step's integrator is a fresh `init` on (t1, t2) (:96,116): its first dt is clipped to the span
            dt_loc = np.float32(min(dt, np.float32(t2 - t1)))
            if self.solver == "SRI":
                r = h.sri_step(self.tableau, u1, noise[n].contiguous(), dz[n].contiguous(), t1, dt_loc, abstol, reltol, self.delta)
            elif self.solver == "RKMil":
                r = h.rkmil_step(u1, noise[n].contiguous(), t1, dt_loc, abstol, reltol)
            else:
                r = h.euler_heun_step(u1, noise[n].contiguous(), t1, dt_loc, abstol, reltol, self.delta)
            reg_val = r["reg_val"]
            nfe += per_step[0]; nfe_g += per_step[1]
            self._last_local = dict(t1=t1, dt=dt_loc, u1=u1, dW=noise[n].contiguous(), abstol=abstol, reltol=reltol,
                                    dZ=dz[n].contiguous() if self.solver == "SRI" else None)
        sol = ODESolution([us[-1]], [t2], nfe)
        return sol, dict(drift=st["drift"], diffusion=st["diffusion"], nfe_drift=nfe, nfe_diffusion=nfe_g,
                         reg_val=reg_val, rng=rng, training=st["training"])

    def pullback(self, x, ps, st, du_end, w_reg=0.0, noise=None):
        """What the reference's Tracker-based pullback gives for  loss = <du_end, sol.u[end]> + w_reg * reg_val
        (test/runtests.jl:361-365, 386-397): (dx, dict(drift=, diffusion=), info).  The forward is re-run with the same
        draws as `__call__` (st['rng']; `noise` if given); the solve is differentiated through its own steps, reg_val
        w.r.t. the parameters only (info['dx_reg'] is None: `gs_x === nothing` in the reference)."""
        if self.adaptive:   # every solver's adaptive layer: the reverse sweep over its record
            return self.pullback_series(x, ps, st, None, du_end=du_end, w_reg=w_reg, path=noise)
        if self.solver == "SRI":   # the fixed-grid loop of four-stage SRI steps, newest first (lrnde_sde_sri_step_backward)
            sol, st2 = self(x, ps, st, noise=noise)
            h = self.handle()
            fs = self._last_solve
            n = len(fs["us"])
            ub, dpf, dpg = du_end.contiguous(), None, None
            for i in range(n - 1, -1, -1):
                ui = x if i == 0 else fs["us"][i - 1]
                r = h.sri_step_backward(self.tableau, ui, fs["dW"][i].contiguous(), fs["dZ"][i].contiguous(),
                                        np.float32(fs["t0"] + np.float32(i) * fs["dt"]), fs["dt"], fs["abstol"], fs["reltol"], self.delta,
                                        du_new=ub, dp_drift=dpf, dp_diff=dpg)
                ub, dpf, dpg = r["dx"], r["dp_drift"], r["dp_diff"]
            mode = self.regularize if st["training"] else "none"
            if mode != "none" and w_reg != 0.0:
                lo = self._last_local
                rg = h.sri_step_backward(self.tableau, lo["u1"], lo["dW"], lo["dZ"], lo["t1"], lo["dt"], lo["abstol"], lo["reltol"], self.delta,
                                         du_new=None, w_reg=w_reg, want_dx=False, dp_drift=dpf, dp_diff=dpg)
                assert rg["reg_val"] == st2["reg_val"]
            return ub, dict(drift=dpf, diffusion=dpg), dict(sol=sol, st=st2, dx_reg=None)
        sol, st2 = self(x, ps, st, noise=noise)
        h = self.handle()
        fs = self._last_solve
        bw = h.solve_fixed_backward(x, fs["u_traj"], fs["dW"].contiguous(), fs["t0"], fs["dt"], du_end, solver=self.solver)
        dpf, dpg = bw["dp_drift"], bw["dp_diff"]
        mode = self.regularize if st["training"] else "none"
        if mode != "none" and w_reg != 0.0:
            lo = self._last_local
            if self.solver == "RKMil":
                rg = h.rkmil_reg_grad(lo["u1"], lo["dW"], lo["t1"], lo["dt"], lo["abstol"], lo["reltol"])
            else:
                rg = h.euler_heun_reg_grad(lo["u1"], lo["dW"], lo["t1"], lo["dt"], lo["abstol"], lo["reltol"], self.delta)
            assert rg["reg_val"] == st2["reg_val"]
            dpf = dpf + np.float32(w_reg) * rg["dp_drift"]
            dpg = dpg + np.float32(w_reg) * rg["dp_diff"]
        return bw["dx"], dict(drift=dpf, diffusion=dpg), dict(sol=sol, st=st2, dx_reg=None)

    def pullback_series(self, x, ps, st, du_series, du_end=None, w_reg=0.0, path=None, z_local=None, path_z=None, z_local2=None):
        """adaptive layer: pullback of  sum_j <du_series[j], sol.u[j]> + w_reg * reg_val  (du_end alone = a cotangent on
        sol.u[end], what `diffeqsol_to_array` passes back).  The forward is re-run with the same draws; the backward is the
        reverse sweep over its recorded accepted steps (lrnde_sde_node_backward_recorded)."""
        sol, st2 = self._call_adaptive(x, ps, st, path=path, z_local=z_local, path_z=path_z, z_local2=z_local2)
        ns = self._last_adaptive["nseries"]
        if du_series is None:
            du_series = torch.zeros((ns,) + tuple(x.shape), dtype=torch.float32, device=x.device)
            du_series[ns - 1] = du_end
        bw = self.handle().node_backward_recorded(du_series, w_reg=w_reg)
        return bw["dx"], dict(drift=bw["dp_drift"], diffusion=bw["dp_diff"]), dict(sol=sol, st=st2, dx_reg=None,
                                                                                  backward=self.handle().last_backward_info())
