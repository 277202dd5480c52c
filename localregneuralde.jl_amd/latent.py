"""The PhysioNet Latent ODE around the Dense-chain NeuralODE (experiments/src/construct.jl:230-252):
LatentGRUCell / Recurrence (src/layers/latent_ode.jl:1-48), rec_to_gen, ReparameterizeLayer (src/layers/common.jl:47-77),
gen_to_data and the loss (construct.jl:36-76, experiments/src/utils.jl:94-101), over the lrnde_latent_* entry points of
include/lrnde.h.  torch is device memory and streams only: every value comes from liblrnde."""
import copy
import ctypes as C
import time

import numpy as np
import torch

from . import _lib as L
from .layers import Activation, Chain, Dense, NeuralODE, diffeqsol_to_timeseries, glorot_chain_params

BLOCKS = ("update_gate", "reset_gate", "new_state", "rec_to_gen", "gen_to_data")


def latent_block_sizes(in_dims, hidden_dims, latent_dims, node_dims):
    """entries of each block of the flat Lux ComponentArray, in its order (gru.update_gate, gru.reset_gate, gru.new_state,
    rec_to_gen, gen_to_data)"""
    I, H, Ld, N = int(in_dims), int(hidden_dims), int(latent_dims), int(node_dims)
    K = 2 * Ld + 2 * I + 1
    gate = H * K + H + Ld * H + Ld
    return dict(update_gate=gate, reset_gate=gate, new_state=H * K + H + 2 * Ld * H + 2 * Ld,
                rec_to_gen=Ld * 2 * Ld + Ld + 2 * N * Ld + 2 * N, gen_to_data=I * N + I)


def split_latent_params(flat, dims):
    """flat vector -> dict of views by block (BLOCKS order); `dims` = (in_dims, hidden_dims, latent_dims, node_dims)"""
    sizes = latent_block_sizes(*dims)
    if flat.shape[0] != sum(sizes.values()):
        raise ValueError(f"{flat.shape[0]} parameters, the model has {sum(sizes.values())}")
    out, pos = {}, 0
    for name in BLOCKS:
        out[name] = flat[pos:pos + sizes[name]]
        pos += sizes[name]
    return out


def join_latent_params(blocks, dims):
    """the inverse of split_latent_params (numpy arrays or tensors)"""
    sizes = latent_block_sizes(*dims)
    parts = [blocks[name] for name in BLOCKS]
    for name, p in zip(BLOCKS, parts):
        if p.shape[0] != sizes[name]:
            raise ValueError(f"block {name} has {p.shape[0]} entries, not {sizes[name]}")
    return torch.cat(list(parts)) if isinstance(parts[0], torch.Tensor) else np.concatenate(parts)


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _dev(t, name, shape):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise ValueError(f"{name} must be a contiguous float32 CUDA tensor")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)} (got {tuple(t.shape)})")
    return C.c_void_p(t.data_ptr())


class LatentHandle:
    """lrnde_latent: encoder, reparameterisation, decoder and loss of one (in, hidden, latent, node) shape.  A shape the
    kernels cannot hold raises NotImplementedError with the library's message."""

    def __init__(self, in_dims, hidden_dims, latent_dims, node_dims, device=None, stream=None):
        if not torch.cuda.is_available():
            raise RuntimeError("liblrnde needs a GPU (gfx950); there is no CPU fallback")
        self.dims = (int(in_dims), int(hidden_dims), int(latent_dims), int(node_dims))
        self.desc = L.LatentDesc(*self.dims)
        self.nparams = int(L.lib.lrnde_latent_param_count(C.byref(self.desc)))
        self.device = torch.cuda.current_device() if device is None else int(device)
        self._stream = torch.cuda.current_stream(self.device) if stream is None else stream
        self._h = C.c_void_p()
        rc = L.lib.lrnde_latent_create(C.byref(self._h), C.byref(self.desc), self.device, C.c_void_p(self._stream.cuda_stream))
        if rc != 0:
            msg = L.lib.lrnde_latent_last_error(None).decode()
            self._h = None
            if rc == 8:
                raise NotImplementedError(msg)
            raise L.LrndeError(rc, "lrnde_latent_create failed: " + msg)
        self._params = None

    def close(self):
        if getattr(self, "_h", None):
            L.lib.lrnde_latent_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            msg = L.lib.lrnde_latent_last_error(self._h).decode()
            if rc == 8:
                raise NotImplementedError(msg)
            raise L.LrndeError(rc, msg)

    @property
    def nparams_encoder(self):
        I, _, _, N = self.dims
        return self.nparams - (I * N + I)

    def set_params(self, ps):
        ps = ps if isinstance(ps, torch.Tensor) else torch.as_tensor(np.asarray(ps, dtype=np.float32))
        ps = ps.to(device=f"cuda:{self.device}", dtype=torch.float32).contiguous().reshape(-1)
        self._params = ps
        self._chk(L.lib.lrnde_latent_set_params(self._h, C.c_void_p(ps.data_ptr()), ps.numel()))

    def encode(self, x, eps=None, training=True):
        """x (B, T, 2*in_dims+1) -> dict(y (B, 2*latent), mu, logvar, z0 (B, node)); one launch"""
        I, _, Ld, N = self.dims
        if x.dim() != 3:
            raise ValueError("x must be (B, T, 2*in_dims+1)")
        B, T = int(x.shape[0]), int(x.shape[1])
        _dev(x, "x", (B, T, 2 * I + 1))
        if training:
            _dev(eps, "eps", (B, N))
        y = torch.empty((B, 2 * Ld), dtype=torch.float32, device=x.device)
        mu, lv, z0 = (torch.empty((B, N), dtype=torch.float32, device=x.device) for _ in range(3))
        self._chk(L.lib.lrnde_latent_encode(self._h, _ptr(x), B, T, int(bool(training)), _ptr(eps if training else None), _ptr(y), _ptr(mu),
                                            _ptr(lv), _ptr(z0)))
        return dict(y=y, mu=mu, logvar=lv, z0=z0)

    def record_generation(self):
        g = C.c_uint64()
        self._chk(L.lib.lrnde_latent_record_generation(self._h, C.byref(g)))
        return int(g.value)

    def encode_backward(self, x, dz0=None, dmu=None, dlogvar=None, want_dx=True, dy=None):
        """pullback of the recorded encode: dict(dp (encoder parameters: gru, rec_to_gen), dx or None)"""
        I, _, _, N = self.dims
        B, T = int(x.shape[0]), int(x.shape[1])
        _dev(x, "x", (B, T, 2 * I + 1))
        for name, t in (("dz0", dz0), ("dmu", dmu), ("dlogvar", dlogvar)):
            if t is not None:
                _dev(t, name, (B, N))
        if dy is not None:
            _dev(dy, "dy", (B, 2 * self.dims[2]))
        dx = torch.empty_like(x) if want_dx else None
        dp = torch.empty(self.nparams_encoder, dtype=torch.float32, device=x.device)
        self._chk(L.lib.lrnde_latent_encode_backward(self._h, _ptr(x), B, T, _ptr(dy), _ptr(dz0), _ptr(dmu), _ptr(dlogvar), _ptr(dx), _ptr(dp)))
        return dict(dp=dp, dx=dx)

    def decode_loss(self, series, data, mask, mu, logvar, w_kl, want_grads=True):
        """series (T, B, node), data / mask (B, T, in): dict(loss, neg_log_likelihood, kl_div, ll (B), kl (B)) and, with
        want_grads, dseries, dmu, dlogvar, dpg"""
        I, _, _, N = self.dims
        T, B = int(series.shape[0]), int(series.shape[1])
        _dev(series, "series", (T, B, N)); _dev(data, "data", (B, T, I)); _dev(mask, "mask", (B, T, I))
        _dev(mu, "mu", (B, N)); _dev(logvar, "logvar", (B, N))
        ll, kl = (torch.empty(B, dtype=torch.float32, device=series.device) for _ in range(2))
        out = dict(ll=ll, kl=kl)
        if want_grads:
            out.update(dseries=torch.empty_like(series), dmu=torch.empty_like(mu), dlogvar=torch.empty_like(mu),
                       dpg=torch.empty(I * N + I, dtype=torch.float32, device=series.device))
        res = (C.c_float * 3)()
        self._chk(L.lib.lrnde_latent_decode_loss(self._h, _ptr(series), T, B, _ptr(data), _ptr(mask), _ptr(mu), _ptr(logvar), float(w_kl), res,
                                                 _ptr(ll), _ptr(kl), _ptr(out.get("dseries")), _ptr(out.get("dmu")), _ptr(out.get("dlogvar")),
                                                 _ptr(out.get("dpg"))))
        out.update(loss=np.float32(res[0]), neg_log_likelihood=np.float32(res[1]), kl_div=np.float32(res[2]))
        return out

    def predict(self, series):
        """gen_to_data on every saved state: series (T, B, node) -> (B, T, in)"""
        I, _, _, N = self.dims
        T, B = int(series.shape[0]), int(series.shape[1])
        _dev(series, "series", (T, B, N))
        pred = torch.empty((B, T, I), dtype=torch.float32, device=series.device)
        self._chk(L.lib.lrnde_latent_decode(self._h, _ptr(series), T, B, _ptr(pred)))
        return pred

    def last_launches(self):
        """diagnostic hook lrnde_latent_last_launches: kernels of the last encode / encode_backward"""
        f, b = C.c_int32(), C.c_int32()
        self._chk(L.lib.lrnde_latent_last_launches(self._h, C.byref(f), C.byref(b)))
        return dict(encode=int(f.value), backward=int(b.value))


class LatentGRUCell:
    """src/layers/latent_ode.jl:1-17: three two-layer gates on vcat(y_mean, y_std, x).  The cell is evaluated by
    `Recurrence` (all steps in one launch); it has no single-step call of its own here."""

    def __init__(self, in_dim, h_dim, latent_dim):
        self.in_dim, self.h_dim, self.latent_dim = int(in_dim), int(h_dim), int(latent_dim)
        _in = self.latent_dim * 2 + self.in_dim * 2 + 1
        # (in, hidden, out, activations) of the three gates, latent_ode.jl:12-14
        self.update_gate = (_in, self.h_dim, self.latent_dim, ("tanh", "sigmoid"))
        self.reset_gate = (_in, self.h_dim, self.latent_dim, ("tanh", "sigmoid"))
        self.new_state = (_in, self.h_dim, self.latent_dim * 2, ("tanh", "tanh"))

    def param_count(self):
        s = latent_block_sizes(self.in_dim, self.h_dim, self.latent_dim, 1)
        return s["update_gate"] + s["reset_gate"] + s["new_state"]


class Recurrence:
    """Lux.Recurrence(cell) with return_sequence = false (construct.jl:231): `y, st = rec(x, ps, st)` walks x (B, T, F) along T
    and returns the last step's vcat(new_y_mean, new_y_std) (B, 2*latent).  ps: the cell's flat parameters (update_gate,
    reset_gate, new_state).  The library's encoder also carries rec_to_gen and the reparameterisation; used alone, the layer
    runs it with those blocks at zero and reads y."""

    def __init__(self, cell):
        self.cell = cell
        self._handle = None

    def initialstates(self, rng):
        return {}

    def _bind(self, ps):
        c = self.cell
        if self._handle is None:
            self._handle = LatentHandle(c.in_dim, c.h_dim, c.latent_dim, 1)
        h = self._handle
        ps = ps if isinstance(ps, torch.Tensor) else torch.as_tensor(np.asarray(ps, dtype=np.float32))
        ps = ps.to(device="cuda", dtype=torch.float32).reshape(-1)
        if ps.numel() != c.param_count():
            raise ValueError(f"{ps.numel()} parameters, the cell has {c.param_count()}")
        full = torch.zeros(h.nparams, dtype=torch.float32, device=ps.device)
        full[:ps.numel()] = ps
        h.set_params(full)
        return h

    def __call__(self, x, ps, st):
        h = self._bind(ps)
        return h.encode(x, training=False)["y"], st

    def pullback(self, x, ps, st, dy):
        """(dx, dps) for the cotangent dy (B, 2*latent) of y: one recorded encode, then the reverse walk"""
        h = self._bind(ps)
        h.encode(x, training=False)
        bw = h.encode_backward(x, dy=dy.contiguous())
        return bw["dx"], bw["dp"][:self.cell.param_count()]


class ReparameterizeLayer:
    """src/layers/common.jl:47-77.  Julia's random stream cannot be matched: eps comes from a numpy Generator (a copy of
    st["rng"], advanced and returned, as Lux.replicate does), so parity with the reference holds for a given eps, not for a
    given seed."""

    def initialstates(self, rng):
        """common.jl:50-53: burns one normal draw, then replicates the rng"""
        rng.standard_normal(1)
        return dict(rng=copy.deepcopy(rng), training=True, mu0=None, logvar=None)

    @staticmethod
    def draw(st, B, N):
        """(eps (B, N) float32 numpy, the advanced copy of st['rng'])"""
        rng = copy.deepcopy(st["rng"])
        return rng.standard_normal((B, N), dtype=np.float32), rng

    def __call__(self, x, ps, st):
        """x (B, 2N) -> (z0, st) with st['mu0'], st['logvar'] (the reference's μ₀, logσ²).  Elementwise on torch device
        memory ops: the model's path is the encoder kernel's tail (LatentHandle.encode); this stand-alone call serves small checks."""
        N = x.shape[1] // 2
        mu = x[:, :N].contiguous()
        if not st["training"]:   # common.jl:73-77
            return mu, dict(st, mu0=mu, logvar=mu)
        eps, rng = self.draw(st, x.shape[0], N)
        lv = x[:, N:].contiguous()
        z0 = mu + torch.exp(lv / 2) * torch.from_numpy(eps).to(x.device)
        return z0, dict(st, rng=rng, mu0=mu, logvar=lv)


def _gen_dynamics(hidden_dims, node_dims):
    """construct.jl:235-243"""
    layers = [Activation("tanh")]
    for _ in range(4):
        layers += [Dense(node_dims, hidden_dims, "tanh"), Dense(hidden_dims, node_dims, "tanh")]
    return Chain(*layers)


class LatentODE:
    """Chain(; gru, rec_to_gen, reparam, neural_ode, diffeqsol_to_array, gen_to_data), construct.jl:251.
    `y, st = model(x, ps, st)`: x (B, T, 2*in_dims+1), y (B, T, in_dims); ps = dict(latent=flat vector of
    split_latent_params' blocks, neural_ode=flat gen_dynamics parameters); st = dict(neural_ode=..., reparam=...)."""

    def __init__(self, in_dims, hidden_dims, latent_dims, node_dims, saveat, **solver_kwargs):
        self.dims = (int(in_dims), int(hidden_dims), int(latent_dims), int(node_dims))
        self.saveat = [float(t) for t in saveat]
        self.gru = Recurrence(LatentGRUCell(in_dims, hidden_dims, latent_dims))
        self.reparam = ReparameterizeLayer()
        self.gen_dynamics = _gen_dynamics(self.dims[1], self.dims[3])
        solver_kwargs.setdefault("regularize", "none")
        # construct.jl:244-248 passes no save_start, so DiffEq's own default holds: the start state is saved only where
        # tspan[1] is one of the saveat times (or saveat is empty) — y then has one state per saveat time, as the loss needs
        t0 = np.float32(solver_kwargs.get("tspan", (0.0, 1.0))[0])
        solver_kwargs.setdefault("save_start", not self.saveat or any(np.float32(t) == t0 for t in self.saveat))
        self.neural_ode = NeuralODE(self.gen_dynamics, field="dense_chain", saveat=self.saveat, **solver_kwargs)
        self._handle = None

    def handle(self):
        if self._handle is None:
            self._handle = LatentHandle(*self.dims)
        return self._handle

    def initialstates(self, rng):
        return dict(neural_ode=self.neural_ode.initialstates(rng), reparam=self.reparam.initialstates(rng))

    def _encode(self, h, x, st):
        B, N = int(x.shape[0]), self.dims[3]
        training = bool(st["reparam"]["training"])
        if training:
            eps, rng = self.reparam.draw(st["reparam"], B, N)
            eps = torch.from_numpy(eps).to(x.device)
        else:
            eps, rng = None, st["reparam"]["rng"]
        enc = h.encode(x, eps, training=training)
        return enc, dict(st["reparam"], rng=rng, mu0=enc["mu"], logvar=enc["logvar"])

    def __call__(self, x, ps, st):
        h = self.handle()
        h.set_params(ps["latent"])
        enc, st_rep = self._encode(h, x, st)
        sol, st_node = self.neural_ode(enc["z0"], ps["neural_ode"], st["neural_ode"])
        series = diffeqsol_to_timeseries(sol).contiguous()
        y = h.predict(series)
        return y, dict(neural_ode=st_node, reparam=st_rep)


def construct_time_series(in_dims=37, hidden_dims=40, latent_dims=50, node_dims=20, saveat=(), **solver_kwargs):
    """_construct_time_series, experiments/src/construct.jl:230-252 (defaults: experiments/configs/physionet.yml)"""
    return LatentODE(in_dims, hidden_dims, latent_dims, node_dims, saveat, **solver_kwargs)


def glorot_latent_params(model, seed=0):
    """Lux's default init (glorot_uniform weights, zero bias) from a numpy stream for every Dense of the model:
    dict(latent=flat vector in BLOCKS order, neural_ode=flat gen_dynamics vector), float32 numpy"""
    I, H, Ld, N = model.dims
    K = 2 * Ld + 2 * I + 1
    rng = np.random.default_rng(seed)

    def dense(out, inn):
        W = ((rng.random((inn, out), dtype=np.float32) - np.float32(0.5)) * np.float32(np.sqrt(24.0 / (inn + out)))).astype(np.float32)
        return [W.ravel(), np.zeros(out, np.float32)]

    parts = []
    for out2 in (Ld, Ld, 2 * Ld):
        parts += dense(H, K) + dense(out2, H)
    parts += dense(Ld, 2 * Ld) + dense(2 * N, Ld) + dense(I, N)
    return dict(latent=np.concatenate(parts), neural_ode=glorot_chain_params(model.gen_dynamics, seed=seed + 1))


def _forward_loss(model, ps, st, batch, weights, record):
    """the forward half of the loss (construct.jl:38-55 / 57-74); with `record` it keeps what the pullback needs"""
    data, mask, dt = batch
    w_reg, w_kl = weights
    x = torch.cat([data, mask, dt], dim=2).contiguous()   # vcat(data, mask, dt), construct.jl:40
    h = model.handle()
    h.set_params(ps["latent"])
    enc, st_rep = model._encode(h, x, st)
    node = model.neural_ode
    keep = dict(x=x, h=h, enc=enc)
    if record:
        # one recorded layer forward (the pullback's own draw convention: NeuralODE.pullback)
        hn = node._bind(ps["neural_ode"], enc["z0"])
        t0, t2 = node.tspan
        kw = node.kwargs
        mode = node.regularize if st["neural_ode"]["training"] else "none"
        rng = copy.deepcopy(st["neural_ode"]["rng"])
        r01 = np.float32(rng.random(dtype=np.float32))
        t1_or_rand = np.float32(r01 * (t2 - t0) + t0) if mode == "unbiased" else r01
        fw = hn.node_forward_record_ts(enc["z0"], t0, t2, kw.get("abstol", 1e-6), kw.get("reltol", 1e-3), model.saveat, mode=mode,
                                       reg_type=node.regularize_type, t1_or_rand=t1_or_rand, maxiters=node.maxiters,
                                       save_start=kw.get("save_start", True))
        series = fw["u"].contiguous()
        st_node = dict(st["neural_ode"], nfe=fw["nfe"], reg_val=fw["reg_val"], rng=rng if mode != "none" else st["neural_ode"]["rng"])
        keep.update(hn=hn)
    else:
        sol, st_node = node(enc["z0"], ps["neural_ode"], st["neural_ode"])
        series = diffeqsol_to_timeseries(sol).contiguous()
    head = h.decode_loss(series, data.contiguous(), mask.contiguous(), enc["mu"], enc["logvar"], w_kl, want_grads=record)
    reg_val = np.float32(st_node["reg_val"]) if node.regularize != "none" else np.float32(0.0)
    loss = np.float32(head["loss"] + np.float32(w_reg) * reg_val) if node.regularize != "none" else head["loss"]
    st_ = dict(neural_ode=st_node, reparam=st_rep)
    stats = dict(neg_log_likelihood=head["neg_log_likelihood"], kl_div=head["kl_div"], loss=loss, nfe=st_node["nfe"], reg_val=reg_val)
    keep.update(head=head, series=series)
    return loss, st_, stats, keep


def latent_ode_loss(model, ps, st, batch, weights):
    """_get_loss_function_latent_ode, construct.jl:36-76: batch = (data, mask, dt) with data / mask (B, T, in_dims) and
    dt (B, T, 1); weights = (w_reg, w_kl).  Returns (loss, st_, stats) with stats = (neg_log_likelihood, kl_div, loss, nfe,
    reg_val) as construct.jl:52-54 / 71-73."""
    loss, st_, stats, _ = _forward_loss(model, ps, st, batch, weights, record=False)
    return loss, st_, stats


def run_latent_training_step(model, ps, st, batch, weights):
    """One forward + pullback of latent_ode_loss (experiments/src/utils.jl:104-123).  Returns (loss, st_, stats, grads, times):
    grads = dict(latent=flat cotangent in BLOCKS order, neural_ode=...), times = dict(fwd_time, bwd_time, opt_time) in seconds
    (wall, synchronised; the optimiser update is the caller's: opt_time = 0)."""
    w_reg, _ = weights
    torch.cuda.synchronize()
    tic = time.perf_counter()
    loss, st_, stats, keep = _forward_loss(model, ps, st, batch, weights, record=True)
    torch.cuda.synchronize()
    fwd_time = time.perf_counter() - tic
    tic = time.perf_counter()
    head, h = keep["head"], keep["h"]
    bw = keep["hn"].node_backward_recorded_ts(head["dseries"], w_reg=float(w_reg) if model.neural_ode.regularize != "none" else 0.0)
    eb = h.encode_backward(keep["x"], dz0=bw["dx"].contiguous(), dmu=head["dmu"], dlogvar=head["dlogvar"], want_dx=False)
    torch.cuda.synchronize()
    bwd_time = time.perf_counter() - tic
    grads = dict(latent=torch.cat([eb["dp"], head["dpg"]]), neural_ode=bw["dp"])
    return loss, st_, stats, grads, dict(fwd_time=fwd_time, bwd_time=bwd_time, opt_time=0.0, adjoint=bw["stats_bwd"])
