"""The MNIST-SDE experiment's model (experiments/src/construct.jl:202-210, BASELINE config 5):

    Chain(flatten, downsample = Dense(784 => 32),
          neural_dsde = NeuralDSDE(Chain(Dense(32 => 64, tanh), Dense(64 => 32)), Dense(32 => 32); reltol, abstol,
                                   save_start = false, regularize, maxiters = 10_000),
          sol_to_arr, classifier = Dense(32 => num_classes))

on the SDE handle: the downsample layer and the head run on the device (csrc/lrnde_sde_model.hpp), the layer is
`sde.NeuralDSDE`.  The training step is `training.run_sde_training_step`."""
import numpy as np
import torch

from .layers import Chain, Dense
from .sde import NeuralDSDE


def _dev(t, device):
    return torch.as_tensor(t, dtype=torch.float32).to(device).contiguous().reshape(-1)


class MlpSde:
    """`(y_pred, st_) = model(x, ps, st)`; ps = dict(downsample=, neural_dsde=dict(drift=, diffusion=), classifier=), flat
    blocks in Lux / ComponentArray order ([vec(W) column-major; b]); st = `initialstates(rng)`."""

    def __init__(self, in_dims, state_dims, hidden_dims, num_classes, neural_dsde):
        if not 1 <= int(num_classes) <= 16:
            raise ValueError("num_classes must be in 1..16 (the head's kernels, include/lrnde.h)")
        self.in_dims, self.state_dims, self.hidden_dims, self.num_classes = int(in_dims), int(state_dims), int(hidden_dims), int(num_classes)
        self.downsample = Dense(in_dims, state_dims)
        self.neural_dsde = neural_dsde
        self.classifier = Dense(state_dims, num_classes)

    def initialstates(self, rng):
        return dict(flatten={}, downsample={}, neural_dsde=self.neural_dsde.initialstates(rng), sol_to_arr={}, classifier={})

    @staticmethod
    def testmode(st, on=True):
        """Lux.testmode / Lux.trainmode: the layer regularises in training mode only (src/layers/neural_sde.jl:74-123)"""
        return dict(st, neural_dsde=dict(st["neural_dsde"], training=not on))

    def flatten(self, x):
        """FlattenLayer: (B, ...) -> (B, in_dims), contiguous float32 on the device"""
        x = x.reshape(x.shape[0], -1)
        if x.shape[1] != self.in_dims:
            raise ValueError(f"the input flattens to {x.shape[1]} values per sample, the model takes {self.in_dims}")
        return x.to(torch.float32).contiguous()

    def device_params(self, ps, device):
        """(downsample, drift, diffusion, classifier) as contiguous float32 vectors on `device`"""
        nd = ps["neural_dsde"]
        return _dev(ps["downsample"], device), _dev(nd["drift"], device), _dev(nd["diffusion"], device), _dev(ps["classifier"], device)

    def __call__(self, x, ps, st, **layer_inputs):
        x = self.flatten(x)
        pd, pf, pg, pc = self.device_params(ps, x.device)
        h = self.neural_dsde.handle()
        u0 = h.dense_forward(x, pd)
        sol, st_n = self.neural_dsde(u0, dict(drift=pf, diffusion=pg), st["neural_dsde"], **layer_inputs)
        labels = torch.zeros(x.shape[0], dtype=torch.int32, device=x.device)   # (the logits do not depend on them)
        y_pred = h.classifier_ce(sol.u[-1].contiguous(), pc, self.num_classes, labels, want_grads=False)["logits"]
        return y_pred, dict(st, neural_dsde=st_n)


def construct_mlp_sde(in_dims=784, state_dims=32, hidden_dims=64, num_classes=10, **nsde_kwargs):
    """`_construct_mlp_sde` (experiments/src/construct.jl:202-210) with its kwargs: save_start = false, maxiters = 10_000; the
    noise is drawn on the device unless the caller says otherwise"""
    kw = dict(save_start=False, maxiters=10_000, noise_source="device")
    kw.update(nsde_kwargs)
    nsde = NeuralDSDE(Chain(Dense(state_dims, hidden_dims, "tanh"), Dense(hidden_dims, state_dims)), Dense(state_dims, state_dims), **kw)
    return MlpSde(in_dims, state_dims, hidden_dims, num_classes, nsde)


def glorot_mlp_sde_params(model, seed=0):
    """Lux's default init (glorot_uniform weights, zero biases) from a numpy stream, every block flat in Lux order:
    dict(downsample=, neural_dsde=dict(drift=, diffusion=), classifier=)"""
    rng = np.random.default_rng(seed)

    def dense(inn, out):
        w = (rng.random((inn, out), dtype=np.float32) - np.float32(0.5)) * np.float32(np.sqrt(24.0 / (inn + out)))
        return np.concatenate([w.astype(np.float32).ravel(), np.zeros(out, np.float32)])   # W[o][k] at o + out * k

    Din, D, H, K = model.in_dims, model.state_dims, model.hidden_dims, model.num_classes
    return dict(downsample=dense(Din, D), neural_dsde=dict(drift=np.concatenate([dense(D, H), dense(H, D)]), diffusion=dense(D, D)),
                classifier=dense(D, K))
