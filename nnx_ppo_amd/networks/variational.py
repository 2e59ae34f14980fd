"""Variational bottlenecks (counterpart of `nnx_ppo/networks/variational.py`):
`VariationalBottleneck` (variational.py:10-89) and `AR1VariationalBottleneck` (92-216).

Input `x [B, 2L]` = `[mean | log_std]`; `sigma = softplus(log_std) + min_std`, `z = mean +
sigma * eps` with `eps ~ N(0, 1)^L` drawn from the row's carried key, and the regulariser
`kl_weight * KL(N(mean, sigma) || N(0, 1))` per row.  The AR1 form adds `ar1_weight * l2_diff`,
`l2_diff = mean_l (z - p~)^2` with `p~ = isnan(p) ? z : p` element-wise, `p` the previous z
(NaN after a reset: no AR1 term).

The carry is this port's int64 key per env (`nnx_ppo_amd.random`, in place of JAX's `[B, 2]`
key data): each call draws `eps = random.unit_normal(k, (L,))` and moves on to
`random.split(k)[..., 0]`.  Keys survive env resets.  In loss replay the stored pre-rollout
carry walks the same chain, so the replay sees the rollout's noise with the current mean and
std — the reparameterisation — and `done[t]` resets the carry after step t (`ppo.py:411-418`):
the AR1 layer's `last_z` becomes NaN, the key chain goes on.

Both the rollout call and the sequence replay run `mi_vb_seq_fwd_f32` (csrc/variational.hip;
the rollout at T = 1), so a rollout step and the replay's step agree bit for bit;
`replay_backward` is `mi_vb_seq_bwd_f32`.
"""
from __future__ import annotations

import math
from typing import Any

import torch

from .. import ops
from .. import random as rnd
from ..envs.constants import constant
from .types import Rngs, StatefulModule, StatefulModuleOutput

# largest latent size the kernels take (mi_vb_max_latent)
MAX_LATENT = 512


class VariationalBottleneck(StatefulModule):
    """variational.py:10-89 — state: int64 keys `[B]`."""

    _AR1 = False

    def __init__(self, latent_size: int, rng: Rngs, kl_weight: float = 1.0,
                 min_std: float = 1e-6):
        name = type(self).__name__
        if isinstance(latent_size, bool) or not isinstance(latent_size, int):
            raise TypeError(f"{name}: latent_size must be an int, got {latent_size!r}")
        if not 1 <= latent_size <= MAX_LATENT:
            raise ValueError(f"{name}: latent_size must be in [1, {MAX_LATENT}], got "
                             f"{latent_size}")
        if not isinstance(rng, Rngs):
            raise TypeError(f"{name}: rng must be a networks.types.Rngs, got "
                            f"{type(rng).__name__}")
        if not math.isfinite(float(kl_weight)):
            raise ValueError(f"{name}: kl_weight must be finite, got {kl_weight}")
        if not (math.isfinite(float(min_std)) and float(min_std) >= 0.0):
            raise ValueError(f"{name}: min_std must be finite and >= 0, got {min_std}")
        self.latent_size = latent_size
        self.kl_weight = float(kl_weight)
        self.min_std = float(min_std)
        # the seed of `initialize_state`'s keys, drawn once (the reference's `self.rng()`)
        self._base_seed = rng.stream_seed("default")
        self.seed = self._base_seed

    def fold_rank(self, rank: int) -> None:
        """Sharded runs: give rank `rank` its own key chains (`ppo.new_training_state` calls
        this on every module that has it, as it folds the samplers' seeds).  Idempotent: the
        seed is always derived from the one drawn at construction."""
        self.seed = (self._base_seed + 0x9E3779B97F4A7C15 * (1 + int(rank))) & (2**63 - 1)

    def _kw(self):
        return dict(kl_weight=self.kl_weight, ar1_weight=0.0, min_std=self.min_std, ar1=False)

    # -- carry layout (the AR1 form overrides these) ---------------------------------
    def _split_state(self, state):
        return state, None

    def _make_state(self, keys, last_z):
        return keys

    def _check_input(self, x: torch.Tensor) -> None:
        if x.shape[-1] != 2 * self.latent_size:
            raise ValueError(f"{type(self).__name__}: input width {x.shape[-1]} != "
                             f"2 * latent_size = {2 * self.latent_size}")

    # -- reference interface -------------------------------------------------------------
    def __call__(self, state, x: torch.Tensor, rollout_extras: Any = None) -> StatefulModuleOutput:
        self._check_input(x)
        B = x.shape[0]
        L = self.latent_size
        keys, last_z = self._split_state(state)
        x3 = x.reshape(1, B, 2 * L)
        r = ops.vb_seq_fwd(x3 if x3.is_contiguous() else x3.contiguous(), keys.contiguous(),
                           None if last_z is None else last_z.contiguous(), None,
                           want_eps=False, want_metrics=True, want_sigma=True, **self._kw())
        metrics = {"mu": x[..., :L], "sigma": r["sigma"][0], "kl_divergence": r["kl"][0]}
        if self._AR1:
            metrics["l2_diff"] = r["l2"][0]
        return StatefulModuleOutput(
            next_state=self._make_state(r["keys"], r["last_z"]),
            output=r["z"][0],
            regularization_loss=r["reg"][0],
            metrics=metrics,
            rollout_extras=None,
        )

    def initialize_state(self, batch_size: int):
        keys = rnd.split(rnd.key(self.seed, self.device), batch_size)
        return self._make_state(keys, None)

    def reset_state(self, prev_state):
        # variational.py:86-88: the key chain goes on across env resets
        return prev_state

    # -- training protocol ---------------------------------------------------------------
    def replay(self, state0, x_seq, done_seq, extras_seq, need_input_grad=True):
        self._check_input(x_seq)
        keys, last_z = self._split_state(state0)
        x = x_seq if x_seq.is_contiguous() else x_seq.contiguous()
        done = None if done_seq is None else done_seq.contiguous()
        last_z = None if last_z is None else last_z.contiguous()
        r = ops.vb_seq_fwd(x, keys.contiguous(), last_z, done, want_eps=need_input_grad,
                           **self._kw())
        ctx = (x, r["eps"], r["z"], last_z, done, need_input_grad)
        return ctx, r["z"], r["reg"], self._make_state(r["keys"], r["last_z"])

    def replay_backward(self, ctx, g_out, g_reg):
        x, eps, z, last_z, done, need_input_grad = ctx
        if not need_input_grad:  # nothing upstream trains: no launch
            return None
        g_z = None if g_out is None else (g_out if g_out.is_contiguous() else g_out.contiguous())
        return ops.vb_seq_bwd(x, eps, z, last_z, done, g_z, g_reg, bptt=self._bptt(),
                              **self._kw())

    def _bptt(self) -> bool:
        return False


class AR1VariationalBottleneck(VariationalBottleneck):
    """variational.py:92-216 — state: `{"keys": int64 [B], "last_z": fp32 [B, L]}`, last_z
    NaN at `initialize_state` and after `reset_state`."""

    _AR1 = True

    def __init__(self, latent_size: int, rng: Rngs, kl_weight: float = 1.0,
                 min_std: float = 1e-6, ar1_weight: float = 1.0,
                 backprop_through_time: bool = True):
        super().__init__(latent_size, rng, kl_weight, min_std)
        if not math.isfinite(float(ar1_weight)):
            raise ValueError(f"AR1VariationalBottleneck: ar1_weight must be finite, got "
                             f"{ar1_weight}")
        if not isinstance(backprop_through_time, bool):
            raise TypeError("AR1VariationalBottleneck: backprop_through_time must be a bool")
        self.ar1_weight = float(ar1_weight)
        self.backprop_through_time = backprop_through_time

    def _kw(self):
        return dict(kl_weight=self.kl_weight, ar1_weight=self.ar1_weight,
                    min_std=self.min_std, ar1=True)

    def _bptt(self) -> bool:
        return self.backprop_through_time

    def _split_state(self, state):
        return state["keys"], state["last_z"]

    def _make_state(self, keys, last_z):
        if last_z is None:
            last_z = torch.full((keys.shape[0], self.latent_size), math.nan,
                                dtype=torch.float32, device=keys.device)
        return {"keys": keys, "last_z": last_z}

    def reset_state(self, prev_state):
        # variational.py:210-216; read-only cached NaNs: the rollout only selects from them
        lz = prev_state["last_z"]
        return {"keys": prev_state["keys"],
                "last_z": constant(lz.shape, torch.float32, math.nan, lz.device)}
