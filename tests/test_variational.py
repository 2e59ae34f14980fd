"""Variational bottlenecks (nnx_ppo/networks/variational.py) — host-side contract and the
fp64 restatement both layers are checked against.

`VBTwin` restates `VariationalBottleneck` / `AR1VariationalBottleneck` single-step semantics
in fp64 on CPU tensors (an `oracle.networks.Module`, so it drops into the oracle's Sequential
and PPO loop), with eps drawn by `nnx_ppo_amd.random.unit_normal` from the same int64 keys and
the AR1 term written with `torch.where` as variational.py:179 writes it.  The CPU tests here pin
the hand-written backward formula the kernels implement (`vb_backward_formula`) against fp64
autograd of that restatement before any kernel runs; tests/test_variational_gpu.py checks the
kernels against both."""
import math

import numpy as np
import pytest
import torch

from nnx_ppo_amd import random as rnd
from nnx_ppo_amd.networks import variational as V
from nnx_ppo_amd.networks.types import Rngs
from oracle import networks as on

D = torch.float64


class VBTwin(on.Module):
    """fp64 restatement of variational.py:35-81 (ar1=False) and 137-216 (ar1=True).
    `noise`: optional callable(keys [B]) -> eps [B, L] replacing the unit_normal draw."""

    def __init__(self, latent_size, seed, kl_weight=1.0, min_std=1e-6, ar1=False,
                 ar1_weight=1.0, backprop_through_time=True, dtype=D):
        self.L, self.seed, self.ar1 = latent_size, seed, ar1
        self.kl_weight, self.min_std = kl_weight, min_std
        self.ar1_weight, self.bptt = ar1_weight, backprop_through_time
        self.dtype = dtype
        self.noise = None

    @classmethod
    def of(cls, m, dtype=D):
        return cls(m.latent_size, m.seed, m.kl_weight, m.min_std, m._AR1,
                   getattr(m, "ar1_weight", 1.0), getattr(m, "backprop_through_time", True),
                   dtype)

    def initialize_state(self, batch_size):
        keys = rnd.split(rnd.key(self.seed), batch_size)
        if not self.ar1:
            return keys
        return {"keys": keys, "last_z": torch.full((batch_size, self.L), math.nan,
                                                   dtype=self.dtype)}

    def reset_state(self, prev):
        if not self.ar1:
            return prev
        return {"keys": prev["keys"], "last_z": torch.full_like(prev["last_z"], math.nan)}

    def __call__(self, state, x, extras=None):
        keys = state["keys"] if self.ar1 else state
        x = x.to(self.dtype)
        L = self.L
        mean, log_std = x[..., :L], x[..., L:]
        std = torch.nn.functional.softplus(log_std) + self.min_std
        if self.noise is not None:
            eps = self.noise(keys).to(self.dtype)
        else:
            eps = rnd.unit_normal(keys.cpu(), (L,)).to(self.dtype)
        z = mean + std * eps
        kl = (0.5 * (mean ** 2 + std ** 2 - 2 * torch.log(std) - 1)).sum(-1)
        reg = self.kl_weight * kl
        metrics = {"mu": mean, "sigma": std, "kl_divergence": kl}
        next_keys = rnd.split(keys)[..., 0]
        if not self.ar1:
            return on.Out(next_keys, z, reg, metrics)
        prev_z = state["last_z"].to(self.dtype)
        if not self.bptt:
            prev_z = prev_z.detach()
        safe_prev_z = torch.where(torch.isnan(prev_z), z, prev_z)
        l2 = ((z - safe_prev_z) ** 2).mean(-1)
        metrics["l2_diff"] = l2
        return on.Out({"keys": next_keys, "last_z": z}, z, reg + self.ar1_weight * l2, metrics)


def twin_scan(twin, state0, x_seq, done_seq, noise_seq=None):
    """T steps of the twin as the loss scan runs them (ppo.py:411-431): `done[t]` resets the
    carry after step t.  Returns (z [T,B,L], reg [T,B], final state)."""
    state = state0
    zs, regs = [], []
    for t in range(x_seq.shape[0]):
        if noise_seq is not None:
            twin.noise = lambda k, t=t: noise_seq[t]
        out = twin(state, x_seq[t])
        reset = twin.reset_state(out.next_state)
        d = done_seq[t]
        if twin.ar1:
            state = {"keys": out.next_state["keys"],
                     "last_z": torch.where(d[:, None], reset["last_z"],
                                           out.next_state["last_z"])}
        else:
            state = out.next_state
        zs.append(out.output)
        regs.append(out.regularization_loss)
    twin.noise = None
    return torch.stack(zs), torch.stack(regs), state


def vb_backward_formula(x, eps, z, last_z0, done, g_z, g_reg, kl_w, ar1_w, min_std, ar1, bptt):
    """The backward the kernels implement (csrc/variational.hip), written out in torch:
        a_t    = g_reg ar1_w (2/L) (z_t - p_t) v_t
        dz_t   = g_z_t + a_t - [bptt] a_{t+1}
        dmean  = dz_t + g_reg kl_w mean
        dsigma = dz_t eps + g_reg kl_w (sigma - 1/sigma),  dlogstd = dsigma sigmoid(log_std)"""
    T, B, L2 = x.shape
    L = L2 // 2
    mean, ls = x[..., :L], x[..., L:]
    s = torch.nn.functional.softplus(ls) + min_std
    dz = g_z.clone()
    if ar1:
        nan = torch.full((1, B, L), math.nan, dtype=x.dtype)
        p0 = nan if last_z0 is None else last_z0[None].to(x.dtype)
        p = torch.cat([p0, torch.where(done[:-1, :, None], nan, z[:-1])], 0)
        a = torch.where(torch.isnan(p), torch.zeros_like(z), g_reg * ar1_w * (2.0 / L) * (z - p))
        dz = dz + a
        if bptt:
            dz[:-1] = dz[:-1] - a[1:]
    dmean = dz + g_reg * kl_w * mean
    dsig = dz * eps + g_reg * kl_w * (s - 1 / s)
    return torch.cat([dmean, dsig * torch.sigmoid(ls)], -1)


def _rand_case(T, B, L, seed, p_done=0.2, last_z=True):
    g = np.random.default_rng(seed)
    x = torch.tensor(g.normal(size=(T, B, 2 * L)), dtype=torch.float32)
    done = torch.tensor(g.random((T, B)) < p_done)
    lz = torch.tensor(g.normal(size=(B, L)), dtype=torch.float32)
    if last_z:
        lz[torch.tensor(g.random((B, L)) < 0.3)] = math.nan  # element-wise NaN as well
        lz[0] = math.nan
    g_z = torch.tensor(g.normal(size=(T, B, L)), dtype=torch.float32)
    return x, done, lz, g_z


def test_state_shapes_dtypes_values():
    vb = V.VariationalBottleneck(4, Rngs(3))
    s = vb.initialize_state(6)
    assert s.shape == (6,) and s.dtype == torch.int64
    assert torch.equal(s, rnd.split(rnd.key(vb.seed), 6))
    assert vb.reset_state(s) is s
    ar = V.AR1VariationalBottleneck(5, Rngs(3))
    st = ar.initialize_state(7)
    assert set(st) == {"keys", "last_z"}
    assert st["keys"].shape == (7,) and st["keys"].dtype == torch.int64
    assert st["last_z"].shape == (7, 5) and st["last_z"].dtype == torch.float32
    assert torch.isnan(st["last_z"]).all()
    assert torch.equal(st["keys"], rnd.split(rnd.key(ar.seed), 7))


def test_reset_keeps_keys_and_sets_last_z_nan():
    ar = V.AR1VariationalBottleneck(3, Rngs(1))
    st = {"keys": torch.arange(4, dtype=torch.int64) * 977,
          "last_z": torch.randn(4, 3)}
    r = ar.reset_state(st)
    assert r["keys"] is st["keys"]
    assert torch.isnan(r["last_z"]).all() and r["last_z"].shape == (4, 3)
    assert r["last_z"].dtype == torch.float32
    # read-only cached constant: the same tensor on every call
    assert ar.reset_state(st)["last_z"] is r["last_z"]


def test_constructor_validation():
    with pytest.raises(ValueError):
        V.VariationalBottleneck(0, Rngs(0))
    with pytest.raises(ValueError, match="512"):
        V.AR1VariationalBottleneck(V.MAX_LATENT + 1, Rngs(0))
    with pytest.raises(TypeError):
        V.VariationalBottleneck(4.0, Rngs(0))
    with pytest.raises(TypeError):
        V.VariationalBottleneck(4, 0)
    with pytest.raises(ValueError):
        V.VariationalBottleneck(4, Rngs(0), min_std=-1.0)
    with pytest.raises(ValueError):
        V.AR1VariationalBottleneck(4, Rngs(0), ar1_weight=math.inf)
    with pytest.raises(TypeError):
        V.AR1VariationalBottleneck(4, Rngs(0), backprop_through_time=1)
    m = V.AR1VariationalBottleneck(V.MAX_LATENT, Rngs(0), kl_weight=0.5, min_std=1e-3,
                                   ar1_weight=2.0, backprop_through_time=False)
    assert (m.latent_size, m.kl_weight, m.min_std, m.ar1_weight, m.backprop_through_time) == \
        (512, 0.5, 1e-3, 2.0, False)


def test_no_advance_rng_and_rank_fold():
    """The VB is no sampler (checkpointing and ppo duck-type samplers by `advance_rng`); the
    rank hook gives every rank its own seed and is idempotent."""
    vb = V.AR1VariationalBottleneck(4, Rngs(5))
    assert not hasattr(vb, "advance_rng")
    s_plain = vb.seed
    vb.fold_rank(0)
    s0 = vb.seed
    vb.fold_rank(1)
    s1 = vb.seed
    vb.fold_rank(1)
    assert vb.seed == s1 and len({s_plain, s0, s1}) == 3
    keys1 = vb.initialize_state(8)["keys"]
    vb.fold_rank(0)
    assert not torch.equal(vb.initialize_state(8)["keys"], keys1)


def test_seed_drawn_from_rngs_once():
    a = V.VariationalBottleneck(4, Rngs(9))
    b = V.VariationalBottleneck(4, Rngs(9))
    c = V.VariationalBottleneck(4, Rngs(10))
    assert a.seed == b.seed != c.seed
    assert torch.equal(a.initialize_state(3), a.initialize_state(3))


@pytest.mark.parametrize("ar1,bptt", [(False, True), (True, True), (True, False)])
@pytest.mark.parametrize("T,B,L", [(1, 3, 1), (5, 4, 3), (9, 6, 7)])
def test_backward_formula_matches_fp64_autograd(ar1, bptt, T, B, L):
    x32, done, lz, g_z32 = _rand_case(T, B, L, seed=T * 100 + L)
    twin = VBTwin(L, seed=11, kl_weight=0.7, min_std=1e-3, ar1=ar1, ar1_weight=1.3,
                  backprop_through_time=bptt)
    st0 = twin.initialize_state(B)
    if ar1:
        st0 = {"keys": st0["keys"], "last_z": lz.to(D)}
    x = x32.to(D).requires_grad_(True)
    z, reg, _ = twin_scan(twin, st0, x, done)
    g_z, g_reg = g_z32.to(D), 0.37
    (gx_auto,) = torch.autograd.grad((z * g_z).sum() + g_reg * reg.sum(), x)
    keys = st0["keys"] if ar1 else st0
    eps = []
    for _ in range(T):
        eps.append(rnd.unit_normal(keys, (L,)).to(D))
        keys = rnd.split(keys)[..., 0]
    gx = vb_backward_formula(x.detach(), torch.stack(eps), z.detach(),
                             lz.to(D) if ar1 else None, done, g_z, g_reg, 0.7, 1.3, 1e-3, ar1,
                             bptt)
    assert torch.isfinite(gx_auto).all()
    assert torch.allclose(gx, gx_auto, rtol=1e-10, atol=1e-12)


def test_twin_ar1_semantics():
    """The restatement itself: l2 is zero where last_z is NaN (element-wise), KL at N(0, 1)
    is ~0, reset sets last_z to NaN and keeps the key chain."""
    twin = VBTwin(3, seed=2, ar1=True, min_std=0.0)
    st = twin.initialize_state(2)
    ls = math.log(math.e - 1)  # softplus(ls) = 1
    x = torch.tensor([[0.0, 0.0, 0.0, ls, ls, ls]] * 2, dtype=D)
    out = twin(st, x)
    assert torch.allclose(out.metrics["kl_divergence"], torch.zeros(2, dtype=D), atol=1e-12)
    assert torch.equal(out.metrics["l2_diff"], torch.zeros(2, dtype=D))
    st2 = dict(out.next_state)
    st2["last_z"] = st2["last_z"].clone()
    st2["last_z"][0, 1] = math.nan
    out2 = twin(st2, x)
    z2, p = out2.output[0], out.output[0]
    want = ((z2[0] - p[0]) ** 2 + (z2[2] - p[2]) ** 2) / 3
    assert torch.allclose(out2.metrics["l2_diff"][0], want)
    r = twin.reset_state(out2.next_state)
    assert torch.isnan(r["last_z"]).all() and torch.equal(r["keys"], out2.next_state["keys"])
