"""The one-launch rollouts (`mi_rollout_mock_ws_bf16`, `mi_rollout_mock_gru_ws_bf16`,
csrc/rollout_ws.hip) and the fused launches around them across the shape envelope their
support predicates accept (tests/_envelope.py; tests/test_envelope.py pins the predicates to
it), not only at obs = 5, act = 1.  Every case has two references:

  (i) the stepwise rollout (`FUSED_ROLLOUT = False`): every leaf bit-identical, the fused
      launch asserted from the C-ABI call record;
 (ii) the oracle (oracle/envs.py, oracle/keys.py; oracle/networks.py + oracle/ppo.py for the
      losses and gradients), which shares none of the kernels' index arithmetic.  The env
      ignores actions, so observations, flags and the carried env state (key, step count,
      wrapper counter) must equal the oracle env's stepped directly, bit for bit.

K0 = 32 is where a thread of the 512-thread tile stages the k = 0 elements of two rows; the
rollouts once published only one of them, so half the envs of every tile replayed one step.
Bars for the bf16 numerics are the suite's (tests/test_bf16_gpu.py)."""
import numpy as np
import pytest
import torch

from _envelope import (C2_PAIR, EDGES, FRONT_CASE, FRONT_K0S, GRU_STEP_ENTRIES, K0_SWEEP,
                       WS_DUAL_PAIRS, hidden)
from test_rollout_fused_gpu import _make, _same_tree

pytestmark = pytest.mark.gpu
D = torch.float64
MLP_LAUNCH, GRU_LAUNCH = "mi_rollout_mock_ws_bf16", "mi_rollout_mock_gru_ws_bf16"


def _rollouts(dev, monkeypatch, make, T, launch, n_roll=2):
    """`n_roll` rollouts in a row, fused and stepwise; asserts (i) and returns the fused run's
    initial env state and [(net_state, env_state, Transition, reset key)] per rollout."""
    from nnx_ppo_amd import _lib, config
    from nnx_ppo_amd import random as rnd
    from nnx_ppo_amd.algorithms.rollout import unroll_env
    from nnx_ppo_amd.networks import policy

    out = []
    with config.use_compute_dtype("bf16"):
        for fused in (True, False):
            monkeypatch.setattr(policy, "FUSED_ROLLOUT", fused)
            env, net, ts = make()
            s0 = ts.env_states   # the initial env state, cloned before anything steps it
            init = dict(key=s0.data["key"].clone(), step_count=s0.data["step_count"].clone(),
                        step_counter=s0.info["step_counter"].clone(), obs=s0.obs.clone())
            key = rnd.key(4321, device=dev)
            net_state, env_state = ts.network_states, ts.env_states
            res = []
            for it in range(n_roll):
                k = rnd.fold_in(key, it)
                with _lib.profiler as prof:
                    net_state, env_state, tr = unroll_env(env, env_state, net, net_state, T, k)
                used = {name for name, *_ in prof.records}
                assert (launch in used) == fused, used
                res.append((net_state, env_state, tr, k))
            out.append((init, res))
    (init, ra), (_, rb) = out
    assert _same_tree([r[:3] for r in ra], [r[:3] for r in rb]) >= n_roll * 18
    return init, ra


def _oracle_events(init, rolls, K0, A, max_steps, max_len, T):
    """(ii): the oracle's EpisodeWrapper(MockEnv) stepped with the oracle's reset keys."""
    from oracle import envs as oe
    from oracle import keys as okeys
    from oracle import ppo as op

    oenv = oe.EpisodeWrapper(oe.MockEnv(K0, A, max_steps=max_steps), max_len)
    c = lambda x: x.detach().cpu()
    N = init["obs"].shape[0]
    st = oe.State(data={"key": c(init["key"]), "step_count": c(init["step_count"])},
                  obs=c(init["obs"]), reward=torch.zeros(N), done=torch.zeros(N), metrics={},
                  info={"step_counter": c(init["step_counter"]),
                        "truncated": torch.zeros(N, dtype=torch.bool)})
    for r, (_, env_state, tr, k) in enumerate(rolls):
        keys_tb = okeys.split(c(k), (T, N))
        for t in range(T):
            nxt = oenv.step(st, None)
            done = nxt.done != 0
            where = f"rollout {r} step {t}"
            assert torch.equal(c(tr.obs[t]), st.obs), where
            assert torch.equal(c(tr.next_obs[t]), nxt.obs), where
            assert torch.equal(c(tr.done[t]), done), (where, int((c(tr.done[t]) != done).sum()))
            assert torch.equal(c(tr.truncated[t]), nxt.info["truncated"]), where
            assert torch.equal(c(tr.rewards[t]), nxt.reward), where
            st = op.tree_where(done, oenv.reset(keys_tb[t]), nxt)
        bad = (c(env_state.data["step_count"]) != st.data["step_count"]).nonzero().flatten()
        assert bad.numel() == 0, (f"rollout {r}: step_count differs in {bad.numel()} envs",
                                  bad[:16].tolist())
        assert torch.equal(c(env_state.data["key"]), st.data["key"]), r
        assert torch.equal(c(env_state.info["step_counter"]), st.info["step_counter"]), r
        assert torch.equal(c(env_state.obs), st.obs), r
        if max_steps < T or max_len <= T:   # every env ended an episode in this rollout
            never = (~c(tr.done).any(0)).nonzero().flatten()
            assert never.numel() == 0, (f"rollout {r}: {never.numel()} envs never done",
                                        never[:16].tolist())


def _mlp_case(dev, monkeypatch, K0, A, pair, N, T, max_steps, max_len):
    actor_h, critic_h = hidden(pair)
    make = lambda: _make(actor_h, critic_h, N, 29, max_steps, max_len, dev, obs=K0, act=A)
    init, rolls = _rollouts(dev, monkeypatch, make, T, MLP_LAUNCH)
    assert rolls[0][2].obs.shape == (T, N, K0)
    assert rolls[0][2].network_output.actions.shape == (T, N, A)
    _oracle_events(init, rolls, K0, A, max_steps, max_len, T)


# ---- a. the MLP one-launch rollout across the observation width ------------------------------
@pytest.mark.parametrize("K0", K0_SWEEP)
def test_mlp_rollout_obs_width(dev, monkeypatch, K0):
    """C2's trunk pair, reset-heavy (max_len < max_steps < T), a ragged last tile (N = 100)."""
    _mlp_case(dev, monkeypatch, K0, 1, C2_PAIR, N=100, T=9, max_steps=6, max_len=5)


# ---- b. every instantiation of the MLP rollout at the corners of (K0, A) ----------------------
@pytest.mark.parametrize("K0,A", EDGES)
@pytest.mark.parametrize("pair", WS_DUAL_PAIRS)
def test_mlp_rollout_every_pair(dev, monkeypatch, pair, K0, A):
    """More tiles than workgroups (N = 9000); the inner env ends every 2 steps."""
    _mlp_case(dev, monkeypatch, K0, A, pair, N=9000, T=4, max_steps=2, max_len=7)


@pytest.mark.parametrize("pair", [C2_PAIR, (64, 2, 64, 2), (128, 1, 128, 1), (256, 1, 256, 1)])
def test_mlp_ppo_step_at_the_edge_vs_oracle(dev, pair):
    """A whole `ppo_step` (one-launch rollout included) at K0 = 32, A = 8 against the fp64
    oracle's: events exact, loss means at the suite's bf16 bars."""
    from nnx_ppo_amd import _lib, config
    from nnx_ppo_amd.algorithms import ppo
    from oracle import envs as oe
    from oracle import keys as okeys
    from oracle import networks as on
    from oracle import ppo as op

    K0, A = EDGES[0]
    N, T = 256, 12
    actor_h, critic_h = hidden(pair)
    with config.use_compute_dtype("bf16"):
        env, net, ts = _make(actor_h, critic_h, N, 31, 5, 4, dev, obs=K0, act=A)
        oenv = oe.EpisodeWrapper(oe.MockEnv(K0, A, max_steps=5), 4)
        onet = on.from_product(net)
        ots = op.new_training_state(oenv, onet, N, 31, okeys, 1e-3)
        for k in range(2):
            with _lib.profiler as prof:
                ts, m = ppo.ppo_step(env, ts, N, T, 0.95, 0.99, 0.2, True, False, 1, 2)
            assert MLP_LAUNCH in {name for name, *_ in prof.records}
            ots, info = op.ppo_step(oenv, ots, N, T, 0.95, 0.99, 0.2, True, 1, 2, okeys)
            assert torch.equal(ts.env_states.obs.cpu(), ots.env_states.obs), k
            assert torch.equal(ts.env_states.data["step_count"].cpu(),
                               ots.env_states.data["step_count"]), k
            assert torch.equal(ts.env_states.info["step_counter"].cpu(),
                               ots.env_states.info["step_counter"]), k
            a, c, r = (info[n].numpy().mean() for n in ("actor", "critic", "regularization"))
            got = [m[f"losses/{n}/mean"].item() for n in ("actor", "critic", "regularization")]
            assert np.allclose(got[0], a, rtol=5e-2, atol=3e-4), (k, got[0], a)
            assert np.allclose(got[1], c, rtol=2e-3), (k, got[1], c)
            assert np.allclose(got[2], r, rtol=5e-2, atol=1e-4), (k, got[2], r)


# ---- c. the GRU one-launch rollout ----------------------------------------------------------
def _gru_case(dev, monkeypatch, K0, A, entry, N, T, max_steps, max_len):
    """The oracle's `ppo_step` is not run on the GRU actor-critic here: the event check steps
    oracle/envs.py directly (the env ignores actions, so the events do not depend on it)."""
    from nnx_ppo_amd.algorithms import ppo
    from nnx_ppo_amd.envs import MockEnv
    from nnx_ppo_amd.networks import factories
    from nnx_ppo_amd.networks.types import Rngs
    from nnx_ppo_amd.wrappers.episode_wrapper import EpisodeWrapper

    hv, nhv, H = entry

    def make():
        env = EpisodeWrapper(MockEnv(K0, A, max_steps=max_steps), max_len)
        net = factories.make_gru_actor_critic(K0, A, H, [hv] * (nhv + 1), Rngs(13))
        return env, net, ppo.new_training_state(env, net, N, 13, 1e-3, device=dev)

    init, rolls = _rollouts(dev, monkeypatch, make, T, GRU_LAUNCH)
    h = rolls[-1][0][-1]["action"][1]     # the carry after the second rollout
    assert h.shape == (N, H)
    done_last = rolls[-1][2].done[-1]
    assert float(h[done_last].abs().sum()) == 0.0   # rows reset at the last step carry zeros
    if bool((~done_last).any()):
        assert float(h[~done_last].abs().sum()) > 0
    _oracle_events(init, rolls, K0, A, max_steps, max_len, T)


@pytest.mark.parametrize("K0", K0_SWEEP)
def test_gru_rollout_obs_width(dev, monkeypatch, K0):
    _gru_case(dev, monkeypatch, K0, 1, (256, 1, 64), N=100, T=9, max_steps=6, max_len=5)


@pytest.mark.parametrize("K0,A", EDGES)
@pytest.mark.parametrize("entry", GRU_STEP_ENTRIES)
def test_gru_rollout_every_entry(dev, monkeypatch, entry, K0, A):
    _gru_case(dev, monkeypatch, K0, A, entry, N=9000, T=4, max_steps=2, max_len=7)


# ---- d. loss gradients at the edges against fp64 autograd -----------------------------------
@pytest.mark.parametrize("K0", [1, 32])
@pytest.mark.parametrize("A", [1, 8])
def test_edge_gradients_vs_fp64_autograd(dev, K0, A):
    """One loss evaluation on a fixed [T, B] = [30, 1024] minibatch through the fused bf16
    replay and the in-backward GAE launch (`mi_policy_ws_bwd_gae_bf16` + the grouped dW),
    C2's trunks: every parameter gradient against fp64 autograd through `op.ppo_loss` on
    `on.from_product(net)`, at the suite's bf16 bar (cosine > 0.99, relative L2 < 0.15)."""
    from nnx_ppo_amd import _lib, config
    from nnx_ppo_amd.algorithms import ppo
    from nnx_ppo_amd.algorithms.types import LoggingLevel, Transition
    from nnx_ppo_amd.networks import factories
    from nnx_ppo_amd.networks.types import PPONetworkOutput, Rngs
    from nnx_ppo_amd.optim import Optimizer
    from oracle import networks as on
    from oracle import ppo as op

    T, B = 30, 1024
    actor_h, critic_h = hidden(C2_PAIR)
    net = factories.make_mlp_actor_critic(K0, A, actor_h, critic_h, Rngs(17))
    net.to(dev)
    opt = Optimizer(net, 1e-4, device=dev)
    rng = np.random.default_rng(K0 * 10 + A)
    ad = net.layers[1]
    stats = torch.tensor(rng.normal(1, 2, size=(4, 8, K0)), dtype=torch.float32, device=dev)
    net.update_statistics([stats, {"action": [None] * len(ad.action.layers),
                                   "value": [None] * len(ad.value.layers)}])
    onet = on.from_product(net)
    obs = rng.normal(size=(T, B, K0)).astype(np.float32)
    nobs = rng.normal(size=(T, B, K0)).astype(np.float32)
    raw = rng.normal(size=(T, B, A)).astype(np.float32)
    ll_old = rng.normal(-1 * A, 0.3, size=(T, B)).astype(np.float32)
    rew = rng.normal(size=(T, B)).astype(np.float32)
    done = rng.random((T, B)) < 0.15
    trunc = done & (rng.random((T, B)) < 0.5)
    g = lambda a, dt=torch.float32: torch.as_tensor(a, dtype=dt).to(dev)
    n_act, n_val = len(ad.action.layers), len(ad.value.layers)
    extras = [g(obs), {"action": [None] * (n_act - 1) + [g(raw)], "value": [None] * n_val}]
    mb = Transition(obs=g(obs), network_output=PPONetworkOutput(None, g(ll_old), None),
                    rewards=g(rew), done=g(done, torch.bool), truncated=g(trunc, torch.bool),
                    next_obs=g(nobs[-1:]), metrics={}, rollout_extras=extras)
    with config.use_compute_dtype("bf16"):
        opt.begin()
        with _lib.profiler as prof:
            ppo.ppo_loss(net, net.initialize_state(B), mb, 0.2, True, False, 0.99, 0.95, 0.5,
                         LoggingLevel.LOSSES)
        torch.cuda.synchronize()
    used = {name for name, *_ in prof.records}
    assert "mi_policy_ws_bwd_gae_bf16" in used, sorted(used)
    c = lambda a, dt=D: torch.as_tensor(a, dtype=dt)
    oextras = [c(obs), {"action": [None] * (n_act - 1) + [c(raw)], "value": [None] * n_val}]
    omb = op.Transition(obs=c(obs, torch.float32), loglikelihoods=c(ll_old), rewards=c(rew),
                        done=c(done, torch.bool), truncated=c(trunc, torch.bool),
                        next_obs=c(nobs, torch.float32), rollout_extras=oextras)
    total, _ = op.ppo_loss(onet, onet.initialize_state(B), omb, 0.2, True, 0.99, 0.95, 0.5)
    want = torch.autograd.grad(total, onet.parameters())
    named = list(net.named_parameters())
    assert len(named) == len(want)
    for (name, p), w in zip(named, want):
        got = p.grad.detach().cpu().to(D)
        assert got.shape == w.shape, (name, got.shape, w.shape)
        if float(w.norm()) == 0:
            continue
        cos = float((got * w).sum() / (got.norm() * w.norm()))
        rel = float((got - w).norm() / w.norm())
        if cos > 0.99 and rel < 0.15:
            continue
        # the edges change the first layer's K0 input columns and the head's 2A output rows:
        # name the worst of them
        detail = []
        for dim, size, what in ((0, K0, "input column"), (-1, 2 * A, "head output")):
            if w.dim() >= 1 and w.shape[dim] == size:
                err = [float((got.select(dim, i) - w.select(dim, i)).norm()
                             / max(float(w.select(dim, i).norm()), 1e-30)) for i in range(size)]
                worst = int(np.argmax(err))
                detail.append(f"{what} {worst} of {size}: rel {err[worst]:.3g}")
        pytest.fail(f"{name} {tuple(w.shape)}: cos {cos:.4f} rel {rel:.4f}; {'; '.join(detail)}")


# ---- e. the GRU front fusion at its edge ----------------------------------------------------
@pytest.mark.parametrize("K0", FRONT_K0S)
def test_gru_front_fusion_obs_width(dev, monkeypatch, K0):
    """`mi_gru_seq_fwd_front_proj_tail_bf16` (the relu Dense(K0 -> H) in front of the GRU in
    the sequence launch) against the unfused launches: parameters, moments and every metric bit
    for bit over two iterations; at K0 = 9 the front launch is not used and nothing changes."""
    from nnx_ppo_amd import _lib, config, ops
    from nnx_ppo_amd.algorithms import ppo
    from nnx_ppo_amd.envs import MockEnv
    from nnx_ppo_amd.networks import containers, factories
    from nnx_ppo_amd.networks.types import Rngs
    from nnx_ppo_amd.wrappers.episode_wrapper import EpisodeWrapper

    T, B, H, N_out = FRONT_CASE
    A, n_envs = N_out // 2, 2 * B
    fits = ops.gru_seq_front_supported(T, B, H, K0, N_out)
    assert fits == (K0 <= 8)
    out = []
    with config.use_compute_dtype("bf16"):
        for front in (True, False):
            for flag in ("REC_TAIL", "REC_TAIL_BWD", "REC_PROJ"):
                monkeypatch.setattr(containers, flag, True)
            monkeypatch.setattr(containers, "REC_FRONT", front)
            env = EpisodeWrapper(MockEnv(K0, A, max_steps=5), 1000)
            net = factories.make_gru_actor_critic(K0, A, H, [256, 256], Rngs(9))
            ts = ppo.new_training_state(env, net, n_envs, 9, 3e-4, device=dev)
            ms = []
            for it in range(2):
                with _lib.profiler as prof:
                    ts, m = ppo.ppo_step(env, ts, n_envs, T, 0.95, 0.99, 0.2, True, False, 2, 2)
                ms.append({k: float(v) for k, v in m.items()})
                used = {name for name, *_ in prof.records}
                assert ("mi_gru_seq_fwd_front_proj_tail_bf16" in used) == (front and fits), used
                assert "mi_gru_seq_bwd_proj_tail_bf16" in used, used
            out.append((ts.optimizer.params.clone(), ts.optimizer.m.clone(), ms))
    (pa, ma, la), (pb, mb, lb) = out
    assert torch.equal(pa, pb) and torch.equal(ma, mb)
    assert la == lb
