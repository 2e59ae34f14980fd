"""Variational bottlenecks on the GPU (csrc/variational.hip through
nnx_ppo_amd.networks.variational): sequence replay forward / backward against the fp64
restatement of tests/test_variational.py, bit-identity of rollout steps and replay, the
reference's variational_test.py / ar1_rollout_test.py contracts, and the layers inside the
PPO / distillation / checkpoint / sharding machinery.

Noise bound: the kernels draw eps = random.unit_normal(key, (L,)) with logf and cospif(2 u2);
the CPU draw evaluates cos(fl(2 pi) u2) in fp32, whose rounded argument alone moves the result by
up to ~2.5e-6 at |sqrt(-2 ln u1)| <= 5.8.  The tests allow |eps_gpu - eps_cpu| <=
EPS_ATOL + EPS_RTOL |eps| and then compare everything else against the restatement evaluated on
the kernel's own eps (saved by the forward for the backward), z / reg at rel <= 1e-5 and
gradients at rel <= 1e-4 (max-norm relative errors)."""
import math

import numpy as np
import pytest
import torch

from nnx_ppo_amd import random as rnd
from oracle import networks as on
from oracle import ppo as op
from oracle import keys as okeys
from test_variational import VBTwin, twin_scan

pytestmark = pytest.mark.gpu
D = torch.float64
EPS_ATOL, EPS_RTOL = 4e-6, 1e-6


def _rel(a, b):
    a, b = a.detach().cpu().to(D), b.detach().cpu().to(D)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _bits_equal(a, b):
    if a.dtype == torch.float32:
        return torch.equal(a.view(torch.int32), b.view(torch.int32))
    return torch.equal(a, b)


def _vb(L, seed=5, ar1=True, **kw):
    from nnx_ppo_amd.networks import variational as V
    from nnx_ppo_amd.networks.types import Rngs

    cls = V.AR1VariationalBottleneck if ar1 else V.VariationalBottleneck
    return cls(L, Rngs(seed), **kw)


def _inputs(dev, T, B, L, seed, p_done=0.2):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(T, B, 2 * L, generator=g, device=dev)
    done = torch.rand(T, B, generator=g, device=dev) < p_done
    lz = torch.randn(B, L, generator=g, device=dev)
    lz[torch.rand(B, L, generator=g, device=dev) < 0.3] = math.nan
    lz[torch.rand(B, generator=g, device=dev) < 0.3] = math.nan
    g_z = torch.randn(T, B, L, generator=g, device=dev)
    return x, done, lz, g_z


MODES = [("vb", False, True), ("ar1", True, True), ("ar1_nobptt", True, False)]


@pytest.mark.parametrize("L", [1, 4, 33, 64, 100, 512])
@pytest.mark.parametrize("B", [1, 37, 1024, 4099])
@pytest.mark.parametrize("T", [1, 7, 30])
def test_replay_forward_backward_vs_restatement(dev, T, B, L):
    """Rows are independent: the kernels run the whole batch, the fp64 restatement checks up
    to 48 of its rows (first, last and a spread between)."""
    rows = torch.unique(torch.linspace(0, B - 1, min(B, 48)).round().long())
    for name, ar1, bptt in MODES:
        kw = dict(ar1_weight=1.3, backprop_through_time=bptt) if ar1 else {}
        vb = _vb(L, seed=T + B + L, ar1=ar1, kl_weight=0.7, min_std=1e-3, **kw)
        vb.to(dev)
        x, done, lz, g_z = _inputs(dev, T, B, L, seed=T * 7919 + B * 31 + L)
        st = vb.initialize_state(B)
        if ar1:
            st = {"keys": st["keys"], "last_z": lz}
        ctx, z, reg, fs = vb.replay(st, x, done, None)
        g_reg = 0.37
        g_x = vb.replay_backward(ctx, g_z, g_reg)
        eps = ctx[1]
        # eps: the CPU draw of the same keys, within the stated bound
        keys = (st["keys"] if ar1 else st)[rows].cpu()
        k = keys
        for t in range(T):
            want = rnd.unit_normal(k, (L,))
            got = eps[t, rows].cpu()
            assert ((got - want).abs() <= EPS_ATOL + EPS_RTOL * want.abs()).all(), (name, t)
            k = rnd.split(k)[..., 0]
        # everything else: fp64 restatement on the kernel's eps
        twin = VBTwin.of(vb)
        xs = x[:, rows].cpu().to(D).requires_grad_(True)
        st_c = {"keys": keys, "last_z": lz[rows].cpu().to(D)} if ar1 else keys
        z_w, reg_w, fs_w = twin_scan(twin, st_c, xs, done[:, rows].cpu(),
                                     noise_seq=eps[:, rows].cpu().to(D))
        assert _rel(z[:, rows], z_w) <= 1e-5, name
        assert _rel(reg[:, rows], reg_w) <= 1e-5, name
        (gx_w,) = torch.autograd.grad((z_w * g_z[:, rows].cpu().to(D)).sum()
                                      + g_reg * reg_w.sum(), xs)
        assert torch.isfinite(g_x).all()
        assert _rel(g_x[:, rows], gx_w) <= 1e-4, name
        if ar1:
            assert torch.equal(fs["keys"][rows].cpu(), fs_w["keys"])
            lz_w = fs_w["last_z"]
            assert torch.equal(torch.isnan(fs["last_z"][rows].cpu()), torch.isnan(lz_w))
            ok = ~torch.isnan(lz_w)
            assert _rel(fs["last_z"][rows].cpu()[ok], lz_w[ok]) <= 1e-5 if ok.any() else True
        else:
            assert torch.equal(fs[rows].cpu(), fs_w)


@pytest.mark.parametrize("ar1", [False, True])
@pytest.mark.parametrize("L", [3, 64, 130])
def test_single_steps_bit_identical_to_replay(dev, ar1, L):
    """T rollout calls with the reset select between them == one replay: z, reg, metrics and
    the final carry, bit for bit."""
    from nnx_ppo_amd import ops
    from nnx_ppo_amd.algorithms.rollout import tree_where

    T, B = 11, 67
    vb = _vb(L, ar1=ar1, kl_weight=0.3, ar1_weight=2.0) if ar1 else _vb(L, ar1=False,
                                                                        kl_weight=0.3)
    vb.to(dev)
    x, done, _, _ = _inputs(dev, T, B, L, seed=L, p_done=0.25)
    st0 = vb.initialize_state(B)
    st = st0
    zs, regs, kls, l2s = [], [], [], []
    for t in range(T):
        out = vb(st, x[t])
        st = tree_where(done[t], vb.reset_state(out.next_state), out.next_state)
        zs.append(out.output)
        regs.append(out.regularization_loss)
        kls.append(out.metrics["kl_divergence"])
        if ar1:
            l2s.append(out.metrics["l2_diff"])
        assert torch.equal(out.metrics["mu"], x[t, :, :L])
    ctx, z, reg, fs = vb.replay(st0, x, done, None)
    assert _bits_equal(torch.stack(zs), z)
    assert _bits_equal(torch.stack(regs), reg)
    lz0 = st0["last_z"] if ar1 else None
    r = ops.vb_seq_fwd(x, (st0["keys"] if ar1 else st0), lz0, done, want_metrics=True,
                       want_sigma=True, **vb._kw())
    assert _bits_equal(torch.stack(kls), r["kl"])
    if ar1:
        assert _bits_equal(torch.stack(l2s), r["l2"])
        assert torch.equal(st["keys"], fs["keys"])
        assert _bits_equal(st["last_z"], fs["last_z"])
    else:
        assert torch.equal(st, fs)


@pytest.mark.parametrize("ar1", [False, True])
def test_minibatch_slicing_bit_identical(dev, ar1):
    """variational_test.py:151 — replay on a gathered subset of envs == those rows of the
    full batch."""
    from nnx_ppo_amd import ops

    T, B, L = 9, 200, 40
    vb = _vb(L, ar1=ar1)
    vb.to(dev)
    x, done, lz, _ = _inputs(dev, T, B, L, seed=3)
    st = vb.initialize_state(B)
    if ar1:
        st = {"keys": st["keys"], "last_z": lz}
    _, z, reg, fs = vb.replay(st, x, done, None)
    idx = torch.randperm(B, generator=torch.Generator().manual_seed(0))[:64].to(dev)
    xg, dg = ops.gather_cols_multi([x, done], idx)
    stg = ({k: v.index_select(0, idx) for k, v in st.items()} if ar1
           else st.index_select(0, idx))
    _, zg, regg, fsg = vb.replay(stg, xg, dg, None)
    assert _bits_equal(zg, z[:, idx]) and _bits_equal(regg, reg[:, idx])
    if ar1:
        assert torch.equal(fsg["keys"], fs["keys"][idx])
        assert _bits_equal(fsg["last_z"], fs["last_z"][idx])
    else:
        assert torch.equal(fsg, fs[idx])


def test_reference_contracts(dev):
    """variational_test.py:43-150 restated: KL ~ 0 at N(0, 1), grows with the mean, kl_weight
    scales the loss, seeds differ, output shapes."""
    L, B = 16, 32
    ls = math.log(math.e - 1.0)  # softplus(ls) = 1
    x0 = torch.cat([torch.zeros(B, L), torch.full((B, L), ls)], -1).to(dev)
    vb = _vb(L, ar1=False, min_std=0.0).to(dev)
    s = vb.initialize_state(B)
    out = vb(s, x0)
    assert out.output.shape == (B, L) and out.regularization_loss.shape == (B,)
    assert out.next_state.shape == (B,) and out.next_state.dtype == torch.int64
    assert out.metrics["sigma"].shape == (B, L)
    assert out.metrics["kl_divergence"].abs().max() < 1e-5
    kls = []
    for m in (0.0, 0.5, 1.0, 2.0):
        kls.append(vb(s, x0 + torch.cat([torch.full((B, L), m), torch.zeros(B, L)], -1)
                      .to(dev)).metrics["kl_divergence"].mean().item())
    assert all(a < b for a, b in zip(kls, kls[1:]))
    x = torch.randn(B, 2 * L, device=dev)
    r1 = _vb(L, ar1=False, kl_weight=1.0).to(dev)(s, x).regularization_loss
    r10 = _vb(L, ar1=False, kl_weight=10.0).to(dev)(s, x).regularization_loss
    assert torch.allclose(r10, 10 * r1, rtol=1e-6)
    a = _vb(L, seed=1, ar1=False).to(dev)
    b = _vb(L, seed=2, ar1=False).to(dev)
    za = a(a.initialize_state(B), x).output
    zb = b(b.initialize_state(B), x).output
    assert not torch.allclose(za, zb)
    # the key chain moves on: a second call with the next state draws other noise
    o1 = a(a.initialize_state(B), x)
    assert not torch.equal(a(o1.next_state, x).output, o1.output)


def test_inside_sequential_and_partial_reset(dev):
    """variational_test.py:119 (Sequential) and ar1_rollout_test.py:104-206 (the AR1 term is
    zero right after a reset, for the reset rows only)."""
    from nnx_ppo_amd.algorithms.rollout import tree_where
    from nnx_ppo_amd.networks.containers import Sequential
    from nnx_ppo_amd.networks.feedforward import Dense
    from nnx_ppo_amd.networks.types import Rngs

    r = Rngs(0)
    L, B = 6, 10
    net = Sequential([Dense(4, 2 * L, r), _vb(L, ar1=True), Dense(L, 3, r)]).to(dev)
    st = net.initialize_state(B)
    x = torch.randn(B, 4, device=dev)
    out = net(st, x)
    assert out.output.shape == (B, 3) and out.regularization_loss.shape == (B,)
    assert out.metrics[1]["l2_diff"].abs().max() == 0  # last_z NaN at the start
    st = out.next_state
    done = torch.arange(B, device=dev) < B // 2
    st = tree_where(done, net.reset_state(st), st)
    out2 = net(st, x)
    l2 = out2.metrics[1]["l2_diff"]
    assert torch.equal(l2[: B // 2], torch.zeros(B // 2, device=dev))
    assert (l2[B // 2:] > 0).all()
    # replay of the same two steps through Sequential's generic per-layer path
    xs = torch.stack([x, x])
    ds = torch.stack([done, torch.zeros_like(done)])
    ctx, y, reg, _ = net.replay(net.initialize_state(B), xs, ds, [None, None, None])
    assert torch.allclose(y[0], out.output) and torch.allclose(y[1], out2.output)
    assert torch.allclose(reg[1], out2.regularization_loss)


def _ar1vb_net(O=5, A=1, L=8, seed=4, bptt=True, entropy_weight=1e-2, kl_weight=1e-2,
               ar1_weight=1e-1):
    """The actor of the reference's checkpoint tests (checkpointing_test.py
    `_make_ar1vb_nets`): Dense, Dense, AR1VB, Dense, sampler; MLP critic; normaliser."""
    from nnx_ppo_amd.networks import variational as V
    from nnx_ppo_amd.networks.adapter import PPOAdapter
    from nnx_ppo_amd.networks.containers import Sequential
    from nnx_ppo_amd.networks.feedforward import Dense
    from nnx_ppo_amd.networks.normalizer import Normalizer
    from nnx_ppo_amd.networks.sampling_layers import NormalTanhSampler
    from nnx_ppo_amd.networks.types import Rngs

    r = Rngs(seed)
    actor = Sequential([Dense(O, 32, r, "relu"), Dense(32, 2 * L, r),
                        V.AR1VariationalBottleneck(L, r, kl_weight=kl_weight,
                                                   ar1_weight=ar1_weight,
                                                   backprop_through_time=bptt),
                        Dense(L, 2 * A, r), NormalTanhSampler(r, entropy_weight)])
    critic = Sequential([Dense(O, 32, r, "relu"), Dense(32, 1, r)])
    return Sequential([Normalizer(O), PPOAdapter(action=actor, value=critic)])


def _twin(net):
    from nnx_ppo_amd.networks import variational as V

    norm, ad = net.layers
    act = on.Sequential([VBTwin.of(l) if isinstance(l, V.VariationalBottleneck)
                         else on.from_product(l) for l in ad.action.layers])
    return on.Sequential([on.from_product(norm), on.PPOAdapter(act, on.from_product(ad.value))])


def _env(max_steps=5):
    from nnx_ppo_amd.envs import MockEnv
    from nnx_ppo_amd.wrappers.episode_wrapper import EpisodeWrapper

    return EpisodeWrapper(MockEnv(5, 1, max_steps=max_steps), 40)


@pytest.mark.parametrize("bptt", [True, False])
def test_ppo_step_vs_oracle(dev, bptt):
    """End-to-end parity: N = 64, T = 12, fp32, 2 iterations against oracle.ppo.ppo_step on a
    twin (from_product for the standard layers, VBTwin for the bottleneck).  Loss statistics
    per iteration within 1e-3 rel; the parameter UPDATE (p - p0) of every tensor within 5e-2
    of the oracle's update in relative L2 norm."""
    from nnx_ppo_amd.algorithms import ppo
    from oracle import envs as oe

    N, T = 64, 12
    env = _env()
    net = _ar1vb_net(bptt=bptt)
    ts = ppo.new_training_state(env, net, N, 18, 1e-3, device=dev)
    p0 = [p.data.detach().cpu().clone() for p in net.parameters()]
    onet = _twin(net)
    q0 = [q.detach().clone() for q in onet.parameters()]
    oenv = oe.EpisodeWrapper(oe.MockEnv(5, 1, max_steps=5), 40)
    ots = op.new_training_state(oenv, onet, N, 18, okeys, 1e-3)
    for k in range(2):
        ts, m = ppo.ppo_step(env, ts, N, T, 0.95, 0.99, 0.2, True, False, 2, 4)
        ots, info = op.ppo_step(oenv, ots, N, T, 0.95, 0.99, 0.2, True, 2, 4, okeys)
        for name, row in (("actor", "losses/actor"), ("critic", "losses/critic"),
                          ("regularization", "losses/regularization")):
            want = info[name].numpy()
            assert np.allclose(m[row + "/mean"].item(), want.mean(), rtol=1e-3, atol=1e-6), \
                (k, name)
            assert np.allclose(m[row + "/std"].item(), want.std(), rtol=2e-2, atol=1e-6), \
                (k, name)
        assert float(info["regularization"].abs().min()) > 0
    vb_state = ts.network_states[1]["action"][2]
    ovb_state = ots.network_states[1]["action"][2]
    assert torch.equal(vb_state["keys"].cpu(), ovb_state["keys"])
    for (name, p), a, q, b in zip(net.named_parameters(), p0, onet.parameters(), q0):
        dp = p.data.detach().cpu().to(D) - a.to(D)
        dq = q.detach() - b
        assert float(dq.norm()) > 0, name
        assert float((dp - dq).norm() / dq.norm()) < 5e-2, name


def test_no_nan_over_rollout_with_resets(dev):
    """ar1_rollout_test.py:21-100, 208-260: resets every 5 steps; actions, log-likelihoods,
    values, losses, gradients and parameters stay finite."""
    from nnx_ppo_amd.algorithms import ppo, rollout

    N, T = 32, 20
    env = _env(max_steps=5)
    net = _ar1vb_net()
    ts = ppo.new_training_state(env, net, N, 3, 1e-3, device=dev)
    ns, es, ro = rollout.unroll_env(env, ts.env_states, net, ts.network_states, T,
                                    rnd.key(1, dev))
    assert bool(ro.done.any())
    for t in (ro.network_output.actions, ro.network_output.loglikelihoods,
              ro.network_output.value_estimates):
        assert torch.isfinite(t).all()
    for _ in range(2):
        ts, m = ppo.ppo_step(env, ts, N, T, 0.95, 0.99, 0.2, True, False, 2, 2)
        for k, v in m.items():
            if isinstance(v, torch.Tensor):
                assert torch.isfinite(v).all(), k
    for p in net.parameters():
        assert torch.isfinite(p.data).all() and torch.isfinite(p.grad).all()


def _cfg(iters=4):
    from nnx_ppo_amd.algorithms.config import EvalConfig, PPOConfig, TrainConfig
    from nnx_ppo_amd.algorithms.types import LoggingLevel

    return TrainConfig(
        ppo=PPOConfig(n_envs=64, rollout_length=8, total_steps=64 * 8 * iters, n_epochs=2,
                      n_minibatches=2, learning_rate=1e-3,
                      logging_level=LoggingLevel.LOSSES | LoggingLevel.GRAD_NORM),
        eval=EvalConfig(enabled=False), seed=11)


def test_train_ppo_graph_equals_eager(dev):
    """A VB network in the HIP-graph replayed iteration == the eager loop, bit for bit."""
    from nnx_ppo_amd.algorithms import ppo

    out = []
    for graph in (True, False):
        net = _ar1vb_net()
        logs = []
        ppo.train_ppo(_env(), net, _cfg(), log_fn=lambda m, s: logs.append((s, dict(m))),
                      hip_graph=graph)
        out.append((net, logs))
    (na, la), (nb, lb) = out
    for p, q in zip(na.parameters(), nb.parameters()):
        assert torch.equal(p.data, q.data)
    assert len(la) == len(lb)
    for (sa, ma), (sb, mb) in zip(la, lb):
        assert sa == sb
        for k in ma:
            if k.startswith("losses/"):
                assert torch.equal(torch.as_tensor(ma[k]), torch.as_tensor(mb[k])), k


def test_checkpoint_resume_bit_identical(dev, tmp_path):
    """AR1VBCheckpointTest: a known last_z and key chain survive the round trip, and the
    resumed run is bit-identical to the uninterrupted one."""
    from nnx_ppo_amd.algorithms import ppo
    from nnx_ppo_amd.algorithms.checkpointing import load_checkpoint, make_checkpoint_fn

    args = (64, 10, 0.95, 0.99, 0.2, True, False, 2, 2)
    env = _env(max_steps=7)
    net = _ar1vb_net(seed=5)
    ts = ppo.new_training_state(env, net, 64, 3, 1e-3, device=dev)
    for _ in range(2):
        ts, _ = ppo.ppo_step(env, ts, *args)
    saved = {k: v.clone() for k, v in ts.network_states[1]["action"][2].items()}
    assert not torch.isnan(saved["last_z"]).all()
    make_checkpoint_fn(str(tmp_path))(ts, step=int(ts.steps_taken))
    for _ in range(2):
        ts, m_ref = ppo.ppo_step(env, ts, *args)

    env2 = _env(max_steps=7)
    net2 = _ar1vb_net(seed=77)
    tmpl = ppo.new_training_state(env2, net2, 64, 3, 1e-3, device=dev)
    ckpt = load_checkpoint(str(tmp_path / f"step_{2 * 64 * 10:010d}"), tmpl.networks,
                           tmpl.optimizer)
    ts2 = ckpt["training_state"]
    got = ts2.network_states[1]["action"][2]
    assert torch.equal(got["keys"], saved["keys"])
    assert _bits_equal(got["last_z"], saved["last_z"])
    for _ in range(2):
        ts2, m2 = ppo.ppo_step(env2, ts2, *args)
    for p, q in zip(net.parameters(), net2.parameters()):
        assert torch.equal(p.data, q.data)
    a, b = ts.network_states[1]["action"][2], ts2.network_states[1]["action"][2]
    assert torch.equal(a["keys"], b["keys"]) and _bits_equal(a["last_z"], b["last_z"])
    for k in m_ref:
        if k.startswith("losses/"):
            assert torch.equal(torch.as_tensor(m_ref[k]), torch.as_tensor(m2[k])), k


def test_distillation_regulariser_reaches_the_loss(dev):
    """One distillation step with an AR1VB student (sampler entropy weight 0, so the whole
    regularisation loss is the bottleneck's): it is positive, and zero with zero weights."""
    from nnx_ppo_amd.algorithms import distillation
    from nnx_ppo_amd.algorithms.types import LoggingLevel

    regs = []
    for w in (1e-1, 0.0):
        env = _env()
        teacher = _ar1vb_net(seed=1)
        student = _ar1vb_net(seed=2, entropy_weight=0.0, kl_weight=w, ar1_weight=w)
        state = distillation.new_distillation_state(env, teacher, student, 16, seed=18,
                                                    device=dev)
        teacher.eval()
        before = [p.data.clone() for p in student.parameters()]
        state, m = distillation.distillation_step(env, teacher, state, 16, 6, 1, 2,
                                                  LoggingLevel.LOSSES)
        regs.append(float(torch.as_tensor(m["losses/regularization/mean"])))
        assert any(not torch.equal(a, p.data) for a, p in zip(before, student.parameters()))
    assert regs[0] > 0 and regs[1] == 0


def test_rank_fold(dev, monkeypatch):
    """new_training_state folds the rank into the VB seed (per-env keys differ between ranks);
    a network without a VB gets exactly the seeds it got before."""
    from nnx_ppo_amd import parallel
    from nnx_ppo_amd.algorithms import ppo
    from nnx_ppo_amd.networks import factories
    from nnx_ppo_amd.networks.types import Rngs

    monkeypatch.setattr(parallel, "is_distributed", lambda: True)
    monkeypatch.setattr(ppo, "Optimizer", lambda *a, **k: None)  # no communicator here
    keys, seeds = [], []
    for rank in (0, 1):
        monkeypatch.setattr(parallel, "rank", lambda rank=rank: rank)
        net = _ar1vb_net()
        ts = ppo.new_training_state(_env(), net, 16, 3, device=dev)
        keys.append(ts.network_states[1]["action"][2]["keys"].cpu())
        plain = factories.make_mlp_actor_critic(5, 1, [8], [8], Rngs(4))
        s0 = plain.layers[1].action.layers[-1].seed
        ppo.new_training_state(_env(), plain, 16, 3, device=dev)
        assert not any(hasattr(m, "fold_rank") for m in plain.modules())
        seeds.append(plain.layers[1].action.layers[-1].seed)
        assert seeds[-1] == (s0 + 0x9E3779B97F4A7C15 * (1 + rank)) & (2**63 - 1)
    assert not torch.equal(keys[0], keys[1])
    assert (keys[0] != keys[1]).all()
