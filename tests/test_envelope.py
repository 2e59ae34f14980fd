"""The support predicates of the one-launch rollouts and of the fused policy steps behind them
(host code, no GPU needed) accept exactly the envelope tests/_envelope.py describes — the one
tests/test_envelope_gpu.py sweeps.  A predicate widened, or a menu entry added, without the
sweep following fails here."""
import itertools

import pytest

from _envelope import (A2_MAX, C2_PAIR, EDGES, FRONT_CASE, FRONT_K0S, GRU_STEP_ENTRIES,
                       K0_MAX, WS_DUAL_PAIRS, accepted_front, accepted_gru, accepted_mlp,
                       swept_gru, swept_mlp)

K0S = range(1, 41)
A2S = range(1, 21)
WIDTHS = [32, 64, 96, 128, 256, 512]
DEPTHS = range(0, 5)   # hidden layers after the first


@pytest.fixture(scope="module")
def ops():
    from nnx_ppo_amd.csrc.build import build

    build()
    from nnx_ppo_amd import ops

    return ops


def _trunks(K0, A2, pair):
    hv, nhv, ha, nha = pair
    relu, none = 1, 0
    a_dims = [K0] + [ha] * (nha + 1) + [A2]
    c_dims = [K0] + [hv] * (nhv + 1) + [1]
    return (a_dims, [relu] * (nha + 1) + [none], c_dims, [relu] * (nhv + 1) + [none])


def _relu_none(ops):
    assert (ops.ACT_RELU, ops.ACT_NONE) == (1, 0)


CANDIDATE_PAIRS = sorted(set(itertools.product(WIDTHS, DEPTHS, WIDTHS, DEPTHS)) | set(WS_DUAL_PAIRS))


def test_mlp_pairs(ops):
    """Every candidate trunk pair at the C2 widths: exactly the menu."""
    _relu_none(ops)
    got_roll = {p for p in CANDIDATE_PAIRS if ops.rollout_mock_ws_supported(*_trunks(5, 2, p))}
    got_dual = {p for p in CANDIDATE_PAIRS if ops.policy_ws_dual_supported(*_trunks(5, 2, p))}
    assert got_roll == set(WS_DUAL_PAIRS), sorted(got_roll ^ set(WS_DUAL_PAIRS))
    assert got_dual == set(WS_DUAL_PAIRS), sorted(got_dual ^ set(WS_DUAL_PAIRS))


@pytest.mark.parametrize("pair", WS_DUAL_PAIRS)
def test_mlp_widths(ops, pair):
    """K0 in 1..40 x A2 in 1..20 for each instantiated pair: exactly the envelope."""
    wrong = []
    for K0, A2 in itertools.product(K0S, A2S):
        want = accepted_mlp(K0, A2, pair)
        got = (ops.rollout_mock_ws_supported(*_trunks(K0, A2, pair)),
               ops.policy_ws_dual_supported(*_trunks(K0, A2, pair)))
        if got != (want, want):
            wrong.append((K0, A2, got))
    assert not wrong, wrong


def test_gru_entries_and_widths(ops):
    cand = sorted(set(itertools.product(WIDTHS, DEPTHS, [32, 64, 96, 128, 256]))
                  | set(GRU_STEP_ENTRIES))
    relu, none = 1, 0
    c = lambda K0, hv, nhv: ([K0] + [hv] * (nhv + 1) + [1], [relu] * (nhv + 1) + [none])
    got = {e for e in cand if ops.gru_policy_step_supported(5, e[2], 2, *c(5, e[0], e[1]))}
    assert got == set(GRU_STEP_ENTRIES), sorted(got ^ set(GRU_STEP_ENTRIES))
    wrong = []
    for e in GRU_STEP_ENTRIES:
        for K0, A2 in itertools.product(K0S, A2S):
            got = ops.gru_policy_step_supported(K0, e[2], A2, *c(K0, e[0], e[1]))
            if got != accepted_gru(K0, A2, e):
                wrong.append((e, K0, A2, got))
    assert not wrong, wrong


def test_gru_front_widths(ops):
    T, B, H, N_out = FRONT_CASE
    got = [K0 for K0 in K0S if ops.gru_seq_front_supported(T, B, H, K0, N_out)]
    assert got == [K0 for K0 in K0S if accepted_front(K0)], got
    # the GPU case runs both ends of the front fusion and the first width past it
    assert min(got) in FRONT_K0S and max(got) in FRONT_K0S and max(got) + 1 in FRONT_K0S


def test_sweep_covers_the_envelope():
    """The GPU sweep runs every instantiation at both corners of (K0, A) and the C2 pair /
    the C2-like GRU entry at both ends of K0."""
    mlp, gru = swept_mlp(), swept_gru()
    assert (K0_MAX, A2_MAX) == (32, 16) and set(EDGES) == {(K0_MAX, A2_MAX // 2), (1, 1)}
    for p in WS_DUAL_PAIRS:
        assert {(K0, 2 * A, p) for K0, A in EDGES} <= mlp
    for e in GRU_STEP_ENTRIES:
        assert {(K0, 2 * A, e) for K0, A in EDGES} <= gru
    for K0 in (1, K0_MAX):
        assert (K0, 2, C2_PAIR) in mlp and (K0, 2, (256, 1, 64)) in gru
    assert all(accepted_mlp(*s) for s in mlp) and all(accepted_gru(*s) for s in gru)
