"""The shape envelope of the one-launch rollouts and the policy steps behind them: what the
support predicates accept (tests/test_envelope.py pins it, no GPU needed) and what the sweep of
tests/test_envelope_gpu.py runs.  Widening a predicate or adding a menu entry without extending
this file (and so the sweep) fails tests/test_envelope.py.

Trunk pairs are written (critic width, critic hidden layers after the first, actor width, actor
hidden layers after the first), as in the HIP menus."""

K0_MAX = 32       # observation width: 1 .. K0_MAX
A2_MAX = 16       # head width 2A: 2, 4, .., A2_MAX (A <= 8)
FRONT_K0_MAX = 8  # the GRU sequence launch takes the relu Dense in front for K0 <= 8

# trunk_ws_fwd.h WS_DUAL_MENU: mi_policy_ws_dual_supported / mi_rollout_mock_ws_supported
WS_DUAL_PAIRS = [
    (256, 1, 64, 3), (256, 1, 64, 2), (256, 1, 64, 1), (256, 1, 256, 1), (256, 0, 256, 0),
    (128, 1, 128, 1), (128, 2, 128, 2), (128, 1, 64, 1), (64, 1, 64, 1), (64, 2, 64, 2),
    (64, 3, 64, 3),
]
C2_PAIR = (256, 1, 64, 3)   # BASELINE configs[1]: actor [64] * 4, critic [256] * 2

# trunk_ws.hip GRU_STEP_MENU: (critic width, critic hidden layers after the first, GRU width)
GRU_STEP_ENTRIES = [(256, 1, 64), (256, 1, 128), (256, 0, 64), (128, 1, 64), (128, 1, 128),
                    (64, 1, 64)]

# the observation widths the rollout sweeps run: both ends, the MFMA k-chunk edges (8, 16) and
# their neighbours, and 32, where one thread stages the k = 0 elements of two rows
K0_SWEEP = [1, 2, 7, 8, 9, 15, 16, 17, 31, 32]
EDGES = [(32, 8), (1, 1)]   # (K0, A) corners every instantiation runs at

# the GRU front fusion: (T, B, H, N_out) of tests/test_envelope_gpu.py's case, and its K0s
FRONT_CASE = (30, 256, 64, 2)
FRONT_K0S = [1, 8, 9]


def hidden(pair):
    """(actor hidden widths, critic hidden widths) of a WS_DUAL_PAIRS entry."""
    hv, nhv, ha, nha = pair
    return [ha] * (nha + 1), [hv] * (nhv + 1)


def accepted_mlp(K0, A2, pair):
    """What mi_rollout_mock_ws_supported / mi_policy_ws_dual_supported must accept."""
    return 1 <= K0 <= K0_MAX and 2 <= A2 <= A2_MAX and A2 % 2 == 0 and pair in WS_DUAL_PAIRS


def accepted_gru(K0, A2, entry):
    """What mi_gru_policy_step_supported must accept."""
    return 1 <= K0 <= K0_MAX and 2 <= A2 <= A2_MAX and A2 % 2 == 0 and entry in GRU_STEP_ENTRIES


def accepted_front(K0):
    """What mi_gru_seq_front_supported must accept at FRONT_CASE."""
    return 1 <= K0 <= FRONT_K0_MAX


def swept_mlp():
    """Every (K0, A2, pair) the GPU sweep runs through the one-launch MLP rollout."""
    out = {(K0, 2, C2_PAIR) for K0 in K0_SWEEP}
    out |= {(K0, 2 * A, p) for p in WS_DUAL_PAIRS for K0, A in EDGES}
    return out


def swept_gru():
    out = {(K0, 2, (256, 1, 64)) for K0 in K0_SWEEP}
    out |= {(K0, 2 * A, e) for e in GRU_STEP_ENTRIES for K0, A in EDGES}
    return out
