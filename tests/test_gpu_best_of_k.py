"""Best-of-K sampled decoding (runtime.rollout_best_of -> vrp_rollout_multi) on the MI355X.

By definition best of K on B instances is the reference's sampled eval-mode rollout on a virtual
batch of V = K B elements in which every instance appears K times (element j = k B + b), followed
by a per-instance selection.  The checker is therefore the oracle's own rollout on an OracleEnv
whose instances are tiled K times, under the protocol and the tolerances of
test_gpu_parity.py::_compare_rollout (eval mode): same host noise on both sides, every HIP choice
the oracle's up to a near tie, identical free-running sequences when nobody took a runner-up, cost
within TOL, accumulated log-prob within TOL max(1, T/4), per-step log-prob within 1e-5.  The
selection is checked exactly against the HIP run's own all_loss."""
from copy import deepcopy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-5        # tests/test_gpu_parity.py: TOL
TIE_GAP = 5e-5    # tests/test_gpu_parity.py: TIE_GAP


def _envs():
    from gym_vrp.envs import IRPEnv, TSPEnv, VRPEnv
    return {0: TSPEnv, 1: VRPEnv, 2: IRPEnv}


def _agents():
    import agents
    return {0: agents.TSPAgent, 1: agents.VRPAgent, 2: agents.IRPAgent}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import vrpgym_hip
    vrpgym_hip.require_gpu()
    yield


def _tiled(oe, K):
    """The oracle env with every instance K times: element k B + b = instance b."""
    te = deepcopy(oe)
    V = K * oe.batch_size
    te.batch_size = V
    te.pos = np.tile(oe.pos, (K, 1, 1))
    te.depots = np.tile(oe.depots, (K, 1))
    te.demands = np.tile(oe.demands, (K, 1, 1))
    te.visited = np.zeros((V, oe.num_nodes))
    te.current_location = te.depots
    if oe.kind == 2:
        te.load = np.ones(shape=(V,))
    return te


CASES = [(0, 20, 12, 5), (1, 20, 12, 5), (2, 20, 12, 5), (0, 40, 8, 16), (1, 63, 5, 12),
         (2, 100, 3, 8), (2, 40, 32, 8), (1, 40, 64, 32), (0, 20, 512, 16), (0, 5, 3, 7)]


# beyond the issue's list: TSP / VRP above 64 nodes, where the two-nodes-per-lane step kernel reads
# the first-node table row and the table kernel runs five to seven row tiles (N = 100: its largest
# LDS footprint, 16-byte stores; N = 66: element-wise stores)
EXTRA_CASES = [(1, 100, 3, 4), (0, 66, 4, 3), (0, 100, 2, 3)]


@pytest.mark.parametrize("kind,N,B,K", CASES + EXTRA_CASES)
def test_best_of_k_against_tiled_oracle(kind, N, B, K):
    from oracle import envs as oenv
    from oracle import policy as opol
    from agents import runtime
    V = K * B
    agent = _agents()[kind](seed=69)
    sd, _ = opol.init_state_dicts(kind, 69)
    model = agent.model
    model.eval()
    env = _envs()[kind](N, B, 1, 1234)
    te = _tiled(oenv.OracleEnv(kind, N, B, 1, 1234), K)
    trace = []
    torch.manual_seed(7)
    with torch.no_grad():
        ol, olp, oT = opol.rollout(sd, deepcopy(te), greedy=False, train=False, trace=trace)
    oacts = np.array([t["idx"].numpy() for t in trace])
    torch.manual_seed(7)
    with torch.no_grad():
        res = runtime.rollout_best_of(model, env, K, noise_mode="host", trace=True)
    T = res.T
    acts = res.all_actions.cpu().numpy()
    assert acts.shape == (T, V)
    Tm = min(T, oT)
    div = (acts[:Tm] != oacts[:Tm]).any(axis=0)
    forced_trace = trace
    if div.any() or T != oT:
        forced_trace = []
        torch.manual_seed(7)    # same noise stream: one (V,N) draw per step
        with torch.no_grad():
            ol, olp, oT2 = opol.rollout(sd, deepcopy(te), greedy=False, train=False,
                                        trace=forced_trace, forced=acts)
        assert oT2 == T
    U = torch.stack([st["u"] for st in forced_trace])                   # (T,V,N)
    A = torch.as_tensor(acts)[:, :, None]
    Q = torch.stack([st["noise"] for st in forced_trace])
    ratio = torch.softmax(U - U.logsumexp(-1, keepdim=True), dim=-1) / Q
    best = ratio.max(dim=2).values
    slack = (best - ratio.gather(2, A)[..., 0]) / best                  # relative
    pick = ratio.argmax(dim=2)
    roots = int((pick != A[..., 0]).any(dim=0).sum())
    all_loss, all_logp = res.all_loss.cpu(), res.all_logp.cpu()
    cost_err = (all_loss.reshape(V) - ol).abs().max().item()
    acc_err = (all_logp.reshape(V) - olp).abs().max().item()
    slp = res.step_logp.cpu()
    olp_t = torch.stack([st["logp"] for st in forced_trace])
    step_err = (slp - olp_t).abs().max().item()
    print(f"best-of-K kind={kind} N={N} B={B} K={K}: T={T} oracle T={oT} slack={slack.max().item():.3e} "
          f"runner-ups={roots} diverged={int(div.sum())} cost_err={cost_err:.3e} "
          f"acc_logp_err={acc_err:.3e} step_logp_err={step_err:.3e}")
    assert slack.max().item() < TIE_GAP, (slack.max().item(), TIE_GAP)
    assert roots <= max(2, V // 100), f"{roots} of {V} elements chose a near-tie runner-up"
    if not roots:
        assert not div.any(), f"{int(div.sum())} elements diverged from the oracle without a near tie"
        assert T == oT
    assert cost_err < TOL, cost_err
    assert acc_err < TOL * max(1, T / 4), acc_err
    assert step_err < 1e-5, step_err

    # ---- selection: exact, from the HIP run's own all_loss ----------------------------
    al = all_loss.numpy()
    assert al.shape == (K, B) and al.dtype == np.float32
    best_k = res.best_k.cpu().numpy()
    assert best_k.dtype == np.int32
    want_k = al.argmax(0)                  # numpy: the lowest index among equal maxima
    assert np.array_equal(best_k, want_k)
    cols = np.arange(B)
    assert np.array_equal(res.acc_loss.cpu().numpy(), al[want_k, cols])
    assert np.array_equal(res.acc_logp.cpu().numpy(), all_logp.numpy()[want_k, cols])
    chosen = res.actions.cpu().numpy()
    assert chosen.shape == (T, B) and chosen.dtype == np.int64
    assert np.array_equal(chosen, acts[:, want_k * B + cols])
    oracle_best = ol.reshape(K, B).max(dim=0).values
    assert (res.acc_loss.cpu() - oracle_best).abs().max().item() < TOL
    if (kind, N, B, K) == (0, 5, 3, 7):
        # the point of this case: some instance's best cost is reached by more than one sample
        assert ((al == al.max(0, keepdims=True)).sum(0) > 1).any()
    # the env ends as if the chosen tours had been played
    assert env.is_done()
    assert np.array_equal(env.current_location[:, 0], chosen[T - 1])
    assert env.step_count == T


@pytest.mark.parametrize("kind,N,B", [(0, 20, 64), (1, 40, 33)])
def test_k1_is_the_ordinary_sampled_rollout(kind, N, B):
    from agents import runtime
    agent = _agents()[kind](seed=69)
    model = agent.model
    model.eval()
    env = _envs()[kind](N, B, 1, 1234)
    torch.manual_seed(7)
    with torch.no_grad():
        ref = runtime.rollout(model, deepcopy(env), greedy=False, noise_mode="host", step_trace=True)
    torch.manual_seed(7)
    with torch.no_grad():
        res = runtime.rollout_best_of(model, deepcopy(env), 1, noise_mode="host")
    assert res.T == ref.T
    T = res.T
    a, r = res.actions.cpu().numpy(), ref.actions[:T].cpu().numpy()
    same = (a == r).all(axis=0)
    print(f"K=1 kind={kind} N={N} B={B}: {int((~same).sum())} graphs differ")
    assert int((~same).sum()) <= max(2, B // 100)
    err = (res.acc_loss.cpu() - ref.acc_loss.cpu()).abs().numpy()[same]
    assert err.max() < TOL, err.max()
    assert np.array_equal(res.best_k.cpu().numpy(), np.zeros(B, np.int32))
    assert torch.equal(res.all_loss[0], res.acc_loss)


def test_device_noise_is_reproducible_and_diverse():
    from agents import runtime
    agent = _agents()[0](seed=69)
    model = agent.model
    model.eval()
    env = _envs()[0](20, 16, 1, 1234)
    runs = []
    for _ in range(2):
        torch.manual_seed(11)
        with torch.no_grad():
            res = runtime.rollout_best_of(model, deepcopy(env), 8, noise_mode="device")
        runs.append((res.all_loss.cpu(), res.actions.cpu()))
    assert torch.equal(runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1], runs[1][1])
    # samples of one instance are not all equal
    al = runs[0][0]
    assert al.shape == (8, 16)
    assert ((al != al[0:1]).any(dim=0)).all(), al


def test_evaluate_keeps_greedy_and_takes_samples():
    from agents import runtime
    agent = _agents()[0](seed=69)
    env = _envs()[0](20, 32, 1, 1234)
    loss = agent.evaluate(deepcopy(env))
    with torch.no_grad():
        ref = runtime.rollout(agent.model, deepcopy(env), greedy=True)
    assert torch.equal(loss, ref.acc_loss)
    torch.manual_seed(3)
    best = agent.evaluate(env, samples=4)
    res = agent.model.last_rollout
    assert res.all_loss.shape == (4, 32)
    assert (best >= res.all_loss.mean(dim=0)).all()
    assert torch.equal(best, res.all_loss.max(dim=0).values)


def _tour_edges(start, tour):
    path = [int(start)] + [int(a) for a in tour]
    return {(min(a, b), max(a, b)) for a, b in zip(path[:-1], path[1:]) if a != b}


def test_sample_best_replays_the_chosen_tours_on_a_watched_env(monkeypatch):
    """A watched env (materialised sampler.graphs, or a video recorder) gets the CHOSEN samples'
    tours replayed on the host, like the greedy evaluation: the rendering flags of exactly the
    traversed edges, and with a recorder one frame per step of the chosen tour."""
    import sys
    import types
    import agents
    from gym_vrp.envs import TSPEnv, VRPEnv
    for Env, Agent in ((TSPEnv, agents.TSPAgent), (VRPEnv, agents.VRPAgent)):
        env = Env(num_nodes=9, batch_size=6, num_draw=2, seed=11)
        agent = Agent(seed=69)
        graphs = env.sampler.graphs          # materialise: the env is watched from here on
        depots = env.depots[:, 0].copy()
        torch.manual_seed(3)
        loss = agent.evaluate(env, samples=5)
        res = agent.model.last_rollout
        tours = res.actions.cpu().numpy()
        assert torch.equal(loss, res.all_loss.max(dim=0).values)
        for b in range(6):
            assert set(graphs[b].visited_edges) == _tour_edges(depots[b], tours[:, b]), b
        assert env.step_count == res.T
    # with a video recorder: one frame per step, each showing that step's location of the chosen tour
    frames = []

    class Recorder:
        def __init__(self, env=None, path=None, **kw):
            self.env, self.frames_per_sec = env, None

        def capture_frame(self):
            frames.append((int(self.env.current_location[0, 0]), int(self.env.step_count),
                           set(self.env.sampler.graphs[0].visited_edges)))

        def close(self):
            pass

    vr = types.ModuleType("gym.wrappers.monitoring.video_recorder")
    vr.VideoRecorder = Recorder
    mods = {"gym": types.ModuleType("gym"), "gym.wrappers": types.ModuleType("gym.wrappers"),
            "gym.wrappers.monitoring": types.ModuleType("gym.wrappers.monitoring"),
            "gym.wrappers.monitoring.video_recorder": vr}
    mods["gym"].wrappers = mods["gym.wrappers"]
    mods["gym.wrappers"].monitoring = mods["gym.wrappers.monitoring"]
    mods["gym.wrappers.monitoring"].video_recorder = vr
    for name, m in mods.items():
        monkeypatch.setitem(sys.modules, name, m)
    env = TSPEnv(num_nodes=9, batch_size=6, num_draw=2, seed=11)
    agent = agents.TSPAgent(seed=69)
    env.enable_video_capturing("unused.mp4")
    depot0 = int(env.depots[0, 0])
    torch.manual_seed(3)
    agent.evaluate(env, samples=5)
    res = agent.model.last_rollout
    tour0 = res.actions.cpu().numpy()[:, 0]
    assert len(frames) == res.T == env.step_count
    for t, (loc, count, edges) in enumerate(frames):
        assert loc == int(tour0[t]) and count == t + 1, (t, loc, count)
        assert edges == _tour_edges(depot0, tour0[: t + 1]), t
    assert np.array_equal(env.current_location[:, 0], res.actions.cpu().numpy()[-1])


def test_train_mode_and_unsupported_size_are_refused():
    from agents import runtime
    agent = _agents()[0](seed=69)
    env = _envs()[0](20, 4, 1, 1234)
    agent.model.train()
    with pytest.raises(ValueError, match="eval mode"):
        runtime.rollout_best_of(agent.model, env, 2)
    agent.model.eval()
    with pytest.raises(ValueError, match="K >= 1"):
        runtime.rollout_best_of(agent.model, env, 0)
    big = _envs()[0](101, 2, 1, 1234)
    with pytest.raises(RuntimeError, match="N <= 100"):
        runtime.rollout_best_of(agent.model, big, 2)
