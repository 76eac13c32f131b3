"""The decoder prologue's tables written by the x3 encoder stack kernel's tail
(encoder_stack_tables_x3_kernel) against the standalone prologue (VRP_STACK_NO_TABLES=1), on the
same instances and weights, each in a child process of its own (the switch is read once)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5          # the suite's tolerance on cost / log-prob (test_gpu_parity.py)

# (kind, B, N): 512 x 20 (16-byte table stores), 1024 x 10 (four graphs per workgroup), 256 x 40
# (one), 512 x 21 (element-wise stores), 100 x 21 (50 workgroups: gated off, both runs take the
# standalone prologue), 6144 x 2 (24 graphs per workgroup: the QG scratch of the stack epilogue)
SHAPES = [(k, B, N) for k in (0, 1, 2)
          for B, N in ((512, 20), (1024, 10), (256, 40), (512, 21), (100, 21))] + [(0, 6144, 2), (1, 6144, 2)]

_CHILD = r"""
import os, sys
sys.path[:0] = [os.path.join(sys.argv[1], "vrp-gym_amd"), sys.argv[1]]
import numpy as np, torch
import agents
from agents import runtime
from gym_vrp.envs import IRPEnv, TSPEnv, VRPEnv
shapes = eval(sys.argv[3])

def al(x):
    return (x + 255) // 256 * 256

out = {}
for kind, B, N in shapes:
    env = (TSPEnv, VRPEnv, IRPEnv)[kind](num_nodes=N, batch_size=B, num_draw=1, seed=13)
    agent = (agents.TSPAgent, agents.VRPAgent, agents.IRPAgent)[kind](seed=69)
    agent.model.eval()
    with torch.no_grad():
        r = runtime.rollout(agent.model, env, True, record=True)
    torch.cuda.synchronize()
    T = r.T
    tag = f"{kind}_{B}_{N}"
    out[tag + "_loss"] = r.acc_loss.cpu().numpy()
    out[tag + "_logp"] = r.acc_logp.cpu().numpy()
    out[tag + "_act"] = r.actions[:T].cpu().numpy()
    out[tag + "_emb"] = r.emb.cpu().numpy()
    # DecWs (decoder_ws.h: carve_decws) up to KK4; the fused prologue's shapes have no PROJ
    f = runtime.workspaces(agent.model, env)[1].view(torch.uint8)
    hn, tb = B * 8 * N * 4, B * N * 8 * N * 4
    kk = B * 8 * N * 48 * 4 if (N <= 63 and B <= 1024 and kind != 2) else 0
    regions = [("g", B * 128 * 4), ("QG", B * 384 * 4), ("SG", hn), ("C0", hn), ("SLD", hn),
               ("row0", hn), ("curs", hn), ("base", hn), ("Efirst", B * 128 * 4),
               ("FK", B * 1024 * 4), ("SL", tb), ("RT", tb), ("KK4", kk)]
    off = 0
    for name, size in regions:
        if name in ("g", "QG", "SG", "C0", "SLD", "row0", "SL", "RT", "KK4") and size:
            out[tag + "_" + name] = f[off:off + size].view(torch.float32).cpu().numpy()
        off += al(size)
np.savez(sys.argv[2], **out)
"""


def _run(tmp_path, tag, extra):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _proc
    drop = ("VRP_STACK_NO_TABLES", "VRP_NO_STACK_QG")
    env = {k: v for k, v in os.environ.items() if k not in drop}
    env.update(extra)
    out = str(tmp_path / f"{tag}.npz")
    r = _proc.run([sys.executable, "-c", _CHILD, ROOT, out, repr(SHAPES)], env=env, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(out)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("stack_tables")
    return {"fused": _run(tmp, "fused", {}),
            "plain": _run(tmp, "plain", {"VRP_STACK_NO_TABLES": "1"}),
            "gemm": _run(tmp, "gemm", {"VRP_STACK_NO_TABLES": "1", "VRP_NO_STACK_QG": "1"})}


@pytest.mark.gpu
@pytest.mark.parametrize("kind,B,N", SHAPES)
def test_stack_tables_equal_standalone_prologue(runs, kind, B, N):
    """SL, RT, SG, C0, SLD, row0 (and KK4 where kept) of the fused tail against the standalone
    prologue on bit-identical embeddings: equal up to fp32 re-association, relative to the largest
    entry of each table."""
    a, b = runs["fused"], runs["plain"]
    tag = f"{kind}_{B}_{N}"
    assert np.array_equal(a[tag + "_emb"], b[tag + "_emb"])
    assert np.array_equal(a[tag + "_QG"], b[tag + "_QG"])
    worst = {}
    for name in ("SL", "RT", "SG", "C0", "SLD", "row0", "KK4"):
        key = f"{tag}_{name}"
        if key not in a.files:
            continue
        x, y = a[key], b[key]
        assert np.isfinite(x).all(), key
        worst[name] = float(np.max(np.abs(x - y)) / max(np.max(np.abs(y)), 1e-30))
    print(tag, " ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert max(worst.values()) <= 1e-5, worst


@pytest.mark.gpu
@pytest.mark.parametrize("kind,B,N", SHAPES)
def test_stack_qg_matches_gemm(runs, kind, B, N):
    """The graph means and QG = Wq_g g + bq of the stack kernel's epilogue against the separate
    GEMM (VRP_NO_STACK_QG=1) -- 24 graphs per workgroup at N = 2 included (the partial sums of
    the epilogue once overwrote the means of graphs >= 16 there)."""
    a, g = runs["fused"], runs["gemm"]
    tag = f"{kind}_{B}_{N}"
    assert np.array_equal(a[tag + "_emb"], g[tag + "_emb"])
    np.testing.assert_allclose(a[tag + "_g"], g[tag + "_g"], rtol=0, atol=1e-6)
    qg, qr = a[tag + "_QG"], g[tag + "_QG"]
    assert np.max(np.abs(qg - qr)) <= 1e-5 * max(np.max(np.abs(qr)), 1.0)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,B,N", SHAPES)
def test_stack_tables_rollouts(runs, kind, B, N):
    """Greedy rollouts on the fused tables against the standalone prologue's: the same tours on at
    least 97 % of the graphs (near-ties), costs and log-probs within the suite's tolerance."""
    a, b = runs["fused"], runs["plain"]
    tag = f"{kind}_{B}_{N}"
    same = (a[tag + "_act"] == b[tag + "_act"]).all(axis=0)
    assert same.mean() >= 0.97, same.mean()
    T = a[tag + "_act"].shape[0]
    assert np.max(np.abs(a[tag + "_loss"][same] - b[tag + "_loss"][same])) < TOL
    assert np.max(np.abs(a[tag + "_logp"][same] - b[tag + "_logp"][same])) < TOL * max(1, T / 4)
