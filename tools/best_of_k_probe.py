#!/usr/bin/env python3
"""Best-of-K sampled decoding against what a user could write before it existed.

  A   runtime.rollout_best_of(model, env, K), device noise: encoder + prologue on B instances,
      V = K B elements decoded per step
  B1  ONE existing sampled rollout on an env of K B distinct instances (generator="device"): the
      same decode work, with the encoder and the prologue on V graphs
  B2  K back-to-back existing sampled rollouts on the B instances

One process, device events around each call, every shape warmed up, A / B1 / B2 alternated,
REPS repetitions each; medians and the 10 % / 90 % quantiles.

usage: best_of_k_probe.py [--reps 30] [--warmup 5] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "vrp-gym_amd"), ROOT]

SHAPES = [(0, 20, 512, 16), (1, 40, 256, 32), (1, 100, 64, 32)]   # kind, N, B, K
NAMES = {0: "TSP", 1: "VRP", 2: "IRP"}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3   # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import agents
    import vrpgym_hip
    from agents import runtime
    from gym_vrp.envs import IRPEnv, TSPEnv, VRPEnv
    envs = {0: TSPEnv, 1: VRPEnv, 2: IRPEnv}
    mk = {0: agents.TSPAgent, 1: agents.VRPAgent, 2: agents.IRPAgent}
    lines = ["source %s  reps %d  warmup %d  (us per call: median [p10 .. p90])"
             % (vrpgym_hip.lib().vrp_source_hash().decode(), args.reps, args.warmup),
             "%-18s %28s %28s %28s %8s %8s" % ("shape", "A best-of-K", "B1 one rollout at K*B",
                                               "B2 K rollouts at B", "B1/A", "B2/A")]
    for kind, N, B, K in SHAPES:
        model = mk[kind](seed=69).model
        model.eval()
        env = envs[kind](N, B, 1, 1234, generator="device")
        envV = envs[kind](N, K * B, 1, 1234, generator="device")
        torch.manual_seed(5)

        def run_a():
            runtime.rollout_best_of(model, env, K, noise_mode="device")

        def run_b1():
            runtime.rollout(model, envV, greedy=False, noise_mode="device", reset_env=True)

        def run_b2():
            for _ in range(K):
                runtime.rollout(model, env, greedy=False, noise_mode="device", reset_env=True)

        runs = {"A": run_a, "B1": run_b1, "B2": run_b2}
        with torch.no_grad():
            for _ in range(args.warmup):
                for fn in runs.values():
                    fn()
            torch.cuda.synchronize()
            t = {k: [] for k in runs}
            for _ in range(args.reps):
                for k, fn in runs.items():
                    t[k].append(timed(fn))
        med = {k: float(np.median(v)) for k, v in t.items()}

        def cell(k):
            v = np.array(t[k])
            return "%9.1f [%8.1f .. %8.1f]" % (med[k], np.quantile(v, 0.1), np.quantile(v, 0.9))

        lines.append("%-18s %28s %28s %28s %8.2f %8.2f" % (
            "%s-%d B=%d K=%d" % (NAMES[kind], N, B, K), cell("A"), cell("B1"), cell("B2"),
            med["B1"] / med["A"], med["B2"] / med["A"]))
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
