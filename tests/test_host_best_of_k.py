"""Best-of-K sampled decoding, the parts that need no GPU: the C ABI (symbols, version, workspace
size), the loud failure without a device, and the register audit of the new kernels read from the
built library's code objects."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# audited at the change that added them: multi_step_kernel<1> 103 and <2> 149 VGPRs (three / two
# waves per SIMD under their launch bounds), multi_first_table_kernel 160 of the 512 a one-wave-
# per-SIMD workgroup may use; nothing spilled, no scratch
NEW_KERNELS = ("multi_step_kernel<1>", "multi_step_kernel<2>", "multi_first_table_kernel<true>",
               "multi_first_table_kernel<false>")


def test_new_symbols_declared_and_exported():
    import vrpgym_hip
    lib = vrpgym_hip.lib()
    header = open(os.path.join(ROOT, "include", "vrpgym_hip.h")).read()
    declared = set(re.findall(r"\b(vrp_[a-z_0-9]+)\s*\(", header))
    for n in ("vrp_multi_workspace_bytes", "vrp_rollout_multi"):
        assert n in declared, f"{n} not declared in include/vrpgym_hip.h"
        assert hasattr(lib, n), f"{n} not exported by the built library"
    assert "typedef struct vrp_multi_io" in header
    import ctypes
    # six pointers, the seed, four pointers, logit_clip (float, padded)
    assert ctypes.sizeof(vrpgym_hip.MultiIO) == 6 * 8 + 8 + 4 * 8 + 8


def test_abi_versions_are_9():
    import vrpgym_hip
    header = open(os.path.join(ROOT, "include", "vrpgym_hip.h")).read()
    want = int(re.search(r"#define\s+VRP_ABI_VERSION\s+(\d+)", header).group(1))
    assert want == 9
    assert vrpgym_hip.ABI_VERSION == 9
    assert vrpgym_hip.lib().vrp_abi_version() == 9


def test_multi_workspace_bytes_positive_and_monotone():
    import vrpgym_hip
    f = vrpgym_hip.lib().vrp_multi_workspace_bytes
    for kind in (0, 1, 2):
        for N in (3, 20, 63, 100):
            prev_k = 0
            for K in (1, 2, 5, 16, 32, 100):
                v = int(f(kind, 12, N, K))
                assert v > 0 and v >= prev_k, (kind, N, K, v, prev_k)
                prev_k = v
            prev_b = 0
            for B in (1, 3, 12, 64, 512, 513):
                v = int(f(kind, B, N, 8))
                assert v > 0 and v >= prev_b, (kind, N, B, v, prev_b)
                prev_b = v
    # per element: a visited row, two mask rows, three node indices and an fp64 load at least
    V, N = 16 * 512, 20
    assert int(f(0, 512, N, 16)) >= V * (3 * N + 3 * 4 + 8)
    # TSP/VRP carry the first-node score table of the B instances, IRP has none
    assert int(f(0, 512, 20, 16)) - int(f(2, 512, 20, 16)) >= 512 * 20 * 8 * 20 * 4
    # an invalid shape has no size
    assert int(f(0, 4, 20, 0)) == 0 and int(f(3, 4, 20, 2)) == 0


def test_rollout_best_of_has_no_cpu_path():
    import agents
    from agents import runtime
    model = agents.TSPAgent().model.cpu()
    model.eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        runtime.rollout_best_of(model, None, 4)
    assert hasattr(model, "sample_best")
    import inspect
    sig = inspect.signature(agents.TSPAgent.evaluate)
    assert sig.parameters["samples"].default is None


def test_new_kernels_do_not_spill():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    table = {name.split("(")[0].replace("void ", "").strip(): r
             for name, r in kernel_resources.resources().items()}
    for k in NEW_KERNELS:
        assert k in table, f"{k} not in the library"
        r = table[k]
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0, (k, r)
    # the launch bounds' register files: 256 threads with three (N <= 64) / two waves per SIMD
    assert table["multi_step_kernel<1>"]["vgpr"] <= 168
    assert table["multi_step_kernel<2>"]["vgpr"] <= 256
