"""Register budget of the x3 stack kernel with the decoder prologue's tables as its tail
(encoder_stack_tables_x3_kernel): read from the built library's code objects, no GPU needed."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# audited at the change that added the tail: 245 / 256 registers, nothing spilled -- the tail's
# VALU blocks live after the layer loop and do not raise its peak
BUDGET = {"encoder_stack_tables_x3_kernel<3>": 0, "encoder_stack_x3_kernel<3>": 0}


def test_stack_tables_kernel_does_not_spill():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    table = {name.split("(")[0].replace("void ", "").strip(): r
             for name, r in kernel_resources.resources().items()}
    for k, budget in BUDGET.items():
        assert k in table, f"{k} not in the library"
        r = table[k]
        assert r["vgpr_spill"] <= budget and r["scratch"] == 0, (k, r)
        assert r["vgpr"] <= 256, (k, r)   # two waves per SIMD: eight waves of 512 threads
