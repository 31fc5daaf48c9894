"""CPU tier: budgets of the Circom map's two kernels (witness_map.hip), read from the built library with tools/kernel_occupancy.py.
Both are one-lane-per-element streaming kernels like the Libsnark map's spmv3_kernel and quotient_kernel and must stay inside those
kernels' register budgets on the same build: no scratch, no LDS (they declare none), no more registers."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
FIELDS = ["Bls12_381FrP", "Bn254FrP"]
PAIRS = [("spmv_circom_kernel", "spmv3_kernel"), ("circom_h_kernel", "quotient_kernel")]


@pytest.fixture(scope="module")
def kernels():
    import kernel_occupancy

    import groth16_amd

    return kernel_occupancy.kernels(groth16_amd.lib().path)


def one(kernels, name, field):
    hit = [k for n, k in kernels.items() if n.startswith(name + "<") and field in n]
    assert len(hit) == 1, (name, field, [n for n in kernels if name in n])
    return hit[0]


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("mine,yardstick", PAIRS)
def test_circom_kernel_budget(kernels, mine, yardstick, field):
    k, ref = one(kernels, mine, field), one(kernels, yardstick, field)
    print(mine, field, k, "against", yardstick, ref)
    assert k["scratch"] == 0, k
    assert k["lds"] == 0, k
    assert k["vgpr"] <= ref["vgpr"], (k, ref)
    assert k["agpr"] == 0, k
