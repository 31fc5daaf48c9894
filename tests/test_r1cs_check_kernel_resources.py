"""CPU tier: budget of the satisfaction check's kernel (r1cs_check.hip), read from the built library with tools/kernel_occupancy.py
as test_circom_kernel_resources.py does for the Circom map.

96 registers is a condition, not a measurement: the yardstick spmv3_kernel sits at 62, two more 8-word sums held across the third
walk add 16, and 96 keeps five waves per SIMD on a latency-bound gather.  No scratch, no LDS (the wave reduces with a ballot), no
accumulation registers."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
FIELDS = ["Bls12_381FrP", "Bn254FrP"]
VGPR_BUDGET = 96


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
def test_check_kernel_budget(kernels, field):
    k = one(kernels, "r1cs_check_kernel", field)
    print("r1cs_check_kernel", field, k, "spmv3_kernel", one(kernels, "spmv3_kernel", field))
    assert k["scratch"] == 0, k
    assert k["lds"] == 0, k
    assert k["agpr"] == 0, k
    assert k["vgpr"] <= VGPR_BUDGET, k


@pytest.mark.parametrize("field", FIELDS)
def test_row_values_kernel_has_no_scratch(kernels, field):
    k = one(kernels, "r1cs_row_values_kernel", field)
    assert k["scratch"] == 0 and k["lds"] == 0 and k["agpr"] == 0, k
