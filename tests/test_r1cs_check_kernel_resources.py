"""CPU tier: budget of the satisfaction check's kernel (r1cs_check.hip), read from the built library with tools/kernel_occupancy.py
as test_circom_kernel_resources.py does for the Circom map.

96 registers is a condition, not a measurement: the yardstick spmv3_kernel sits at 62, two more 8-word sums held across the third
walk add 16, and 96 keeps five waves per SIMD on a latency-bound gather.  No scratch, no LDS (the wave reduces with a ballot), no
accumulation registers."""
import pytest

import kernel_inventory as inv

FIELDS = ["Bls12_381FrP", "Bn254FrP"]
VGPR_BUDGET = 96


@pytest.fixture(scope="module")
def kernels():
    return inv.kernels()


@pytest.mark.parametrize("field", FIELDS)
def test_check_kernel_budget(kernels, field):
    k = inv.one(kernels, field, prefix="r1cs_check_kernel<")
    print("r1cs_check_kernel", field, k, "spmv3_kernel", inv.one(kernels, field, prefix="spmv3_kernel<"))
    assert k["scratch"] == 0, k
    assert k["lds"] == 0, k
    assert k["agpr"] == 0, k
    assert k["vgpr"] <= VGPR_BUDGET, k


@pytest.mark.parametrize("field", FIELDS)
def test_row_values_kernel_has_no_scratch(kernels, field):
    k = inv.one(kernels, field, prefix="r1cs_row_values_kernel<")
    assert k["scratch"] == 0 and k["lds"] == 0 and k["agpr"] == 0, k
