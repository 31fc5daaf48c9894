"""CPU tier: budgets of the Circom map's two kernels (witness_map.hip), read from the built library with tools/kernel_occupancy.py.
Both are one-lane-per-element streaming kernels like the Libsnark map's spmv3_kernel and quotient_kernel and must stay inside those
kernels' register budgets on the same build: no scratch, no LDS (they declare none), no more registers."""
import pytest

import kernel_inventory as inv

FIELDS = ["Bls12_381FrP", "Bn254FrP"]
PAIRS = [("spmv_circom_kernel", "spmv3_kernel"), ("circom_h_kernel", "quotient_kernel")]


@pytest.fixture(scope="module")
def kernels():
    return inv.kernels()


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("mine,yardstick", PAIRS)
def test_circom_kernel_budget(kernels, mine, yardstick, field):
    k, ref = inv.one(kernels, field, prefix=mine + "<"), inv.one(kernels, field, prefix=yardstick + "<")
    print(mine, field, k, "against", yardstick, ref)
    assert k["scratch"] == 0, k
    assert k["lds"] == 0, k
    assert k["vgpr"] <= ref["vgpr"], (k, ref)
    assert k["agpr"] == 0, k
