"""CPU tier: budgets of the decompression kernels (verify_decompress.hip), read from the built library.  A lane keeps the running
power, the base and one product's temporaries; the exponentiation is out of line, so scratch holds little more than the operands
passed to it.  The figures are the ones the build gives (DESIGN.md 4.6 records them): scratch rounded up to the next KB as a
ceiling, the waves per SIMD as a floor."""
import operator

import pytest

import kernel_inventory as inv

# (kernel, curve): (scratch ceiling in bytes, waves-per-SIMD floor); read: BLS12-381 G1 224 B / 4, G2 912 B / 4,
# BN254 G1 48 B / 6, G2 480 B / 4
BUDGET = {
    ("decompress_g1_kernel", "Bls12_381FqP"): (1024, 4),
    ("decompress_g2_kernel", "Bls12_381FqP"): (1024, 4),
    ("decompress_g1_kernel", "Bn254FqP"): (1024, 6),
    ("decompress_g2_kernel", "Bn254FqP"): (1024, 4),
}


@pytest.fixture(scope="module")
def kernels():
    return inv.kernels()


@pytest.mark.parametrize("kernel,curve", sorted(BUDGET))
def test_decompress_kernel_budget(kernels, kernel, curve):
    scratch, waves = BUDGET[(kernel, curve)]
    assert scratch <= 16 * 1024 and waves >= 2
    inv.check_budget(inv.one(kernels, kernel, curve), wg=64, scratch=scratch, lds=0, waves=waves, lds_cmp=operator.eq)


def test_combine_kernel_and_names(kernels):
    k = inv.one(kernels, "decompress_combine_kernel")
    assert k["scratch"] == 0 and k["lds"] == 0, k
    others = ("subgroup_", "verify_agg_", "verify_batch_kernel", "pairing_", "verify_window_table_kernel")
    mine = [n for n in kernels if "decompress_" in n]
    assert len(mine) == 5, mine
    for name in mine:
        assert not any(s in name for s in others), name
