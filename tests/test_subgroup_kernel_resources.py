"""CPU tier: budgets of the membership kernels (verify_subgroup.hip), read from the built library.  The chains need one XYZZ
accumulator and Fq / Fq2 products only, so they stay far below the pairing kernels' scratch and above their two waves per SIMD.
The figures are the ones the build gives (DESIGN.md 4.6 records them): scratch rounded up to the next KB as a ceiling, the waves
per SIMD as a floor."""
import operator

import pytest

import kernel_inventory as inv

# (kernel, curve): (scratch ceiling in bytes, waves-per-SIMD floor); read: BLS12-381 G1 816 B / 4, G2 3552 B / 4,
# BN254 G1 0 B / 8 (on-curve test only), G2 2032 B / 4
BUDGET = {
    ("subgroup_g1_kernel", "Bls12_381FqP"): (1024, 4),
    ("subgroup_g2_kernel", "Bls12_381FqP"): (4096, 4),
    ("subgroup_g1_kernel", "Bn254FqP"): (0, 8),
    ("subgroup_g2_kernel", "Bn254FqP"): (2048, 4),
}


@pytest.fixture(scope="module")
def kernels():
    return inv.kernels()


@pytest.mark.parametrize("kernel,curve", sorted(BUDGET))
def test_membership_kernel_budget(kernels, kernel, curve):
    scratch, waves = BUDGET[(kernel, curve)]
    assert scratch <= 16 * 1024 and waves >= 2
    inv.check_budget(inv.one(kernels, kernel, curve), wg=64, scratch=scratch, lds=0, waves=waves, lds_cmp=operator.eq)


def test_combine_kernel_and_names(kernels):
    k = inv.one(kernels, "subgroup_combine_kernel")
    assert k["scratch"] == 0 and k["lds"] == 0, k
    others = ("verify_agg_", "verify_batch_kernel", "pairing_", "verify_window_table_kernel", "bucket_accumulate30_kernel", "ntt30_",
              "digits_kernel", "build_window_tables_kernel", "spmv3_kernel")
    mine = [n for n in kernels if "subgroup_" in n]
    assert len(mine) == 5, mine
    for name in mine:
        assert not any(s in name for s in others), name
