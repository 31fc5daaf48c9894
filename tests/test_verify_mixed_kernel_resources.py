"""CPU tier: budgets of the mixed-key aggregate verifier's kernels (verify_mixed.hip), read from the built library.  The kernels
that run Miller loops or multiply Fq12 values across a wave are held to what tests/test_verify_aggregate_kernel_resources.py
demands of their single-key counterparts: two waves per SIMD, scratch <= 16 KB per lane, 64-lane workgroups (the wave reductions
move values across the lanes of ONE wave)."""
import operator

import pytest

import kernel_inventory as inv

CURVES = ["Bls12_381", "Bn254"]
MILLER = ["verify_mixed_miller_kernel", "verify_mixed_key_kernel", "verify_mixed_delta_kernel", "verify_mixed_reduce_kernel"]
ALL = MILLER + ["verify_mixed_scalar_kernel", "verify_mixed_csum_kernel"]


@pytest.fixture(scope="module")
def kernels():
    return inv.kernels()


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("kernel", MILLER)
def test_pairing_stage_budget(kernels, kernel, curve):
    inv.check_budget(inv.one(kernels, kernel, curve), wg=64, scratch=16 * 1024, lds=0, waves=2, lds_cmp=operator.eq)


@pytest.mark.parametrize("curve", CURVES)
def test_scalar_and_sum_stage_budget(kernels, curve):
    """Fr sums: registers only, one Fr per lane of LDS for the workgroup's tree; the per-key sum of the records: one wave"""
    inv.check_budget(inv.one(kernels, "verify_mixed_scalar_kernel", curve), scratch=0, lds=32 * 256, waves=4, lds_cmp=operator.eq)
    inv.check_budget(inv.one(kernels, "verify_mixed_csum_kernel", curve), wg=64, scratch=16 * 1024, waves=2)


def test_names_stay_out_of_the_other_budgets(kernels):
    """the other *_kernel_resources.py tests pick kernels by substring, and count those that carry verify_agg_"""
    others = ("verify_agg_", "verify_batch_kernel", "pairing_product_kernel", "pairing_prepare_kernel", "verify_window_table_kernel",
              "subgroup_", "decompress_", "pairing_", "bucket_accumulate30_kernel", "ntt30_", "digits_kernel", "build_window_tables_kernel", "spmv3_kernel")
    mixed = [n for n in kernels if "verify_mixed_" in n]
    assert len(mixed) == len(ALL) * len(CURVES), mixed
    for name in mixed:
        assert sum(k in name for k in ALL) == 1, name
        assert not any(s in name for s in others), name
