"""CPU tier: budgets of the aggregate verifier's kernels (verify_aggregate.hip), read from the built library.  The per-proof
stage keeps what tests/test_verify_kernel_resources.py demands of verify_batch_kernel: scratch <= 16 KB per lane, two waves per
SIMD, 64-lane workgroups (the wave reduction moves values across the lanes of ONE wave)."""
import operator

import pytest

import kernel_inventory as inv

CURVES = ["Bls12_381FqP", "Bn254FqP"]


@pytest.fixture(scope="module")
def kernels():
    return inv.kernels()


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("kernel", ["verify_agg_miller_kernel", "verify_agg_reduce_kernel"])
def test_pairing_stage_budget(kernels, kernel, curve):
    inv.check_budget(inv.one(kernels, kernel, curve), wg=64, scratch=16 * 1024, lds=0, waves=2, lds_cmp=operator.eq)


@pytest.mark.parametrize("curve", CURVES)
def test_scalar_stage_budget(kernels, curve):
    """Fr sums: registers only, one Fr per lane of LDS for the workgroup's tree"""
    for sub, lanes in (("verify_agg_scalar_kernel", 256), ("verify_agg_scalar_reduce_kernel", 64)):
        inv.check_budget(inv.one(kernels, sub, curve), scratch=0, lds=32 * lanes, waves=4, lds_cmp=operator.eq)


def test_names_stay_out_of_the_other_budgets(kernels):
    """tests/test_verify_kernel_resources.py and the prover's budget tests match kernels by substring"""
    others = ("pairing_prepare_kernel", "pairing_product_kernel", "verify_window_table_kernel", "verify_batch_kernel",
              "bucket_accumulate30_kernel", "ntt30_", "digits_kernel", "build_window_tables_kernel", "spmv3_kernel")
    agg = [n for n in kernels if "verify_agg_" in n]
    assert len(agg) == 8, agg
    for name in agg:
        assert not any(s in name for s in others), name
