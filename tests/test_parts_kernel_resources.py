"""Register / scratch budget of the bucket-part walk's kernels (the pass kernel in msm.hip, the layout kernels in msm_sort.hip), read from the code objects inside the BUILT product
library (no GPU needed); beside tests/test_kernel_resources.py, which holds the segment walk's kernel to the same budgets.
bucket_parts30_kernel keeps zero scratch and the occupancy of the segment walk's kernel -- G1 three waves per SIMD (four on BN254),
the lane-pair G2 kernel two -- and no more LDS than the parked accumulator; the two layout kernels use at most 64 registers and no
scratch, so that a wave of theirs fits beside a pass.  The scans are msm_sort.hip's, in one code object: tests/test_kernel_inventory.py."""
import pytest

import kernel_inventory as inv


@pytest.fixture(scope="module")
def kernels():
    return inv.kernels()


def test_names_and_counts(kernels):
    """four pass instantiations and the two layout kernels are there; the totals are the inventory's"""
    inv.pick(kernels, prefix="bucket_parts30_kernel<", count=4)
    for name in ("part_count_kernel", "part_place_kernel"):
        inv.pick(kernels, prefix=name, count=1)


@pytest.mark.parametrize("curve,limbs,g1_waves", [("Bls12_381FqP", 13, 3), ("Bn254FqP", 9, 4)])
def test_part_walk_keeps_the_pass_budgets(kernels, curve, limbs, g1_waves):
    for field, waves in (("Fp30<", g1_waves), ("Fp2p30<", 2)):
        ((name, k),) = inv.pick(kernels, "bucket_parts30_kernel<", field + curve, count=1).items()
        s = inv.one(kernels, "bucket_accumulate30_kernel", field + curve, "false")
        assert k["scratch"] == 0, (name, k)
        assert k["waves_per_simd"] >= waves and k["waves_per_simd"] >= s["waves_per_simd"], (name, k, s)
        assert k["lds"] == 4 * limbs * 64 * 4 == s["lds"], (name, k)   # x, y, zz, zzz: NL words each for 64 lanes, nothing else


def test_part_layout_kernels_fit_beside_a_pass(kernels):
    for sub in ("part_count_kernel", "part_place_kernel"):
        for name, k in inv.pick(kernels, sub).items():
            assert k["vgpr"] <= 64 and k["scratch"] == 0, (name, k)
            assert k["max_flat_wg"] <= 256, (name, k)
            assert k["lds"] == 0, (name, k)                # dynamic: Lmax (+ 97) words, 0.6 KB at Lmax = 64
