"""CPU tier: budgets of the key loader's kernels (key_bytes.hip), read from the built library.  The uncompressed decode takes no square
root: a lane range-checks two or four coordinates, converts them and evaluates the curve equation once, so it stays inside the
budget the decompression kernels meet -- scratch <= 1 KB, >= 4 waves per SIMD -- and the figures pinned here are the ones the build
gives (DESIGN.md 4.7 records them).  The compressed decode and the membership tests are NOT instantiated a second time."""
import operator

import pytest

import kernel_inventory as inv

CEILING_SCRATCH, FLOOR_WAVES = 1024, 4
# (kernel, curve): (scratch in bytes, waves per SIMD) as built: BLS12-381 G1 224 B / 4, G2 976 B / 4, BN254 G1 0 B / 8, G2 368 B / 7
BUILT = {
    ("keyload_decode_g1_kernel", "Bls12_381FqP"): (224, 4),
    ("keyload_decode_g2_kernel", "Bls12_381FqP"): (976, 4),
    ("keyload_decode_g1_kernel", "Bn254FqP"): (0, 8),
    ("keyload_decode_g2_kernel", "Bn254FqP"): (368, 7),
}


@pytest.fixture(scope="module")
def kernels():
    return inv.kernels()


@pytest.mark.parametrize("kernel,curve", sorted(BUILT))
def test_decode_kernel_budget(kernels, kernel, curve):
    scratch, waves = BUILT[(kernel, curve)]
    assert scratch <= CEILING_SCRATCH and waves >= FLOOR_WAVES
    inv.check_budget(inv.one(kernels, kernel, curve), wg=64, scratch=scratch, lds=0, waves=waves, lds_cmp=operator.eq)


def test_fold_kernel_and_names(kernels):
    k = inv.one(kernels, "keyload_fold_kernel")
    assert k["scratch"] == 0 and k["lds"] == 0 and k["max_flat_wg"] == 256 and k["waves_per_simd"] == 8, k
    mine = sorted(n for n in kernels if "keyload_" in n)
    assert len(mine) == 5, mine   # two decode kernels per curve and the fold
    others = ("decompress_", "subgroup_", "verify_", "pairing_", "bucket_accumulate30_kernel", "ntt30_", "digits_kernel",
              "build_window_tables_kernel", "spmv3_kernel", "merged")
    for name in mine:
        assert not any(s in name for s in others), name
    # the stages this path borrows exist exactly once per curve: loading keys added no instantiation of them
    for sub in ("decompress_g1_kernel", "decompress_g2_kernel", "subgroup_g1_kernel", "subgroup_g2_kernel"):
        assert len([n for n in kernels if sub in n]) == 2, sub
