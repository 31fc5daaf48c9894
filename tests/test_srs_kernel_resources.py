"""CPU tier: the kernels of the setup from an SRS (srs_setup.hip), read from the built library.  Every one runs whole group operations
per lane in 64-lane groups and uses no LDS.  The two that multiply by a full-size scalar (the butterfly and the column sum) are the
heavy ones -- a complete addition, a doubling and the scalar's words live at once, and the words are indexed at run time -- so they
sit at one or two waves per SIMD with kilobytes of scratch; the figures pinned here are the ones the build gives (DESIGN.md 4.8
records them) and are ceilings / floors, not targets met.  How often the fixed-base kernels the SRS generator borrows, and every
other kernel, are instantiated is tests/kernel_inventory.py's to say."""
import operator

import pytest

import kernel_inventory as inv

G1_BLS, G2_BLS, G1_BN, G2_BN = "Fp<Bls12_381FqP>", "Fp2<Bls12_381FqP>", "Fp<Bn254FqP>", "Fp2<Bn254FqP>"
# (kernel, coordinate field): (vector registers incl. accumulation registers, scratch bytes, waves per SIMD) as built
BUILT = {
    ("srs_butterfly_kernel", G1_BLS): (242, 1664, 2), ("srs_butterfly_kernel", G2_BLS): (268, 5232, 1),
    ("srs_butterfly_kernel", G1_BN): (232, 464, 2), ("srs_butterfly_kernel", G2_BN): (308, 2208, 1),
    ("srs_colsum_kernel", G1_BLS): (242, 1568, 2), ("srs_colsum_kernel", G2_BLS): (268, 4848, 1),
    ("srs_colsum_kernel", G1_BN): (232, 304, 2), ("srs_colsum_kernel", G2_BN): (316, 2080, 1),
    ("srs_colfold_kernel", G1_BLS): (122, 640, 4), ("srs_colfold_kernel", G2_BLS): (197, 2336, 2),
    ("srs_colfold_kernel", G1_BN): (134, 0, 3), ("srs_colfold_kernel", G2_BN): (220, 848, 2),
    ("srs_colfinish_kernel", G1_BLS): (102, 400, 4), ("srs_colfinish_kernel", G2_BLS): (150, 752, 3),
    ("srs_colfinish_kernel", G1_BN): (84, 64, 5), ("srs_colfinish_kernel", G2_BN): (151, 448, 3),
    ("srs_normalize_kernel", G1_BLS): (102, 400, 4), ("srs_normalize_kernel", G2_BLS): (150, 752, 3),
    ("srs_normalize_kernel", G1_BN): (84, 64, 5), ("srs_normalize_kernel", G2_BN): (151, 448, 3),
    ("srs_lift_kernel", G1_BLS): (62, 0, 8), ("srs_lift_kernel", G2_BLS): (90, 0, 5),
    ("srs_lift_kernel", G1_BN): (42, 0, 8), ("srs_lift_kernel", G2_BN): (62, 0, 8),
    ("srs_diff_kernel", G1_BLS): (134, 928, 3), ("srs_diff_kernel", G1_BN): (112, 208, 4),
    ("srs_scale_kernel", G1_BLS): (122, 976, 4), ("srs_scale_kernel", G1_BN): (188, 208, 2),
}


@pytest.fixture(scope="module")
def kernels():
    return inv.kernels()


@pytest.mark.parametrize("kernel,field", sorted(BUILT))
def test_srs_kernel_budget(kernels, kernel, field):
    regs, scratch, waves = BUILT[(kernel, field)]
    inv.check_budget(inv.one(kernels, prefix=kernel + "<" + field), 64, regs, scratch, 0, waves, lds_cmp=operator.eq)


def test_srs_kernel_names_and_counts(kernels):
    mine = sorted(n for n in kernels if "srs_" in n)
    assert len(mine) == 28 == len(BUILT), mine   # six kernels for G1 and G2 of both curves, the h difference and the delta step for G1
    assert all(n.startswith("srs_") for n in mine)
    others = ("decompress_", "subgroup_", "verify_", "pairing_", "keyload_", "bucket_", "ntt30_", "digits_kernel", "build_window_tables_kernel",
              "spmv", "merged", "fixed_base_", "sub_count_kernel", "sub_partition_kernel", "final_sort_kernel", "quotient_kernel", "circom_",
              "r1cs_", "scan_", "class_", "reduce_kernel", "combine_kernel", "bitrev_scale_kernel", "dwm_column_kernel")
    for name in mine:
        assert not any(s in name for s in others), name


def test_existing_instantiations_unchanged(kernels):
    """the SRS generator borrows fixed_base_mul_kernel / fixed_base_table_kernel as they are: four instantiations each, as the inventory says"""
    for sub in ("fixed_base_mul_kernel", "fixed_base_table_kernel"):
        assert len(inv.pick(kernels, sub)) == 4 == inv.INVENTORY[inv.MAIN][sub], sub
