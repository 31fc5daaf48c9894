"""Which kernels each built library holds, and the helpers the *_kernel_resources.py tests share (a plain module, no pytest hooks).

INVENTORY maps a library to {kernel-name prefix: instantiations}; every kernel of the library starts with exactly one prefix
(tests/test_kernel_inventory.py).  A new kernel means one line here and a budget test of its own, nothing else."""
import operator
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

MAIN = "libg16_mi355x.so"
INVENTORY = {
    MAIN: {
        # ntt.hip, witness_map.hip, r1cs_check.hip
        "bitrev_scale_kernel": 2, "gen_powers_kernel": 2, "ntt30_dif_dit_kernel": 2, "ntt30_pass_kernel": 4, "scale_table_kernel": 2,
        "tw_convert_kernel": 2, "circom_h_kernel": 2, "dwm_column_kernel": 20, "mark_unit_kernel": 2, "quotient_kernel": 2, "spmv3_kernel": 2,
        "spmv_circom_kernel": 2, "r1cs_check_kernel": 2, "r1cs_row_values_kernel": 2,
        # msm_sort.hip (one object for both curves), msm.hip (one object per curve; every kernel a template on the base field)
        "affine_level_kernel": 8, "bucket_accumulate30_kernel": 8, "bucket_combine_kernel": 4, "bucket_count_kernel": 1,
        "bucket_count_merged_kernel": 1, "bucket_reduce_kernel": 4, "bucket_scatter_kernel": 1, "bucket_scatter_merged_kernel": 1,
        "bucket_slots_kernel": 1, "bucket_wg_scan_kernel": 1, "build_window_tables_kernel": 4, "class_count_kernel": 2,
        "class_partition_kernel": 2, "convert_bases30_kernel": 4, "digits_kernel": 2, "final_sort_kernel": 1, "heavy_reduce_kernel": 4,
        "scan_block_offsets_kernel": 1, "scan_block_sums_kernel": 1, "scan_write_kernel": 1, "sub_count_kernel": 1, "sub_partition_kernel": 1,
        "window_reduce_kernel": 4,
        # the bucket-part walk: the pass kernel in msm.hip, the layout kernels in msm_sort.hip
        "bucket_parts30_kernel<": 4, "part_count_kernel": 1, "part_place_kernel": 1,
        # synth.hip, setup.hip, srs_setup.hip
        "mad_rate_kernel": 1, "synth_bases_kernel": 4, "fixed_base_mul_kernel": 4, "fixed_base_table_kernel": 4, "srs_butterfly_kernel": 4,
        "srs_colfinish_kernel": 4, "srs_colfold_kernel": 4, "srs_colsum_kernel": 4, "srs_diff_kernel": 2, "srs_lift_kernel": 4,
        "srs_normalize_kernel": 4, "srs_scale_kernel": 2,
        # the verify files, key_bytes.hip
        "pairing_prepare_kernel": 2, "pairing_product_kernel": 2, "verify_batch_kernel": 2, "verify_window_table_kernel": 2,
        "verify_agg_miller_kernel": 2, "verify_agg_reduce_kernel": 2, "verify_agg_scalar_kernel": 2, "verify_agg_scalar_reduce_kernel": 2,
        "verify_mixed_csum_kernel": 2, "verify_mixed_delta_kernel": 2, "verify_mixed_key_kernel": 2, "verify_mixed_miller_kernel": 2,
        "verify_mixed_reduce_kernel": 2, "verify_mixed_scalar_kernel": 2, "subgroup_combine_kernel": 1, "subgroup_g1_kernel": 2,
        "subgroup_g2_kernel": 2, "decompress_combine_kernel": 1, "decompress_g1_kernel": 2, "decompress_g2_kernel": 2,
        "keyload_decode_g1_kernel": 2, "keyload_decode_g2_kernel": 2, "keyload_fold_kernel": 1,
        # the labs (test hooks): devtest.hip, towerlab.hip, preplab.hip, stdlab.hip
        "devlab_op<": 162, "devlab_tower_op<": 2, "devlab_prepare_inputs<": 2, "devlab_std_op<": 10,
    },
    "libg16_ceremony.so": {"ceremony_digits128_kernel": 1, "ceremony_first_bad_kernel": 1},
    "libg16_phase1.so": {"batch_scalar_mul_kernel": 4, "phase1_powers_kernel": 2},
    "libg16_keycheck.so": {"keycheck_add_kernel": 2, "keycheck_rho_kernel": 2, "keycheck_rows_kernel": 2, "keycheck_scatter_odd_kernel": 2},
    "libg16_lagrange.so": {"lagrange_addsub_kernel": 4, "lagrange_bitrev_kernel": 4, "lagrange_twiddle_mul_kernel": 4},
}

_read = {}


def objects(libname=MAIN):
    """one {kernel name: figures} per code object of a built library (tools/kernel_occupancy.py), read once per process"""
    import kernel_occupancy

    import groth16_amd

    path = os.path.join(os.path.dirname(groth16_amd.lib().path), libname)
    assert os.path.exists(path), path
    if path not in _read:
        _read[path] = kernel_occupancy.kernels_per_object(path)
    assert _read[path], "could not read the code objects of " + path
    return _read[path]


def kernels(libname=MAIN):
    return {name: k for obj in objects(libname) for name, k in obj.items()}


def pick(kernels, *subs, prefix="", count=None):
    """the kernels whose name starts with `prefix` and holds every one of `subs` (spaces ignored): at least one, or exactly `count`"""
    hit = {n: k for n, k in kernels.items() if n.replace(" ", "").startswith(prefix.replace(" ", "")) and all(s in n for s in subs)}
    assert hit if count is None else len(hit) == count, (prefix, subs, count, sorted(hit) or sorted(kernels))
    return hit


def one(kernels, *subs, prefix=""):
    return next(iter(pick(kernels, *subs, prefix=prefix, count=1).values()))


def check_budget(k, wg=None, regs=None, scratch=None, lds=None, waves=None, lds_cmp=operator.le):
    """workgroup ==, registers <=, scratch <=, LDS `lds_cmp`, waves per SIMD >=; a bound left None is not checked"""
    assert wg is None or k["max_flat_wg"] == wg, k
    assert regs is None or k["vgpr"] + k["agpr"] <= regs, k
    assert scratch is None or k["scratch"] <= scratch, k
    assert lds is None or lds_cmp(k["lds"], lds), k
    assert waves is None or k["waves_per_simd"] >= waves, k
