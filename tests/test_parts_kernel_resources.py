"""Register / scratch budget of the bucket-part walk's kernels, read from the code object inside the BUILT part-walk library
(libg16_partwalk.so, beside the product library, which links against it; no GPU needed); beside tests/test_kernel_resources.py, which
holds the segment walk's kernel to the same budgets.  bucket_parts30_kernel keeps zero scratch and the occupancy of the segment walk's
kernel -- G1 three waves per SIMD (four on BN254), the lane-pair G2 kernel two -- and no more LDS than the parked accumulator; the two
layout kernels use at most 64 registers and no scratch, so that a wave of theirs fits beside a pass.  The library holds these kernels and
its own copy of the three scan kernels, nothing else."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _kernels(path):
    import kernel_occupancy

    return kernel_occupancy.kernels(path)


@pytest.fixture(scope="module")
def kernels():
    import groth16_amd

    path = os.path.join(os.path.dirname(groth16_amd.lib().path), "libg16_partwalk.so")
    assert os.path.exists(path), path
    return _kernels(path)


@pytest.fixture(scope="module")
def prover_kernels():
    import groth16_amd

    return _kernels(groth16_amd.lib().path)


def pick(kernels, *subs):
    hit = {n: k for n, k in kernels.items() if all(s in n for s in subs)}
    assert hit, f"no kernel matches {subs}"
    return hit


def test_names_and_counts(kernels):
    names = sorted(n for n in kernels if n)
    assert len([n for n in names if n.startswith("bucket_parts30_kernel<")]) == 4, names
    rest = sorted(n.split("(")[0] for n in names if not n.startswith("bucket_parts30_kernel<"))
    assert rest == ["part_count_kernel", "part_place_kernel", "scan_block_offsets_kernel", "scan_block_sums_kernel", "scan_write_kernel"], names


@pytest.mark.parametrize("curve,limbs,g1_waves", [("Bls12_381FqP", 13, 3), ("Bn254FqP", 9, 4)])
def test_part_walk_keeps_the_pass_budgets(kernels, prover_kernels, curve, limbs, g1_waves):
    for field, waves in (("Fp30<", g1_waves), ("Fp2p30<", 2)):
        part = pick(kernels, "bucket_parts30_kernel<", field + curve)
        seg = pick(prover_kernels, "bucket_accumulate30_kernel", field + curve, "false")
        assert len(part) == 1 and len(seg) == 1
        (name, k), (_, s) = list(part.items())[0], list(seg.items())[0]
        assert k["scratch"] == 0, (name, k)
        assert k["waves_per_simd"] >= waves and k["waves_per_simd"] >= s["waves_per_simd"], (name, k, s)
        assert k["lds"] == 4 * limbs * 64 * 4 == s["lds"], (name, k)   # x, y, zz, zzz: NL words each for 64 lanes, nothing else


def test_part_layout_kernels_fit_beside_a_pass(kernels):
    for sub in ("part_count_kernel", "part_place_kernel"):
        for name, k in pick(kernels, sub).items():
            assert k["vgpr"] <= 64 and k["scratch"] == 0, (name, k)
            assert k["max_flat_wg"] <= 256, (name, k)
            assert k["lds"] == 0, (name, k)                # dynamic: Lmax (+ 97) words, 0.6 KB at Lmax = 64
