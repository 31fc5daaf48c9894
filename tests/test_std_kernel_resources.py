"""Figures of the standard-form lab's kernels (stdlab.hip: devlab_std_op<curve, kind>), read from the code objects inside the BUILT
product library (no GPU needed) and pinned as this build gives them.  A lab kernel is no product kernel and nothing is tuned here; the
figures are pinned so that a change in how field.hpp / curve.hpp compile for the device -- a product that stops being out of line, a
formula that starts to spill -- shows in a diff.  Scratch is expected: the out-of-line products and the out-of-line mul_bits,
to_affine and inverse pass their operands through call frames, as in the product kernels that run them."""
import pytest

import kernel_inventory as inv

# (curve, kind) -> (VGPR + AGPR, scratch bytes); kind 0 Fr, 1 Fq, 2 Fq2, 3 G1, 4 G2
FIGURES = {
    ("Bls12_381", 0): (66, 96), ("Bls12_381", 1): (90, 240), ("Bls12_381", 2): (138, 544), ("Bls12_381", 3): (246, 1280), ("Bls12_381", 4): (264, 4464),
    ("Bn254", 0): (66, 96), ("Bn254", 1): (66, 96), ("Bn254", 2): (148, 240), ("Bn254", 3): (292, 368), ("Bn254", 4): (308, 1696),
}


@pytest.fixture(scope="module")
def kernels():
    return inv.kernels()


def test_names_and_counts(kernels):
    inv.pick(kernels, prefix="devlab_std_op<", count=10)


@pytest.mark.parametrize("curve,kind", sorted(FIGURES))
def test_std_lab_kernel_figures(kernels, curve, kind):
    k = inv.one(kernels, "%sConsts, %d>, %d>" % (curve, 0 if curve == "Bls12_381" else 1, kind), prefix="devlab_std_op<")
    regs, scratch = FIGURES[(curve, kind)]
    assert k["max_flat_wg"] == 64 and k["lds"] == 0, k
    assert (k["vgpr"] + k["agpr"], k["scratch"]) == (regs, scratch), k
