"""Resource budget of the sort's sub-class partition and LDS-resident final level, read from the code objects inside the BUILT
library (no GPU needed).

h's sort runs underneath the G2 bucket pass (2 x 194 registers of a SIMD lane's 512, 8 x 13 KB of a compute unit's 160 KB of LDS);
the kernels that replace the histogram-matrix scatter must fit beside it like the ones they replace: at most 64 registers, nothing
in scratch and at most 48 KB of LDS per 256-lane workgroup.  The numbers only -- what the kernels compute is checked on the GPU
(tests/test_gpu_sort_shapes.py)."""
import pytest

import kernel_inventory as inv

NEW_KERNELS = ("sub_count_kernel", "sub_partition_kernel", "final_sort_kernel")


@pytest.fixture(scope="module")
def kernels():
    ks = inv.kernels()
    assert len(ks) > 40, "could not read the code objects of the built library"
    return ks


@pytest.mark.parametrize("sub", NEW_KERNELS)
def test_new_sort_kernels_fit_beside_the_g2_bucket_pass(kernels, sub):
    for name, k in inv.pick(kernels, sub).items():
        assert k["vgpr"] <= 64, (name, k)
        assert k["scratch"] == 0, (name, k)
        assert k["lds"] <= 48 * 1024, (name, k)
        assert k["max_flat_wg"] <= 256, (name, k)
