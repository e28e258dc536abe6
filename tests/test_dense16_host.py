"""The 16-bit dense design without a device: the entry points are declared, and a float16 array reaches the library."""
import numpy as np
import pytest

from adelie_amd import _abi


def test_the_entry_points_are_listed():
    assert {"design_create_dense16", "design_adopt_dense16_dev"} <= set(_abi.HIP_SYMBOLS)
    b = _abi.hip_backend()
    assert b.has("design_create_dense16") and b.has("design_adopt_dense16_dev")


def test_float16_without_a_device_has_no_cpu_fallback():
    b = _abi.hip_backend()
    if b.fn("device_count")() > 0:
        pytest.skip("a GPU is visible")
    import adelie_amd as ad

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ad.matrix.dense(np.zeros((4, 2), np.float16, order="F"))
