"""The multi-vector apply's boundary without a GPU: both C entry points are
exported and declared, a null handle is refused without a device, the binding's
operand helper refuses every malformed batch before any pointer reaches the C
ABI, and the C++ facade exports the two new methods."""
import ctypes
import subprocess

import pytest


def test_library_exports_multi_symbols():
    import mas_amd
    lib = ctypes.CDLL(mas_amd.LIB_PATH)
    for sym in ("mas_apply_multi_device", "mas_apply_multi"):
        assert hasattr(lib, sym), sym
        assert sym in mas_amd.EXPORTS
    assert mas_amd.MAS_MAX_RHS == 8


def test_null_handle_without_device():
    import mas_amd
    L = mas_amd.lib()
    assert L.mas_apply_multi_device(None, 2, None, None, None) == -1
    assert L.mas_apply_multi(None, 2, None, None) == -1


def test_dev_multi_operand_checks_without_gpu():
    """_dev_multi: raw pointers are the caller's contract; tensors are checked
    for dtype, layout, shape, then device; K is 1..8 and equal for z and r."""
    import numpy as np
    import torch
    from mas_amd import _dev_multi, _ptr_array, MasError
    nV = 5
    assert _dev_multi([4096, 8192, 4096], nV, "r") == [4096, 8192, 4096]
    assert _dev_multi((16,), nV, "r", count=1) == [16]
    arr = _ptr_array([4096, 8192])
    assert len(arr) == 2 and arr[1] == 8192
    with pytest.raises(MasError, match="not on a GPU"):  # a CPU tensor, otherwise right
        _dev_multi(torch.zeros(2, nV, 4), nV, "z")
    with pytest.raises(MasError, match="not on a GPU"):
        _dev_multi([torch.zeros(nV, 4), torch.zeros(nV, 4)], nV, "z")
    with pytest.raises(MasError, match="expected torch.float32"):
        _dev_multi(torch.zeros(2, nV, 4, dtype=torch.float64), nV, "z")
    with pytest.raises(MasError, match="expected torch.float32"):
        _dev_multi([4096, torch.zeros(nV, 4, dtype=torch.int32)], nV, "z")
    with pytest.raises(MasError, match="contiguous"):
        _dev_multi(torch.zeros(nV, 2, 4).transpose(0, 1), nV, "z")
    with pytest.raises(MasError, match="contiguous"):
        _dev_multi([torch.zeros(nV, 8)[:, :4]], nV, "z")
    with pytest.raises(MasError, match="trailing shape"):
        _dev_multi(torch.zeros(2, nV, 3), nV, "z")
    with pytest.raises(MasError, match="trailing shape"):
        _dev_multi(torch.zeros(2, nV + 1, 4), nV, "z")
    with pytest.raises(MasError, match=r"\[K, 5, 4\]"):
        _dev_multi(torch.zeros(nV, 4), nV, "z")  # one vector is not a batch
    with pytest.raises(MasError, match=r"expected a \[5, 4\] tensor"):
        _dev_multi([torch.zeros(1, nV, 4)], nV, "z")
    with pytest.raises(MasError, match="MAS_ERR_ARG.*got 0"):
        _dev_multi([], nV, "z")
    with pytest.raises(MasError, match="MAS_ERR_ARG.*got 9"):
        _dev_multi(list(range(16, 16 * 10, 16)), nV, "z")
    with pytest.raises(MasError, match="MAS_ERR_ARG.*other operand has 3"):
        _dev_multi([16, 32], nV, "residual", count=3)
    with pytest.raises(MasError, match="torch cuda tensor or a raw device pointer"):
        _dev_multi([np.zeros((nV, 4), np.float32)], nV, "z")
    with pytest.raises(MasError, match="sequence"):
        _dev_multi(np.zeros((2, nV, 4), np.float32), nV, "z")
    with pytest.raises(MasError, match="missing"):
        _dev_multi(None, nV, "z")


def test_facade_exports_multi_methods():
    import mas_amd
    out = subprocess.run(["nm", "-D", "-C", "--defined-only", mas_amd.FACADE_PATH], capture_output=True,
                         text=True, check=True).stdout
    for sym in ("SE::SeSchwarzPreconditioner::PreconditioningMulti("
                "SE::SeVec3fSimd* const*, SE::SeVec3fSimd const* const*, int, int)",
                "SE::SeSchwarzPreconditioner::PreconditioningDeviceMulti("
                "SE::SeVec3fSimd* const*, SE::SeVec3fSimd const* const*, int, void*)"):
        assert sym in out, sym
