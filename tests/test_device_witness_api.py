"""CPU tests of the device-witness interface (ms_witness_create_device / msbb_witness_create_device): the Python wrappers
exist on both System classes, refuse everything that has no device pointer before the library is called, and the two
entry points are exported. No GPU is touched: the wrappers are driven on System objects that were never created."""
import ctypes

import numpy as np
import pytest


class FakeDeviceArray:
    """an object with __cuda_array_interface__ (the pointer is never dereferenced in these tests)"""

    def __init__(self, shape, typestr="<u8", ptr=0x1000, strides=None):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, False), "strides": strides, "version": 3}


def _unborn(cls, n_circuits=1):
    """a System that was never created: any call into the library through it would fail on the missing handle"""
    s = object.__new__(cls)
    s.n_circuits = n_circuits
    return s


def _systems(pkg):
    return [pkg.System, pkg.babybear.System]


def test_wrapper_exists_on_both_systems(pkg):
    for cls in _systems(pkg):
        assert callable(getattr(cls, "witness_from_device"))


def test_new_symbols_are_listed_and_exported(pkg):
    assert "ms_witness_create_device" in pkg.exported_symbols()
    assert "msbb_witness_create_device" in pkg.babybear.exported_symbols()
    L = ctypes.CDLL(pkg.LIB_PATH)
    assert hasattr(L, "ms_witness_create_device") and hasattr(L, "msbb_witness_create_device")


def test_dev_matrix_mirror_has_the_c_layout(pkg):
    """ms_dev_matrix: pointer, u64, u32 (+ padding), two i64"""
    m = pkg.DevMatrix
    assert [f[0] for f in m._fields_] == ["ptr", "height", "elem_bytes", "row_stride", "col_stride"]
    assert (m.ptr.offset, m.height.offset, m.elem_bytes.offset, m.row_stride.offset, m.col_stride.offset) == (0, 8, 16, 24, 32)
    assert ctypes.sizeof(m) == 40


@pytest.mark.parametrize("which", [0, 1])
def test_numpy_array_is_refused(pkg, fe, which):
    s = _unborn(_systems(pkg)[which])
    with pytest.raises(pkg.MstarkError, match="no device pointer"):
        s.witness_from_device([np.zeros((4, 3), dtype=np.uint64)], fe.pack_claims([]))


@pytest.mark.parametrize("which", [0, 1])
def test_cpu_tensor_is_refused(pkg, fe, which):
    import torch

    s = _unborn(_systems(pkg)[which])
    with pytest.raises(pkg.MstarkError, match="CPU tensor"):
        s.witness_from_device([torch.zeros((4, 3), dtype=torch.int64)], fe.pack_claims([]))


@pytest.mark.parametrize("which", [0, 1])
def test_one_dimensional_object_is_refused(pkg, fe, which):
    s = _unborn(_systems(pkg)[which])
    with pytest.raises(pkg.MstarkError, match="2-D"):
        s.witness_from_device([FakeDeviceArray((12,))], fe.pack_claims([]))
    with pytest.raises(pkg.MstarkError, match="2-D"):
        s.witness_from_device([FakeDeviceArray((2, 3, 2))], fe.pack_claims([]))


@pytest.mark.parametrize("which", [0, 1])
def test_wrong_number_of_traces_is_refused(pkg, fe, which):
    s = _unborn(_systems(pkg)[which], n_circuits=2)
    with pytest.raises(pkg.MstarkError, match="one trace per circuit"):
        s.witness_from_device([None], fe.pack_claims([]))


@pytest.mark.parametrize("which", [0, 1])
def test_wrong_width_is_refused_before_the_library_is_called(pkg, fe, which):
    s = _unborn(_systems(pkg)[which])
    s.circuit_info = lambda ci: {"main_width": 5}
    with pytest.raises(pkg.MstarkError, match="main_width is 5"):
        s.witness_from_device([FakeDeviceArray((4, 3))], fe.pack_claims([]))


def test_strides_are_taken_from_the_object_in_elements(pkg):
    """row-major default, explicit byte strides (a column-major view), and axes of one element"""
    arr, heights, seen = pkg._device_traces([FakeDeviceArray((8, 3), "<u4"), FakeDeviceArray((8, 3), "<i2", strides=(2, 16)), None,
                                             FakeDeviceArray((1, 3), "|u1", strides=(0, 1)), FakeDeviceArray((4, 1), "<u8", strides=(8, 0))],
                                            5, lambda i: [3, 3, 9, 3, 1][i])
    assert heights == [8, 8, 0, 1, 4] and seen is None
    got = [(m.ptr, m.height, m.elem_bytes, m.row_stride, m.col_stride) for m in arr]
    assert got == [(0x1000, 8, 4, 3, 1), (0x1000, 8, 2, 1, 8), (None, 0, 1, 1, 1), (0x1000, 1, 1, 3, 1), (0x1000, 4, 8, 1, 1)]
    with pytest.raises(pkg.MstarkError, match="whole elements"):
        pkg._device_traces([FakeDeviceArray((8, 3), "<u4", strides=(6, 2))], 1, lambda i: 3)


def test_package_imports_without_torch():
    """torch is imported by witness_from_device only, and only when a torch tensor is seen"""
    import subprocess
    import sys
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys\n"
            "sys.modules['torch'] = None\n"  # any `import torch` now raises ImportError
            "sys.path.insert(0, %r)\n"
            "from __graft_entry__ import load_package\n"
            "pkg = load_package()\n"
            "assert hasattr(pkg.System, 'witness_from_device')\n"
            "print('ok')\n") % root
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-2000:]
