"""The argument checks of the locate entry points that run before any device call (no GPU): null pointers, `unique` other than 0 / 1, and a
handle that is not one."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from gbwt_rs_amd import _lib


@pytest.fixture(scope="module", autouse=True)
def _build():
    subprocess.check_call(["make", "-C", _lib.CSRC], stdout=subprocess.DEVNULL)


def message():
    return _lib.lib().gbwt_hip_last_error().decode()


def test_null_arguments_are_bad_arguments():
    L = _lib.lib()
    states = np.zeros(2, dtype=[("node", "<u8"), ("start", "<u8"), ("end", "<u8")])
    offsets, ids, valid, total = np.zeros(3, np.uint64), np.zeros(4, np.uint64), np.zeros(2, np.uint8), C.c_uint64(7)
    rows, info = _lib.Located(), _lib.LocateInfo()
    p = lambda a: a.ctypes.data
    # no handle at all: nothing is touched but the outputs
    assert L.gbwt_hip_locate(None, None, p(states), 2, 0, p(offsets), p(ids), 4, C.byref(total), p(valid)) == _lib.BAD_ARGUMENT
    assert total.value == 0 and "index" in message()
    assert L.gbwt_hip_locate_device(None, None, p(states), 2, 0, C.byref(rows)) == _lib.BAD_ARGUMENT
    assert L.gbwt_hip_locate_states_device(None, None, None, None, 0, 1, C.byref(rows)) == _lib.BAD_ARGUMENT
    assert (rows.d_offsets, rows.d_ids, rows.d_valid, rows.n, rows.total) == (None, None, None, 0, 0)
    assert L.gbwt_hip_locate_positions(None, None, p(states), 2, p(ids), p(valid)) == _lib.BAD_ARGUMENT
    assert L.gbwt_hip_locate_index_info(None, C.byref(info)) == _lib.BAD_ARGUMENT
    steps, positions = C.c_uint64(3), C.c_uint64(3)
    assert L.gbwt_hip_locate_count_steps(None, None, p(states), 2, C.byref(steps), C.byref(positions)) == _lib.BAD_ARGUMENT
    assert (steps.value, positions.value) == (0, 0)
    walk, sort = C.c_float(0), C.c_float(0)
    assert L.gbwt_hip_last_locate_ms(None, C.byref(walk), C.byref(sort)) == _lib.BAD_ARGUMENT
    # unique is 0 or 1
    for unique in (2, -1):
        assert L.gbwt_hip_locate(None, None, p(states), 2, unique, p(offsets), p(ids), 4, C.byref(total), p(valid)) == _lib.BAD_ARGUMENT and "unique" in message()
        assert L.gbwt_hip_locate_device(None, None, p(states), 2, unique, C.byref(rows)) == _lib.BAD_ARGUMENT and "unique" in message()
        assert L.gbwt_hip_locate_states_device(None, None, None, None, 0, unique, C.byref(rows)) == _lib.BAD_ARGUMENT and "unique" in message()
    # missing outputs
    assert L.gbwt_hip_locate(None, None, p(states), 2, 0, p(offsets), p(ids), 4, None, p(valid)) == _lib.BAD_ARGUMENT and "null buffer" in message()
    assert L.gbwt_hip_locate(None, None, p(states), 2, 0, None, p(ids), 4, C.byref(total), p(valid)) == _lib.BAD_ARGUMENT and "null buffer" in message()
    assert L.gbwt_hip_locate(None, None, p(states), 2, 0, p(offsets), p(ids), 4, C.byref(total), None) == _lib.BAD_ARGUMENT and "null buffer" in message()
    assert L.gbwt_hip_locate_device(None, None, p(states), 2, 0, None) == _lib.BAD_ARGUMENT and "null output" in message()
    assert L.gbwt_hip_locate_states_device(None, None, None, None, 0, 0, None) == _lib.BAD_ARGUMENT and "null output" in message()
    assert L.gbwt_hip_locate_positions(None, None, p(states), 2, None, p(valid)) == _lib.BAD_ARGUMENT and "null buffer" in message()
    assert L.gbwt_hip_locate_index_info(None, None) == _lib.BAD_ARGUMENT
    assert L.gbwt_hip_locate_count_steps(None, None, p(states), 2, None, None) == _lib.BAD_ARGUMENT


def test_python_mirror_validates_before_it_calls():
    import gbwt_rs_amd as G
    dev = object.__new__(G.GBWT)                       # no handle: the checks below run before the library is asked
    with pytest.raises(TypeError):
        dev.locate_csr(np.zeros(3, dtype=G.api.POS_DTYPE))
    with pytest.raises(TypeError):
        dev.locate_csr(np.zeros((3, 3), dtype=np.float64))
    with pytest.raises(ValueError):
        dev.locate_csr(np.zeros((3, 2), dtype=np.uint64))
    with pytest.raises(ValueError):
        dev.locate_csr(np.zeros((2, 2), dtype=G.api.STATE_DTYPE))
    with pytest.raises(ValueError):
        dev.locate_positions(np.zeros((3, 3), dtype=np.uint64))
    with pytest.raises(ValueError):
        dev.locate_positions(np.array([[1, -1]]))
    with pytest.raises(TypeError):
        dev.locate_states_device(np.zeros(3, dtype=G.api.STATE_DTYPE))
