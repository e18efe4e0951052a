"""The rows layout of the sample-rate converter, without a GPU: the header declares the three
entry points, the library exports them, the binding table binds them, and the argument checks
that come before the device answer with libsamplerate's codes."""
import ctypes
import os
import re

from conftest import ROOT

NAMES = ("sdrgpu_src_new_rows", "sdrgpu_src_process_rows", "sdrgpu_src_process_rows_dev")


def test_header_declares_and_library_exports(sdr):
    text = open(os.path.join(ROOT, "include", "sdrgpu.h")).read()
    L = sdr.lib()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert getattr(L, name) is not None
    assert re.search(r"sdrgpu_src_process_rows_dev\s*\([^)]*size_t\s+ld_in,\s*size_t\s+ld_out\)", text)


def test_new_rows_rejections_come_before_the_device(sdr):
    L = sdr.lib()
    err = ctypes.c_int(0)
    assert not L.sdrgpu_src_new_rows(0, 9, 4, ctypes.byref(err)) and err.value == 10
    assert not L.sdrgpu_src_new_rows(0, -1, 4, ctypes.byref(err)) and err.value == 10
    assert not L.sdrgpu_src_new_rows(0, 4, 0, ctypes.byref(err)) and err.value == 11
    assert not L.sdrgpu_src_new_rows(0, 2, -3, None)


def test_rows_process_on_null_handle(sdr):
    from sdrgpu import resample
    L = sdr.lib()
    d = resample.SrcData(None, None, 0, 0, 0, 0, 0, 1.0)
    assert L.sdrgpu_src_process_rows(None, ctypes.byref(d), 0, 0) == 2
    assert L.sdrgpu_src_process_rows_dev(None, ctypes.byref(d), 0, 0) == 2
    assert L.sdrgpu_src_process_rows(None, None, 0, 0) == 2


def test_python_surface(sdr):
    from sdrgpu import fm, resample
    for m in ("process", "process_dev", "reset", "try_clone", "set_ratio", "set_stream", "stream",
              "sync"):
        assert callable(getattr(resample.SampleRateRows, m)), m
    assert callable(fm.receivers)

