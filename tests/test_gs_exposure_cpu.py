"""CPU: the exposure-compensation entry points of the tape-free GS trainer are declared in include/cut3r_hip.h and bound in the ctypes
table (no compute)."""
import os
import re

from cut3r_slam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cut3r_exposure_forward", "cut3r_exposure_partial_rows", "cut3r_exposure_backward", "cut3r_gs_exposure_step")


def test_the_four_exposure_entry_points_are_declared_and_bound():
    src = open(os.path.join(ROOT, "include", "cut3r_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = dict((name, ret) for ret, name in re.findall(r"\b(int|long long)\s+(cut3r_\w+)\s*\(", src))
    for name in NAMES:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
    # the row count is the one 64-bit return among them, on both sides
    assert declared["cut3r_exposure_partial_rows"] == "long long" and _lib.RESTYPES["cut3r_exposure_partial_rows"] is _lib.c_ll
    assert all(declared[n] == "int" and n not in _lib.RESTYPES for n in NAMES if n != "cut3r_exposure_partial_rows")
    # argument counts follow the header (pointers, sizes, the stream last)
    assert [len(_lib.SIGNATURES[n]) for n in NAMES] == [6, 2, 9, 5]
