"""The refusal messages of the columnar entry points (dsrc_amd/csrc/host_columns.h) on the CPU: the library compiled against the HIP
emulator in tests/emu, every case of tests/columns_messages_cases.py compared with tests/golden/columns_messages_golden.json for
equality of return code and text."""
import os
import subprocess

import pytest

from tests import columns_messages_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu", "libdsrc_emu.so")


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "emu")], stdout=subprocess.DEVNULL)
    old = os.environ.get("DSRC_GPU_LIB")
    os.environ["DSRC_GPU_LIB"] = EMU
    from dsrc_amd import _lib
    _lib._lib = None
    yield _lib
    _lib._lib = None
    if old is None:
        os.environ.pop("DSRC_GPU_LIB", None)
    else:
        os.environ["DSRC_GPU_LIB"] = old


def test_refusal_messages(emu):
    cases.run_messages(emu)
