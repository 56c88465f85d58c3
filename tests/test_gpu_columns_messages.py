"""The refusal messages of the columnar entry points (dsrc_amd/csrc/host_columns.h) on the MI355X: the product library, the same
cases and the same golden file as tests/test_emu_columns_messages.py."""
import os

import pytest

from tests import columns_messages_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    os.environ.pop("DSRC_GPU_LIB", None)
    from dsrc_amd import _lib
    _lib._lib = None
    return _lib


def test_refusal_messages(gpu):
    cases.run_messages(gpu)
