"""Columnar encode (dsrcgpu_compress_columns_device, dsrcgpu_columns_cut; dsrc_amd/csrc/k_columns_enc.h) on the CPU: the kernel
sources compiled against the HIP emulator in tests/emu (workgroups of 256 threads), driven through the C ABI and both Python
layers, and compared with the ORACLE's blocks (tests/columns_enc_cases.py).  Exact equality throughout."""
import os
import subprocess

import pytest

from tests import columns_enc_cases as ce
from tests.cases import LEVELS

SHAPES = ce.SHAPES["emu"]

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


@pytest.mark.parametrize("d,q,lossy,crc", LEVELS)
def test_tiny(emu, d, q, lossy, crc):
    ce.run_tiny(emu, SHAPES, d, q, lossy, crc)


@pytest.mark.parametrize("d,q", [(0, 0), (3, 2)])
def test_wave_boundaries(emu, d, q):
    ce.run_wave_boundaries(emu, SHAPES, d, q)


def test_block_bases_crc_verify(emu):
    ce.run_block_bases(emu, SHAPES)


def test_iontorrent_lossy(emu):
    ce.run_iontorrent_lossy(emu, SHAPES)


def test_other_dataset_flags(emu):
    ce.run_dataset_flags(emu, SHAPES)


@pytest.mark.parametrize("d,q,lossy,crc", LEVELS)
def test_fuzz(emu, d, q, lossy, crc):
    ce.run_fuzz(emu, SHAPES, d, q, lossy, crc)


def test_nonzero_start(emu):
    ce.run_nonzero_start(emu, SHAPES)


def test_two_calls_carry_the_state(emu):
    ce.run_two_calls(emu, SHAPES)


def test_empty_single_record_and_color_space(emu):
    ce.run_empty_single_color(emu, SHAPES)


def test_argument_errors(emu):
    ce.run_arg_errors(emu, SHAPES)


def test_input_errors_are_refused_by_the_check_pass(emu):
    ce.run_input_errors(emu, SHAPES)


def test_zero_length_read_follows_the_text_call(emu):
    ce.run_zero_length_read(emu, SHAPES)


def test_columns_cut(emu):
    ce.run_columns_cut(emu, SHAPES)


def test_closed_loop_through_torch(emu):
    ce.run_closed_loop(emu, SHAPES, "cpu")
