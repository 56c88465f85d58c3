"""Columnar encode (dsrcgpu_compress_columns_device, dsrcgpu_columns_cut; dsrc_amd/csrc/k_columns_enc.h) on the MI355X: the
product library, through the C ABI and both Python layers, compared with the ORACLE's blocks -- the same cases as
tests/test_emu_columns_enc.py (tests/columns_enc_cases.py), here with workgroups of 1024 threads.  Exact equality throughout."""
import os

import pytest

from tests import columns_enc_cases as ce
from tests.cases import LEVELS

SHAPES = ce.SHAPES["gpu"]

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    os.environ.pop("DSRC_GPU_LIB", None)
    from dsrc_amd import _lib
    _lib._lib = None
    return _lib


@pytest.mark.parametrize("d,q,lossy,crc", LEVELS)
def test_tiny(gpu, d, q, lossy, crc):
    ce.run_tiny(gpu, SHAPES, d, q, lossy, crc)


@pytest.mark.parametrize("d,q", [(0, 0), (3, 2)])
def test_wave_boundaries(gpu, d, q):
    ce.run_wave_boundaries(gpu, SHAPES, d, q)


def test_block_bases_crc_verify(gpu):
    ce.run_block_bases(gpu, SHAPES)


def test_iontorrent_lossy(gpu):
    ce.run_iontorrent_lossy(gpu, SHAPES)


def test_other_dataset_flags(gpu):
    ce.run_dataset_flags(gpu, SHAPES)


@pytest.mark.parametrize("d,q,lossy,crc", LEVELS)
def test_fuzz(gpu, d, q, lossy, crc):
    ce.run_fuzz(gpu, SHAPES, d, q, lossy, crc)


def test_nonzero_start(gpu):
    ce.run_nonzero_start(gpu, SHAPES)


def test_two_calls_carry_the_state(gpu):
    ce.run_two_calls(gpu, SHAPES)


def test_empty_single_record_and_color_space(gpu):
    ce.run_empty_single_color(gpu, SHAPES)


def test_argument_errors(gpu):
    ce.run_arg_errors(gpu, SHAPES)


def test_input_errors_are_refused_by_the_check_pass(gpu):
    ce.run_input_errors(gpu, SHAPES)


def test_zero_length_read_follows_the_text_call(gpu):
    ce.run_zero_length_read(gpu, SHAPES)


def test_columns_cut(gpu):
    ce.run_columns_cut(gpu, SHAPES)


def test_closed_loop_through_torch(gpu):
    ce.run_closed_loop(gpu, SHAPES, "cuda:0")
