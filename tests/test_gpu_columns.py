"""Columnar decode (dsrcgpu_decompress_batch_columns_device, dsrc_amd/csrc/k_columns.h) on the MI355X: the product library,
through the C ABI and both Python layers, compared with the arrays derived from the ORACLE's decoded text -- the same cases as
tests/test_emu_columns.py (tests/columns_cases.py), here with workgroups of 1024 threads.  Exact equality throughout."""
import os

import pytest

from tests import columns_cases as cc
from tests.cases import LEVELS

SHAPES = cc.SHAPES["gpu"]

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    os.environ.pop("DSRC_GPU_LIB", None)
    from dsrc_amd import _lib
    _lib._lib = None
    return _lib


@pytest.mark.parametrize("d,q,lossy,crc", LEVELS)
def test_tiny(gpu, d, q, lossy, crc):
    cc.run_tiny(gpu, SHAPES, d, q, lossy, crc)


@pytest.mark.parametrize("d,q", [(0, 0), (3, 2)])
def test_wave_boundaries(gpu, d, q):
    cc.run_wave_boundaries(gpu, SHAPES, d, q)


@pytest.mark.parametrize("d,q,lossy", [(2, 1, True), (0, 0, False)])
def test_scan_tiles_and_carry(gpu, d, q, lossy):
    cc.run_scan_tiles(gpu, SHAPES, d, q, lossy)


def test_block_bases(gpu):
    cc.run_block_bases(gpu, SHAPES)


def test_empty_batch_and_single_block(gpu):
    cc.run_empty_and_single(gpu, SHAPES)


def test_capacity(gpu):
    cc.run_capacity(gpu, SHAPES)


def test_titles_off(gpu):
    cc.run_titles_off(gpu, SHAPES)


def test_other_dataset_flags(gpu):
    cc.run_dataset_flags(gpu, SHAPES)


def test_color_space_is_refused(gpu):
    cc.run_color_space(gpu, SHAPES)


@pytest.mark.parametrize("d,q,lossy,crc", LEVELS)
def test_fuzz(gpu, d, q, lossy, crc):
    cc.run_fuzz(gpu, SHAPES, d, q, lossy, crc)


def test_text_path_unchanged(gpu):
    cc.run_text_path_unchanged(gpu, SHAPES)


def test_torch_wrapper(gpu):
    cc.run_torch_wrapper(gpu, SHAPES, "cuda:0")
