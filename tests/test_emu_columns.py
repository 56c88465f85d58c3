"""Columnar decode (dsrcgpu_decompress_batch_columns_device, dsrc_amd/csrc/k_columns.h) on the CPU: the kernel sources compiled
against the HIP emulator in tests/emu (workgroups of 256 threads), driven through the C ABI and both Python layers, and compared
with the arrays derived from the ORACLE's decoded text (tests/columns_cases.py).  Exact equality throughout."""
import os
import subprocess

import pytest

from tests import columns_cases as cc
from tests.cases import LEVELS

SHAPES = cc.SHAPES["emu"]

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
    cc.run_tiny(emu, SHAPES, d, q, lossy, crc)


@pytest.mark.parametrize("d,q", [(0, 0), (3, 2)])
def test_wave_boundaries(emu, d, q):
    cc.run_wave_boundaries(emu, SHAPES, d, q)


@pytest.mark.parametrize("d,q,lossy", [(2, 1, True), (0, 0, False)])
def test_scan_tiles_and_carry(emu, d, q, lossy):
    cc.run_scan_tiles(emu, SHAPES, d, q, lossy)


def test_block_bases(emu):
    cc.run_block_bases(emu, SHAPES)


def test_empty_batch_and_single_block(emu):
    cc.run_empty_and_single(emu, SHAPES)


def test_capacity(emu):
    cc.run_capacity(emu, SHAPES)


def test_titles_off(emu):
    cc.run_titles_off(emu, SHAPES)


def test_other_dataset_flags(emu):
    cc.run_dataset_flags(emu, SHAPES)


def test_color_space_is_refused(emu):
    cc.run_color_space(emu, SHAPES)


@pytest.mark.parametrize("d,q,lossy,crc", LEVELS)
def test_fuzz(emu, d, q, lossy, crc):
    cc.run_fuzz(emu, SHAPES, d, q, lossy, crc)


def test_text_path_unchanged(emu):
    cc.run_text_path_unchanged(emu, SHAPES)


def test_torch_wrapper(emu):
    cc.run_torch_wrapper(emu, SHAPES, "cpu")
