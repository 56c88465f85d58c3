"""Columnar profile (dsrcgpu_columns_profile; dsrc_amd/csrc/k_columns_profile.h) on the CPU: the kernel sources compiled against the
HIP emulator in tests/emu (workgroups of 256 threads), driven through the C ABI and both Python layers, and compared with the
integer model of tests/columns_profile_cases.py.  Exact equality of every word throughout."""
import os
import subprocess

import pytest

from tests import columns_profile_cases as cf

SHAPES = cf.SHAPES["emu"]

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


@pytest.mark.parametrize("n_cycles", cf.CYCLES)
def test_geometry_lengths_and_the_fold(emu, n_cycles):
    cf.run_geometry(emu, SHAPES, n_cycles)


def test_values_one_value_gc_bins_and_rounding(emu):
    cf.run_values(emu, SHAPES)


def test_plans_in(emu):
    cf.run_plans_in(emu, SHAPES)


def test_accumulate_and_overwrite(emu):
    cf.run_accumulate(emu, SHAPES)


def test_argument_refusals(emu):
    cf.run_arg_refusals(emu, SHAPES)


def test_input_errors(emu):
    cf.run_input_errors(emu, SHAPES)


def test_codec_state_is_left_alone(emu):
    cf.run_codec_state(emu, SHAPES)


@pytest.mark.parametrize("n", SHAPES["counts"])
def test_record_counts(emu, n):
    cf.run_count(emu, SHAPES, n)


@pytest.mark.parametrize("seed", range(SHAPES["prof_fuzz"][0]))
def test_fuzz(emu, seed):
    cf.run_fuzz(emu, SHAPES, seed)


def test_profile_columns_through_torch(emu):
    cf.run_python_layers(emu, SHAPES, "cpu")


def test_profile_of_a_plan_equals_profile_of_the_selection(emu):
    cf.run_plan_equals_selection(emu, SHAPES, "cpu")


def test_filter_columns_with_and_without_profile(emu):
    cf.run_filter_columns(emu, SHAPES, "cpu")


def test_filter_pairs_with_and_without_profile(emu):
    cf.run_filter_pairs(emu, SHAPES, "cpu")
