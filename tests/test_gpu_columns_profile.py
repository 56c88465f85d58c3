"""Columnar profile (dsrcgpu_columns_profile; dsrc_amd/csrc/k_columns_profile.h) on the MI355X: the product library, through the C
ABI and both Python layers, compared with the integer model of tests/columns_profile_cases.py -- the same cases as
tests/test_emu_columns_profile.py, here with workgroups of 1024 threads, the full fuzz, the record counts that take the grid stride
of either table size into a second round, and the record whose quality sum passes 2^32 in one cycle.  Exact equality of every word
throughout."""
import os

import pytest

from tests import columns_profile_cases as cf

SHAPES = cf.SHAPES["gpu"]

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    os.environ.pop("DSRC_GPU_LIB", None)
    from dsrc_amd import _lib
    _lib._lib = None
    return _lib


@pytest.mark.parametrize("n_cycles", cf.CYCLES)
def test_geometry_lengths_and_the_fold(gpu, n_cycles):
    cf.run_geometry(gpu, SHAPES, n_cycles)


def test_values_one_value_gc_bins_and_rounding(gpu):
    cf.run_values(gpu, SHAPES)


def test_plans_in(gpu):
    cf.run_plans_in(gpu, SHAPES)


def test_accumulate_and_overwrite(gpu):
    cf.run_accumulate(gpu, SHAPES)


def test_argument_refusals(gpu):
    cf.run_arg_refusals(gpu, SHAPES)


def test_input_errors(gpu):
    cf.run_input_errors(gpu, SHAPES)


def test_codec_state_is_left_alone(gpu):
    cf.run_codec_state(gpu, SHAPES)


@pytest.mark.parametrize("n", SHAPES["counts"])
def test_record_counts(gpu, n):
    cf.run_count(gpu, SHAPES, n)


@pytest.mark.parametrize("n_cycles,n", SHAPES["stride_counts"])
def test_grid_stride_second_round(gpu, n_cycles, n):
    cf.run_stride(gpu, SHAPES, n_cycles, n)


def test_no_counter_wraps_at_2_to_32(gpu):
    cf.run_no_wrap(gpu, SHAPES)


@pytest.mark.parametrize("seed", range(SHAPES["prof_fuzz"][0]))
def test_fuzz(gpu, seed):
    cf.run_fuzz(gpu, SHAPES, seed)


def test_profile_columns_through_torch(gpu):
    cf.run_python_layers(gpu, SHAPES, "cuda:0")


def test_profile_of_a_plan_equals_profile_of_the_selection(gpu):
    cf.run_plan_equals_selection(gpu, SHAPES, "cuda:0")


def test_filter_columns_with_and_without_profile(gpu):
    cf.run_filter_columns(gpu, SHAPES, "cuda:0")


def test_filter_pairs_with_and_without_profile(gpu):
    cf.run_filter_pairs(gpu, SHAPES, "cuda:0")
