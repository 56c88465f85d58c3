"""Columnar complexity plan (dsrcgpu_columns_complexity_plan; dsrc_amd/csrc/k_columns_complexity.h) on the MI355X: the product
library, through the C ABI and both Python layers, compared with the integer model of tests/columns_complexity_cases.py -- the same
cases as tests/test_emu_columns_complexity.py, here with workgroups of 1024 threads, the full fuzz and the record count that takes
the planner's grid stride into a second round.  Exact equality throughout."""
import os

import pytest

from tests import columns_complexity_cases as cx

SHAPES = cx.SHAPES["gpu"]

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    os.environ.pop("DSRC_GPU_LIB", None)
    from dsrc_amd import _lib
    _lib._lib = None
    return _lib


@pytest.mark.parametrize("base", range(4))
def test_geometry_of_runs(gpu, base):
    cx.run_geometry(gpu, SHAPES, base)


@pytest.mark.parametrize("rate", cx.RATES)
def test_error_budget_exact_and_one_more(gpu, rate):
    cx.run_budget(gpu, SHAPES, rate)


def test_the_score(gpu):
    cx.run_score(gpu, SHAPES)


def test_complexity(gpu):
    cx.run_complexity(gpu, SHAPES)


def test_dust_lengths(gpu):
    cx.run_dust_lengths(gpu, SHAPES)


def test_dust_windows_and_thresholds(gpu):
    cx.run_dust_windows(gpu, SHAPES)


def test_dust_triplet_mapping(gpu):
    cx.run_dust_triplets(gpu, SHAPES)


def test_ranges_keep_in_place_and_info(gpu):
    cx.run_ranges(gpu, SHAPES)


def test_argument_refusals(gpu):
    cx.run_arg_refusals(gpu, SHAPES)


def test_input_errors(gpu):
    cx.run_input_errors(gpu, SHAPES)


def test_codec_state_is_left_alone(gpu):
    cx.run_codec_state(gpu, SHAPES)


@pytest.mark.parametrize("n", SHAPES["counts"])
def test_record_counts(gpu, n):
    cx.run_count(gpu, SHAPES, n)


def test_grid_stride_second_round(gpu):
    cx.run_count(gpu, SHAPES, SHAPES["stride_count"])


def test_fuzz_exercises_every_statistic(gpu):
    cx.run_fuzz_exercises_everything(gpu, SHAPES)


@pytest.mark.parametrize("seed", range(SHAPES["cplx_fuzz"][0]))
def test_fuzz(gpu, seed):
    cx.run_fuzz(gpu, SHAPES, seed)


def test_complexity_plan_through_torch(gpu):
    cx.run_python_layers(gpu, SHAPES, "cuda:0")


def test_filter_columns_with_complexity(gpu):
    cx.run_filter_columns(gpu, SHAPES, "cuda:0")


def test_filter_pairs_with_complexity(gpu):
    cx.run_filter_pairs(gpu, SHAPES, "cuda:0")


def test_closed_loop_through_torch(gpu):
    cx.run_closed_loop(gpu, SHAPES, "cuda:0")
