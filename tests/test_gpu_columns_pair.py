"""Columnar pair plan (dsrcgpu_columns_pair_plan; dsrc_amd/csrc/k_columns_pair.h) on the MI355X: the product library, through the
C ABI and both Python layers, compared with the integer model of tests/columns_pair_cases.py -- the same cases as
tests/test_emu_columns_pair.py, here with workgroups of 1024 threads, the full fuzz and the pair count that takes the planner's grid
stride into a second round.  Exact equality throughout."""
import os

import pytest

from tests import columns_pair_cases as cp

SHAPES = cp.SHAPES["gpu"]

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    os.environ.pop("DSRC_GPU_LIB", None)
    from dsrc_amd import _lib
    _lib._lib = None
    return _lib


@pytest.mark.parametrize("k", range(3))
def test_geometry_lengths_shifts_candidates(gpu, k):
    cp.run_geometry(gpu, SHAPES, k)


@pytest.mark.parametrize("rate", cp.RATES)
def test_budget_exact_and_one_more(gpu, rate):
    cp.run_budget(gpu, SHAPES, rate)


def test_budget_edges(gpu):
    cp.run_budget_edges(gpu, SHAPES)


def test_which_candidate(gpu):
    cp.run_which_candidate(gpu, SHAPES)


def test_plans_in(gpu):
    cp.run_plans_in(gpu, SHAPES)


def test_keep_min_length_in_place_stats_and_long_ranges(gpu):
    cp.run_keep_and_inplace(gpu, SHAPES)


def test_argument_refusals(gpu):
    cp.run_arg_refusals(gpu, SHAPES)


def test_input_errors(gpu):
    cp.run_input_errors(gpu, SHAPES)


def test_codec_state_is_left_alone(gpu):
    cp.run_codec_state(gpu, SHAPES)


@pytest.mark.parametrize("n", SHAPES["counts"])
def test_pair_counts(gpu, n):
    cp.run_count(gpu, SHAPES, n)


def test_grid_stride_second_round(gpu):
    cp.run_count(gpu, SHAPES, SHAPES["stride_count"])


def test_second_pair_of_a_wave_finds_no_stale_planes(gpu):
    cp.run_second_pair_of_a_wave(gpu, SHAPES)


@pytest.mark.parametrize("seed", range(SHAPES["pair_fuzz"][0]))
def test_fuzz(gpu, seed):
    cp.run_fuzz(gpu, SHAPES, seed)


def test_pair_plan_through_torch(gpu):
    cp.run_python_layers(gpu, SHAPES, "cuda:0")


def test_filter_pairs(gpu):
    cp.run_filter_pairs(gpu, SHAPES, "cuda:0")


def test_closed_loop_through_torch(gpu):
    cp.run_closed_loop(gpu, SHAPES, "cuda:0")
