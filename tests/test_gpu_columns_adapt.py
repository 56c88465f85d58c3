"""Columnar adapter trim (dsrcgpu_columns_adapter_plan; dsrc_amd/csrc/k_columns_adapt.h) on the MI355X: the product library,
through the C ABI and both Python layers, compared with the integer model of tests/columns_adapt_cases.py -- the same cases as
tests/test_emu_columns_adapt.py, here with workgroups of 1024 threads, the full fuzz and the record count that takes the planner's
grid stride into a second round.  Exact equality throughout."""
import os

import pytest

from tests import columns_adapt_cases as ca

SHAPES = ca.SHAPES["gpu"]

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    os.environ.pop("DSRC_GPU_LIB", None)
    from dsrc_amd import _lib
    _lib._lib = None
    return _lib


@pytest.mark.parametrize("la", ca.ADAPTER_LENGTHS)
def test_geometry_lengths_positions_overhang(gpu, la):
    ca.run_geometry(gpu, SHAPES, la)


@pytest.mark.parametrize("rate", ca.RATES)
def test_error_budget_exact_and_one_more(gpu, rate):
    ca.run_budget(gpu, SHAPES, rate)


def test_error_budget_edges(gpu):
    ca.run_budget_edges(gpu, SHAPES)


def test_which_hit(gpu):
    ca.run_which_hit(gpu, SHAPES)


def test_ranges_in(gpu):
    ca.run_ranges(gpu, SHAPES)


def test_keep_min_length_in_place_and_stats(gpu):
    ca.run_keep_and_inplace(gpu, SHAPES)


def test_argument_refusals(gpu):
    ca.run_arg_refusals(gpu, SHAPES)


def test_input_errors(gpu):
    ca.run_input_errors(gpu, SHAPES)


def test_codec_state_is_left_alone(gpu):
    ca.run_codec_state(gpu, SHAPES)


@pytest.mark.parametrize("n", SHAPES["counts"])
def test_record_counts(gpu, n):
    ca.run_count(gpu, SHAPES, n)


def test_grid_stride_second_round(gpu):
    ca.run_count(gpu, SHAPES, SHAPES["stride_count"])


@pytest.mark.parametrize("seed", range(SHAPES["adapt_fuzz"][0]))
def test_fuzz(gpu, seed):
    ca.run_fuzz(gpu, SHAPES, seed)


def test_adapter_plan_through_torch(gpu):
    ca.run_python_layers(gpu, SHAPES, "cuda:0")


def test_filter_columns_with_adapters(gpu):
    ca.run_filter_columns(gpu, SHAPES, "cuda:0")


def test_closed_loop_through_torch(gpu):
    ca.run_closed_loop(gpu, SHAPES, "cuda:0")
