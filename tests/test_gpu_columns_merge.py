"""Columnar merge (dsrcgpu_columns_merge_device; dsrc_amd/csrc/k_columns_merge.h) on the MI355X: the product library, through the
C ABI and both Python layers, compared with the integer model of tests/columns_merge_cases.py -- the same cases as
tests/test_emu_columns_merge.py, here with workgroups of 1024 threads, the full pair-plan fuzz and the pair count that takes the
judge's and the writer's grid stride into a second round.  Exact equality throughout."""
import os

import pytest

from tests import columns_merge_cases as cm

SHAPES = cm.SHAPES["gpu"]

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    os.environ.pop("DSRC_GPU_LIB", None)
    from dsrc_amd import _lib
    _lib._lib = None
    return _lib


def test_geometry_overlaps_lengths_offsets(gpu):
    cm.run_geometry(gpu, SHAPES)


def test_consensus(gpu):
    cm.run_consensus(gpu, SHAPES)


def test_reasons_and_their_order(gpu):
    cm.run_reasons(gpu, SHAPES)


@pytest.mark.parametrize("rate", cm.BUDGET_RATES)
def test_budget_exact_and_one_more(gpu, rate):
    cm.run_budget(gpu, SHAPES, rate)


@pytest.mark.parametrize("seed", range(SHAPES["pair_fuzz"][0]))
def test_behind_the_pair_plan(gpu, seed):
    cm.run_with_pair_plan(gpu, SHAPES, seed)


def test_capacities_and_empty_cases(gpu):
    cm.run_capacity(gpu, SHAPES)


def test_argument_refusals(gpu):
    cm.run_arg_refusals(gpu, SHAPES)


def test_input_errors(gpu):
    cm.run_input_errors(gpu, SHAPES)


def test_codec_state_is_left_alone(gpu):
    cm.run_codec_state(gpu, SHAPES)


@pytest.mark.parametrize("n", SHAPES["counts"])
def test_pair_counts(gpu, n):
    cm.run_count(gpu, SHAPES, n)


def test_grid_stride_second_round(gpu):
    cm.run_count(gpu, SHAPES, SHAPES["stride_count"])


def test_second_pair_of_a_wave(gpu):
    cm.run_second_pair_of_a_wave(gpu, SHAPES)


def test_merge_pairs_through_torch(gpu):
    cm.run_python_layers(gpu, SHAPES, "cuda:0")


def test_filter_pairs_with_merge(gpu):
    cm.run_filter_pairs(gpu, SHAPES, "cuda:0")


def test_closed_loop_through_torch(gpu):
    cm.run_closed_loop(gpu, SHAPES, "cuda:0")
