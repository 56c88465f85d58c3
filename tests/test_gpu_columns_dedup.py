"""Columnar dedup plan (dsrcgpu_columns_dedup_plan; dsrc_amd/csrc/k_columns_dedup.h) on the MI355X: the product library, through the
C ABI and both Python layers, compared with the integer model of tests/columns_dedup_cases.py -- the same cases as
tests/test_emu_columns_dedup.py, here with workgroups of 1024 threads, the full fuzz, the contention batch (every record on one of
three table slots, twice) and the record count that takes the wave-per-record grid stride into a second round.  Exact equality
throughout."""
import os

import pytest

from tests import columns_dedup_cases as cd

SHAPES = cd.SHAPES["gpu"]

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    os.environ.pop("DSRC_GPU_LIB", None)
    from dsrc_amd import _lib
    _lib._lib = None
    return _lib


def test_geometry_lengths_alignments_codes(gpu):
    cd.run_geometry(gpu, SHAPES)


def test_key_bases(gpu):
    cd.run_key_bases(gpu, SHAPES)


def test_prefer_first_and_quality(gpu):
    cd.run_prefer(gpu, SHAPES)


def test_plans_in_in_place_and_null_outputs(gpu):
    cd.run_plans_in(gpu, SHAPES)


def test_pairs_are_keyed_on_both_mates(gpu):
    cd.run_pairs(gpu, SHAPES)


def test_hash_bits_change_nothing(gpu):
    cd.run_hash_bits(gpu, SHAPES)


@pytest.mark.parametrize("n", SHAPES["counts"])
def test_record_counts(gpu, n):
    cd.run_count(gpu, SHAPES, n)


def test_argument_refusals(gpu):
    cd.run_arg_refusals(gpu, SHAPES)


def test_input_errors(gpu):
    cd.run_input_errors(gpu, SHAPES)


def test_codec_state_is_left_alone(gpu):
    cd.run_codec_state(gpu, SHAPES)


@pytest.mark.parametrize("seed", range(SHAPES["dedup_fuzz"][0]))
def test_fuzz(gpu, seed):
    cd.run_fuzz(gpu, SHAPES, seed)


def test_dedup_plan_through_torch(gpu):
    cd.run_python_layers(gpu, SHAPES, "cuda:0")


def test_filter_columns_with_dedup(gpu):
    cd.run_filter_columns(gpu, SHAPES, "cuda:0")


def test_filter_pairs_with_dedup(gpu):
    cd.run_filter_pairs(gpu, SHAPES, "cuda:0")


def test_closed_loop_through_torch(gpu):
    cd.run_closed_loop(gpu, SHAPES, "cuda:0")


def test_contention_three_slots_twice(gpu):
    cd.run_contention(gpu, SHAPES)


def test_grid_stride_second_round(gpu):
    cd.run_grid_stride(gpu, SHAPES)
