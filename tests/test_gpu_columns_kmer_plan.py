"""Columnar k-mer plan (dsrcgpu_columns_kmer_plan; dsrc_amd/csrc/k_columns_kmer_plan.h) on the MI355X: the product library, through the
C ABI and both Python layers, compared with the integer model of tests/columns_kmer_plan_cases.py -- the same cases as
tests/test_emu_columns_kmer_plan.py, here with workgroups of 1024 threads, the full fuzz and the record count that takes the
wave-per-record grid stride into a second round.  Exact equality throughout."""
import os

import pytest

from tests import columns_kmer_plan_cases as kp

SHAPES = kp.SHAPES["gpu"]

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    os.environ.pop("DSRC_GPU_LIB", None)
    from dsrc_amd import _lib
    _lib._lib = None
    return _lib


@pytest.mark.parametrize("k", kp.KS)
def test_geometry_lengths_and_offsets(gpu, k):
    kp.run_geometry(gpu, SHAPES, k)


def test_first_miss_and_first_hit_positions(gpu):
    kp.run_positions(gpu, SHAPES)


def test_broken_windows(gpu):
    kp.run_broken(gpu, SHAPES)


def test_median(gpu):
    kp.run_median(gpu, SHAPES)


def test_count_above_the_cap(gpu):
    kp.run_count_cap(gpu, SHAPES)


def test_lds_boundary(gpu):
    kp.run_lds_boundary(gpu, SHAPES)


def test_the_two_strands_and_palindromes(gpu):
    kp.run_strands(gpu, SHAPES)


def test_hash_bits_change_nothing(gpu):
    kp.run_hash_bits(gpu, SHAPES)


def test_plans_in_empty_ranges_dropped_records_in_place(gpu):
    kp.run_plans_in(gpu, SHAPES)


def test_reasons(gpu):
    kp.run_reasons(gpu, SHAPES)


@pytest.mark.parametrize("n", SHAPES["counts"])
def test_record_counts(gpu, n):
    kp.run_count(gpu, SHAPES, n)


def test_grid_stride_second_round(gpu):
    kp.run_grid_stride(gpu, SHAPES)


def test_argument_refusals(gpu):
    kp.run_arg_refusals(gpu, SHAPES)


def test_input_errors(gpu):
    kp.run_input_errors(gpu, SHAPES)


def test_codec_state_is_left_alone(gpu):
    kp.run_codec_state(gpu, SHAPES)


@pytest.mark.parametrize("seed", range(SHAPES["plan_fuzz"][0]))
def test_fuzz(gpu, seed):
    kp.run_fuzz(gpu, SHAPES, seed)


def test_kmer_plan_through_torch(gpu):
    kp.run_python_layers(gpu, SHAPES, "cuda:0")


def test_filters_with_a_screen(gpu):
    kp.run_filters(gpu, SHAPES, "cuda:0")


def test_closed_loop_through_torch(gpu):
    kp.run_closed_loop(gpu, SHAPES, "cuda:0")
