"""Columnar k-mer correction (dsrcgpu_columns_kmer_correct; dsrc_amd/csrc/k_columns_kmer_correct.h) on the MI355X: the product library,
through the C ABI and both Python layers, compared with the integer model of tests/columns_kmer_correct_cases.py -- the same cases as
tests/test_emu_columns_kmer_correct.py, here with workgroups of 1024 threads, the full fuzz and the record count that takes the
wave-per-record grid stride into a second round.  Exact equality throughout."""
import os

import pytest

from tests import columns_kmer_correct_cases as kc

SHAPES = kc.SHAPES["gpu"]

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    os.environ.pop("DSRC_GPU_LIB", None)
    from dsrc_amd import _lib
    _lib._lib = None
    return _lib


def test_the_fuzz_seeds_reach_every_verdict():
    kc.run_fuzz_covers(SHAPES)


def test_hand_cases(gpu):
    kc.run_hand(gpu, SHAPES)


@pytest.mark.parametrize("k", kc.KS)
def test_placement_and_its_borders(gpu, k):
    kc.run_placement(gpu, SHAPES, k)


def test_step_borders(gpu):
    kc.run_step_borders(gpu, SHAPES)


def test_codes_that_are_no_bases(gpu):
    kc.run_ns(gpu, SHAPES)


def test_ambiguity_no_candidate_quality_min_count(gpu):
    kc.run_verdicts(gpu, SHAPES)


def test_the_two_strands_and_palindromes(gpu):
    kc.run_strands(gpu, SHAPES)


def test_hash_bits_change_nothing(gpu):
    kc.run_hash_bits(gpu, SHAPES)


def test_plans_in_slices_pads_in_place(gpu):
    kc.run_plans_in(gpu, SHAPES)


def test_a_long_record(gpu):
    kc.run_long_record(gpu, SHAPES)


@pytest.mark.parametrize("n", SHAPES["counts"])
def test_record_counts(gpu, n):
    kc.run_count(gpu, SHAPES, n)


def test_grid_stride_second_round(gpu):
    kc.run_grid_stride(gpu, SHAPES)


def test_idempotence(gpu):
    kc.run_idempotent(gpu, SHAPES)


def test_argument_refusals(gpu):
    kc.run_arg_refusals(gpu, SHAPES)


def test_input_errors(gpu):
    kc.run_input_errors(gpu, SHAPES)


def test_codec_state_is_left_alone(gpu):
    kc.run_codec_state(gpu, SHAPES)


@pytest.mark.parametrize("seed", range(SHAPES["correct_fuzz"][0]))
def test_fuzz(gpu, seed):
    kc.run_fuzz(gpu, SHAPES, seed)


def test_correct_kmers_through_torch(gpu):
    kc.run_python_layers(gpu, SHAPES, "cuda:0")


def test_filters_with_a_correction(gpu):
    kc.run_filters(gpu, SHAPES, "cuda:0")


def test_closed_loop_through_torch(gpu):
    kc.run_closed_loop(gpu, SHAPES, "cuda:0")
