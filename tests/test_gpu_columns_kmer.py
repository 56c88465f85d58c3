"""Columnar k-mer count (dsrcgpu_columns_kmer_count and the three calls on its table; dsrc_amd/csrc/k_columns_kmer.h) on the MI355X:
the product library, through the C ABI and both Python layers, compared with the integer model of tests/columns_kmer_cases.py -- the
same cases as tests/test_emu_columns_kmer.py, here with workgroups of 1024 threads, the full fuzz, the contention batch (20 000 reads
of three sequences, twice, equal sorted tables) and the record count that takes the wave-per-record grid stride into a second round.
Exact equality throughout."""
import os

import pytest

from tests import columns_kmer_cases as ck

SHAPES = ck.SHAPES["gpu"]

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    os.environ.pop("DSRC_GPU_LIB", None)
    from dsrc_amd import _lib
    _lib._lib = None
    return _lib


@pytest.mark.parametrize("k", ck.KS)
def test_geometry_lengths_and_alignments(gpu, k):
    ck.run_geometry(gpu, SHAPES, k)


def test_non_bases_break_their_windows(gpu):
    ck.run_non_bases(gpu, SHAPES)


def test_palindromes_and_the_two_strands(gpu):
    ck.run_strands(gpu, SHAPES)


def test_homopolymer_runs(gpu):
    ck.run_homopolymers(gpu, SHAPES)


def test_plans_in_empty_ranges_and_dropped_records(gpu):
    ck.run_plans_in(gpu, SHAPES)


@pytest.mark.parametrize("n", SHAPES["counts"])
def test_record_counts(gpu, n):
    ck.run_count(gpu, SHAPES, n)


def test_accumulate_and_merge(gpu):
    ck.run_accumulate_and_merge(gpu, SHAPES)


def test_hash_bits_change_nothing(gpu):
    ck.run_hash_bits(gpu, SHAPES)


def test_forced_overflow_present_means_exact(gpu):
    ck.run_forced_overflow(gpu, SHAPES)


def test_spectrum(gpu):
    ck.run_spectrum(gpu, SHAPES)


def test_lookup(gpu):
    ck.run_lookup(gpu, SHAPES)


def test_argument_refusals(gpu):
    ck.run_arg_refusals(gpu, SHAPES)


def test_input_errors(gpu):
    ck.run_input_errors(gpu, SHAPES)


def test_codec_state_is_left_alone(gpu):
    ck.run_codec_state(gpu, SHAPES)


@pytest.mark.parametrize("seed", range(SHAPES["kmer_fuzz"][0]))
def test_fuzz(gpu, seed):
    ck.run_fuzz(gpu, SHAPES, seed)


def test_count_kmers_through_torch(gpu):
    ck.run_python_layers(gpu, SHAPES, "cuda:0")


def test_filters_with_kmers(gpu):
    ck.run_filters(gpu, SHAPES, "cuda:0")


def test_closed_loop_through_torch(gpu):
    ck.run_closed_loop(gpu, SHAPES, "cuda:0")


def test_contention_three_sequences_twice(gpu):
    ck.run_contention(gpu, SHAPES)


def test_grid_stride_second_round(gpu):
    ck.run_grid_stride(gpu, SHAPES)
