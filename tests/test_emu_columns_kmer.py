"""Columnar k-mer count (dsrcgpu_columns_kmer_count and the three calls on its table; dsrc_amd/csrc/k_columns_kmer.h) on the CPU: the
kernel sources compiled against the HIP emulator in tests/emu (workgroups of 256 threads), driven through the C ABI and both Python
layers, and compared with the integer model of tests/columns_kmer_cases.py.  Exact equality throughout."""
import os
import subprocess

import pytest

from tests import columns_kmer_cases as ck

SHAPES = ck.SHAPES["emu"]

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


def test_the_two_models_agree():
    ck.run_models_agree()


@pytest.mark.parametrize("k", ck.KS)
def test_geometry_lengths_and_alignments(emu, k):
    ck.run_geometry(emu, SHAPES, k)


def test_non_bases_break_their_windows(emu):
    ck.run_non_bases(emu, SHAPES)


def test_palindromes_and_the_two_strands(emu):
    ck.run_strands(emu, SHAPES)


def test_homopolymer_runs(emu):
    ck.run_homopolymers(emu, SHAPES)


def test_plans_in_empty_ranges_and_dropped_records(emu):
    ck.run_plans_in(emu, SHAPES)


@pytest.mark.parametrize("n", SHAPES["counts"])
def test_record_counts(emu, n):
    ck.run_count(emu, SHAPES, n)


def test_accumulate_and_merge(emu):
    ck.run_accumulate_and_merge(emu, SHAPES)


def test_hash_bits_change_nothing(emu):
    ck.run_hash_bits(emu, SHAPES)


def test_forced_overflow_present_means_exact(emu):
    ck.run_forced_overflow(emu, SHAPES)


def test_spectrum(emu):
    ck.run_spectrum(emu, SHAPES)


def test_lookup(emu):
    ck.run_lookup(emu, SHAPES)


def test_argument_refusals(emu):
    ck.run_arg_refusals(emu, SHAPES)


def test_input_errors(emu):
    ck.run_input_errors(emu, SHAPES)


def test_codec_state_is_left_alone(emu):
    ck.run_codec_state(emu, SHAPES)


@pytest.mark.parametrize("seed", range(SHAPES["kmer_fuzz"][0]))
def test_fuzz(emu, seed):
    ck.run_fuzz(emu, SHAPES, seed)


def test_count_kmers_through_torch(emu):
    ck.run_python_layers(emu, SHAPES, "cpu")


def test_filters_with_kmers(emu):
    ck.run_filters(emu, SHAPES, "cpu")


def test_closed_loop_through_torch(emu):
    ck.run_closed_loop(emu, SHAPES, "cpu")
