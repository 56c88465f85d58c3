"""Columnar k-mer correction (dsrcgpu_columns_kmer_correct; dsrc_amd/csrc/k_columns_kmer_correct.h) on the CPU: the kernel sources compiled
against the HIP emulator in tests/emu (workgroups of 256 threads), driven through the C ABI and both Python layers, and compared with
the integer model of tests/columns_kmer_correct_cases.py.  Exact equality throughout."""
import os
import subprocess

import pytest

from tests import columns_kmer_correct_cases as kc

SHAPES = kc.SHAPES["emu"]

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
    kc.run_models_agree()


def test_the_rule_halves_the_errors_and_spoils_nothing():
    kc.run_accuracy()


def test_the_fuzz_seeds_reach_every_verdict():
    kc.run_fuzz_covers(SHAPES)


def test_hand_cases(emu):
    kc.run_hand(emu, SHAPES)


@pytest.mark.parametrize("k", kc.KS)
def test_placement_and_its_borders(emu, k):
    kc.run_placement(emu, SHAPES, k)


def test_step_borders(emu):
    kc.run_step_borders(emu, SHAPES)


def test_codes_that_are_no_bases(emu):
    kc.run_ns(emu, SHAPES)


def test_ambiguity_no_candidate_quality_min_count(emu):
    kc.run_verdicts(emu, SHAPES)


def test_the_two_strands_and_palindromes(emu):
    kc.run_strands(emu, SHAPES)


def test_hash_bits_change_nothing(emu):
    kc.run_hash_bits(emu, SHAPES)


def test_plans_in_slices_pads_in_place(emu):
    kc.run_plans_in(emu, SHAPES)


def test_a_long_record(emu):
    kc.run_long_record(emu, SHAPES)


@pytest.mark.parametrize("n", SHAPES["counts"])
def test_record_counts(emu, n):
    kc.run_count(emu, SHAPES, n)


def test_idempotence(emu):
    kc.run_idempotent(emu, SHAPES)


def test_argument_refusals(emu):
    kc.run_arg_refusals(emu, SHAPES)


def test_input_errors(emu):
    kc.run_input_errors(emu, SHAPES)


def test_codec_state_is_left_alone(emu):
    kc.run_codec_state(emu, SHAPES)


@pytest.mark.parametrize("seed", range(SHAPES["correct_fuzz"][0]))
def test_fuzz(emu, seed):
    kc.run_fuzz(emu, SHAPES, seed)


def test_correct_kmers_through_torch(emu):
    kc.run_python_layers(emu, SHAPES, "cpu")


def test_filters_with_a_correction(emu):
    kc.run_filters(emu, SHAPES, "cpu")


def test_closed_loop_through_torch(emu):
    kc.run_closed_loop(emu, SHAPES, "cpu")
