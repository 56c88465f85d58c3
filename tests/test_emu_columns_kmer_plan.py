"""Columnar k-mer plan (dsrcgpu_columns_kmer_plan; dsrc_amd/csrc/k_columns_kmer_plan.h) on the CPU: the kernel sources compiled against
the HIP emulator in tests/emu (workgroups of 256 threads), driven through the C ABI and both Python layers, and compared with the
integer model of tests/columns_kmer_plan_cases.py.  Exact equality throughout."""
import os
import subprocess

import pytest

from tests import columns_kmer_plan_cases as kp

SHAPES = kp.SHAPES["emu"]

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
    kp.run_models_agree()


@pytest.mark.parametrize("k", kp.KS)
def test_geometry_lengths_and_offsets(emu, k):
    kp.run_geometry(emu, SHAPES, k)


def test_first_miss_and_first_hit_positions(emu):
    kp.run_positions(emu, SHAPES)


def test_broken_windows(emu):
    kp.run_broken(emu, SHAPES)


def test_median(emu):
    kp.run_median(emu, SHAPES)


def test_count_above_the_cap(emu):
    kp.run_count_cap(emu, SHAPES)


def test_lds_boundary(emu):
    kp.run_lds_boundary(emu, SHAPES)


def test_the_two_strands_and_palindromes(emu):
    kp.run_strands(emu, SHAPES)


def test_hash_bits_change_nothing(emu):
    kp.run_hash_bits(emu, SHAPES)


def test_plans_in_empty_ranges_dropped_records_in_place(emu):
    kp.run_plans_in(emu, SHAPES)


def test_reasons(emu):
    kp.run_reasons(emu, SHAPES)


@pytest.mark.parametrize("n", SHAPES["counts"])
def test_record_counts(emu, n):
    kp.run_count(emu, SHAPES, n)


def test_argument_refusals(emu):
    kp.run_arg_refusals(emu, SHAPES)


def test_input_errors(emu):
    kp.run_input_errors(emu, SHAPES)


def test_codec_state_is_left_alone(emu):
    kp.run_codec_state(emu, SHAPES)


@pytest.mark.parametrize("seed", range(SHAPES["plan_fuzz"][0]))
def test_fuzz(emu, seed):
    kp.run_fuzz(emu, SHAPES, seed)


def test_kmer_plan_through_torch(emu):
    kp.run_python_layers(emu, SHAPES, "cpu")


def test_filters_with_a_screen(emu):
    kp.run_filters(emu, SHAPES, "cpu")


def test_closed_loop_through_torch(emu):
    kp.run_closed_loop(emu, SHAPES, "cpu")
