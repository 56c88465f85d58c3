"""Columnar dedup plan (dsrcgpu_columns_dedup_plan; dsrc_amd/csrc/k_columns_dedup.h) on the CPU: the kernel sources compiled against
the HIP emulator in tests/emu (workgroups of 256 threads), driven through the C ABI and both Python layers, and compared with the
integer model of tests/columns_dedup_cases.py.  Exact equality throughout."""
import os
import subprocess

import pytest

from tests import columns_dedup_cases as cd

SHAPES = cd.SHAPES["emu"]

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


def test_geometry_lengths_alignments_codes(emu):
    cd.run_geometry(emu, SHAPES)


def test_key_bases(emu):
    cd.run_key_bases(emu, SHAPES)


def test_prefer_first_and_quality(emu):
    cd.run_prefer(emu, SHAPES)


def test_plans_in_in_place_and_null_outputs(emu):
    cd.run_plans_in(emu, SHAPES)


def test_pairs_are_keyed_on_both_mates(emu):
    cd.run_pairs(emu, SHAPES)


def test_hash_bits_change_nothing(emu):
    cd.run_hash_bits(emu, SHAPES)


@pytest.mark.parametrize("n", SHAPES["counts"])
def test_record_counts(emu, n):
    cd.run_count(emu, SHAPES, n)


def test_argument_refusals(emu):
    cd.run_arg_refusals(emu, SHAPES)


def test_input_errors(emu):
    cd.run_input_errors(emu, SHAPES)


def test_codec_state_is_left_alone(emu):
    cd.run_codec_state(emu, SHAPES)


@pytest.mark.parametrize("seed", range(SHAPES["dedup_fuzz"][0]))
def test_fuzz(emu, seed):
    cd.run_fuzz(emu, SHAPES, seed)


def test_dedup_plan_through_torch(emu):
    cd.run_python_layers(emu, SHAPES, "cpu")


def test_filter_columns_with_dedup(emu):
    cd.run_filter_columns(emu, SHAPES, "cpu")


def test_filter_pairs_with_dedup(emu):
    cd.run_filter_pairs(emu, SHAPES, "cpu")


def test_closed_loop_through_torch(emu):
    cd.run_closed_loop(emu, SHAPES, "cpu")
