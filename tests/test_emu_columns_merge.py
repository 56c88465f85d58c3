"""Columnar merge (dsrcgpu_columns_merge_device; dsrc_amd/csrc/k_columns_merge.h) on the CPU: the kernel sources compiled against
the HIP emulator in tests/emu (workgroups of 256 threads), driven through the C ABI and both Python layers, and compared with the
integer model of tests/columns_merge_cases.py.  Exact equality throughout."""
import os
import subprocess

import pytest

from tests import columns_merge_cases as cm

SHAPES = cm.SHAPES["emu"]

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


def test_geometry_overlaps_lengths_offsets(emu):
    cm.run_geometry(emu, SHAPES)


def test_consensus(emu):
    cm.run_consensus(emu, SHAPES)


def test_reasons_and_their_order(emu):
    cm.run_reasons(emu, SHAPES)


@pytest.mark.parametrize("rate", cm.BUDGET_RATES)
def test_budget_exact_and_one_more(emu, rate):
    cm.run_budget(emu, SHAPES, rate)


@pytest.mark.parametrize("seed", range(SHAPES["pair_fuzz"][0]))
def test_behind_the_pair_plan(emu, seed):
    cm.run_with_pair_plan(emu, SHAPES, seed)


def test_capacities_and_empty_cases(emu):
    cm.run_capacity(emu, SHAPES)


def test_argument_refusals(emu):
    cm.run_arg_refusals(emu, SHAPES)


def test_input_errors(emu):
    cm.run_input_errors(emu, SHAPES)


def test_codec_state_is_left_alone(emu):
    cm.run_codec_state(emu, SHAPES)


@pytest.mark.parametrize("n", SHAPES["counts"])
def test_pair_counts(emu, n):
    cm.run_count(emu, SHAPES, n)


def test_second_pair_of_a_wave(emu):
    cm.run_second_pair_of_a_wave(emu, SHAPES)


def test_merge_pairs_through_torch(emu):
    cm.run_python_layers(emu, SHAPES, "cpu")


def test_filter_pairs_with_merge(emu):
    cm.run_filter_pairs(emu, SHAPES, "cpu")


def test_closed_loop_through_torch(emu):
    cm.run_closed_loop(emu, SHAPES, "cpu")
