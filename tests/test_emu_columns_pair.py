"""Columnar pair plan (dsrcgpu_columns_pair_plan; dsrc_amd/csrc/k_columns_pair.h) on the CPU: the kernel sources compiled against
the HIP emulator in tests/emu (workgroups of 256 threads), driven through the C ABI and both Python layers, and compared with the
integer model of tests/columns_pair_cases.py.  Exact equality throughout."""
import os
import subprocess

import pytest

from tests import columns_pair_cases as cp

SHAPES = cp.SHAPES["emu"]

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


@pytest.mark.parametrize("k", range(3))
def test_geometry_lengths_shifts_candidates(emu, k):
    cp.run_geometry(emu, SHAPES, k)


@pytest.mark.parametrize("rate", cp.RATES)
def test_budget_exact_and_one_more(emu, rate):
    cp.run_budget(emu, SHAPES, rate)


def test_budget_edges(emu):
    cp.run_budget_edges(emu, SHAPES)


def test_which_candidate(emu):
    cp.run_which_candidate(emu, SHAPES)


def test_plans_in(emu):
    cp.run_plans_in(emu, SHAPES)


def test_keep_min_length_in_place_stats_and_long_ranges(emu):
    cp.run_keep_and_inplace(emu, SHAPES)


def test_argument_refusals(emu):
    cp.run_arg_refusals(emu, SHAPES)


def test_input_errors(emu):
    cp.run_input_errors(emu, SHAPES)


def test_codec_state_is_left_alone(emu):
    cp.run_codec_state(emu, SHAPES)


@pytest.mark.parametrize("n", SHAPES["counts"])
def test_pair_counts(emu, n):
    cp.run_count(emu, SHAPES, n)


def test_second_pair_of_a_wave_finds_no_stale_planes(emu):
    cp.run_second_pair_of_a_wave(emu, SHAPES)


@pytest.mark.parametrize("seed", range(SHAPES["pair_fuzz"][0]))
def test_fuzz(emu, seed):
    cp.run_fuzz(emu, SHAPES, seed)


def test_pair_plan_through_torch(emu):
    cp.run_python_layers(emu, SHAPES, "cpu")


def test_filter_pairs(emu):
    cp.run_filter_pairs(emu, SHAPES, "cpu")


def test_closed_loop_through_torch(emu):
    cp.run_closed_loop(emu, SHAPES, "cpu")
