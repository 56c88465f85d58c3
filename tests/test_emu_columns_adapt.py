"""Columnar adapter trim (dsrcgpu_columns_adapter_plan; dsrc_amd/csrc/k_columns_adapt.h) on the CPU: the kernel sources compiled
against the HIP emulator in tests/emu (workgroups of 256 threads), driven through the C ABI and both Python layers, and compared
with the integer model of tests/columns_adapt_cases.py.  Exact equality throughout."""
import os
import subprocess

import pytest

from tests import columns_adapt_cases as ca

SHAPES = ca.SHAPES["emu"]

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


@pytest.mark.parametrize("la", ca.ADAPTER_LENGTHS)
def test_geometry_lengths_positions_overhang(emu, la):
    ca.run_geometry(emu, SHAPES, la)


@pytest.mark.parametrize("rate", ca.RATES)
def test_error_budget_exact_and_one_more(emu, rate):
    ca.run_budget(emu, SHAPES, rate)


def test_error_budget_edges(emu):
    ca.run_budget_edges(emu, SHAPES)


def test_which_hit(emu):
    ca.run_which_hit(emu, SHAPES)


def test_ranges_in(emu):
    ca.run_ranges(emu, SHAPES)


def test_keep_min_length_in_place_and_stats(emu):
    ca.run_keep_and_inplace(emu, SHAPES)


def test_argument_refusals(emu):
    ca.run_arg_refusals(emu, SHAPES)


def test_input_errors(emu):
    ca.run_input_errors(emu, SHAPES)


def test_codec_state_is_left_alone(emu):
    ca.run_codec_state(emu, SHAPES)


@pytest.mark.parametrize("n", SHAPES["counts"])
def test_record_counts(emu, n):
    ca.run_count(emu, SHAPES, n)


@pytest.mark.parametrize("seed", range(SHAPES["adapt_fuzz"][0]))
def test_fuzz(emu, seed):
    ca.run_fuzz(emu, SHAPES, seed)


def test_adapter_plan_through_torch(emu):
    ca.run_python_layers(emu, SHAPES, "cpu")


def test_filter_columns_with_adapters(emu):
    ca.run_filter_columns(emu, SHAPES, "cpu")


def test_closed_loop_through_torch(emu):
    ca.run_closed_loop(emu, SHAPES, "cpu")
