"""Columnar complexity plan (dsrcgpu_columns_complexity_plan; dsrc_amd/csrc/k_columns_complexity.h) on the CPU: the kernel sources
compiled against the HIP emulator in tests/emu (workgroups of 256 threads), driven through the C ABI and both Python layers, and
compared with the integer model of tests/columns_complexity_cases.py.  Exact equality throughout."""
import os
import subprocess

import pytest

from tests import columns_complexity_cases as cx

SHAPES = cx.SHAPES["emu"]

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


def test_model_forms_agree(emu):
    cx.run_model_forms(emu, SHAPES)


@pytest.mark.parametrize("base", range(4))
def test_geometry_of_runs(emu, base):
    cx.run_geometry(emu, SHAPES, base)


@pytest.mark.parametrize("rate", cx.RATES)
def test_error_budget_exact_and_one_more(emu, rate):
    cx.run_budget(emu, SHAPES, rate)


def test_the_score(emu):
    cx.run_score(emu, SHAPES)


def test_complexity(emu):
    cx.run_complexity(emu, SHAPES)


def test_dust_lengths(emu):
    cx.run_dust_lengths(emu, SHAPES)


def test_dust_windows_and_thresholds(emu):
    cx.run_dust_windows(emu, SHAPES)


def test_dust_triplet_mapping(emu):
    cx.run_dust_triplets(emu, SHAPES)


def test_ranges_keep_in_place_and_info(emu):
    cx.run_ranges(emu, SHAPES)


def test_argument_refusals(emu):
    cx.run_arg_refusals(emu, SHAPES)


def test_input_errors(emu):
    cx.run_input_errors(emu, SHAPES)


def test_codec_state_is_left_alone(emu):
    cx.run_codec_state(emu, SHAPES)


@pytest.mark.parametrize("n", SHAPES["counts"])
def test_record_counts(emu, n):
    cx.run_count(emu, SHAPES, n)


def test_fuzz_exercises_every_statistic(emu):
    cx.run_fuzz_exercises_everything(emu, SHAPES)


@pytest.mark.parametrize("seed", range(SHAPES["cplx_fuzz"][0]))
def test_fuzz(emu, seed):
    cx.run_fuzz(emu, SHAPES, seed)


def test_complexity_plan_through_torch(emu):
    cx.run_python_layers(emu, SHAPES, "cpu")


def test_filter_columns_with_complexity(emu):
    cx.run_filter_columns(emu, SHAPES, "cpu")


def test_filter_pairs_with_complexity(emu):
    cx.run_filter_pairs(emu, SHAPES, "cpu")


def test_closed_loop_through_torch(emu):
    cx.run_closed_loop(emu, SHAPES, "cpu")
