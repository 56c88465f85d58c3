"""Columnar select (dsrcgpu_columns_trim_plan, dsrcgpu_columns_select_device; dsrc_amd/csrc/k_columns_sel.h) on the CPU: the kernel
sources compiled against the HIP emulator in tests/emu (workgroups of 256 threads), driven through the C ABI and both Python
layers, and compared with the integer model of tests/columns_sel_cases.py.  Exact equality throughout."""
import os
import subprocess

import pytest

from tests import columns_sel_cases as cs

SHAPES = cs.SHAPES["emu"]

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


@pytest.mark.parametrize("cutoff", [1, 20, 41, 255])
def test_plan_lengths_patterns_modes(emu, cutoff):
    cs.run_plan_crafted(emu, SHAPES, cutoff)


def test_plan_ties_breaks_and_crossing(emu):
    cs.run_plan_model_says(emu, SHAPES)


def test_plan_refusals_and_edges(emu):
    cs.run_plan_refusals(emu, SHAPES)


def test_plan_filters(emu):
    cs.run_plan_filters(emu, SHAPES)


@pytest.mark.parametrize("seed", range(SHAPES["sel_fuzz"][0]))
def test_plan_fuzz(emu, seed):
    cs.run_plan_fuzz(emu, SHAPES, seed)


def test_plan_start_offset_and_input_errors(emu):
    cs.run_plan_offset_and_errors(emu, SHAPES)


def test_select_keep_patterns(emu):
    cs.run_select_patterns(emu, SHAPES)


@pytest.mark.parametrize("n", SHAPES["counts"])
def test_select_record_counts(emu, n):
    cs.run_select_count(emu, SHAPES, n)


def test_select_titles_source_and_host_path(emu):
    cs.run_select_titles(emu, SHAPES)


def test_select_capacity(emu):
    cs.run_select_capacity(emu, SHAPES)


def test_select_start_offset_and_no_records(emu):
    cs.run_select_offset(emu, SHAPES)


def test_select_input_errors(emu):
    cs.run_select_input_errors(emu, SHAPES)


def test_closed_loop_through_torch(emu):
    cs.run_closed_loop(emu, SHAPES, "cpu")


def test_codec_state_is_left_alone(emu):
    cs.run_codec_state(emu, SHAPES)


def test_mates_stay_in_step(emu):
    cs.run_mates(emu, SHAPES, "cpu")
