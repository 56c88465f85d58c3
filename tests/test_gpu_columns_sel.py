"""Columnar select (dsrcgpu_columns_trim_plan, dsrcgpu_columns_select_device; dsrc_amd/csrc/k_columns_sel.h) on the MI355X: the
product library, through the C ABI and both Python layers, compared with the integer model of tests/columns_sel_cases.py -- the
same cases as tests/test_emu_columns_sel.py, here with workgroups of 1024 threads, the full fuzz and the record count that takes
the scan of the tile sums into a second round.  Exact equality throughout."""
import os

import pytest

from tests import columns_sel_cases as cs

SHAPES = cs.SHAPES["gpu"]

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    os.environ.pop("DSRC_GPU_LIB", None)
    from dsrc_amd import _lib
    _lib._lib = None
    return _lib


@pytest.mark.parametrize("cutoff", [1, 20, 41, 255])
def test_plan_lengths_patterns_modes(gpu, cutoff):
    cs.run_plan_crafted(gpu, SHAPES, cutoff)


def test_plan_ties_breaks_and_crossing(gpu):
    cs.run_plan_model_says(gpu, SHAPES)


def test_plan_refusals_and_edges(gpu):
    cs.run_plan_refusals(gpu, SHAPES)


def test_plan_filters(gpu):
    cs.run_plan_filters(gpu, SHAPES)


@pytest.mark.parametrize("seed", range(SHAPES["sel_fuzz"][0]))
def test_plan_fuzz(gpu, seed):
    cs.run_plan_fuzz(gpu, SHAPES, seed)


def test_plan_start_offset_and_input_errors(gpu):
    cs.run_plan_offset_and_errors(gpu, SHAPES)


def test_select_keep_patterns(gpu):
    cs.run_select_patterns(gpu, SHAPES)


@pytest.mark.parametrize("n", SHAPES["counts"])
def test_select_record_counts(gpu, n):
    cs.run_select_count(gpu, SHAPES, n)


def test_select_titles_source_and_host_path(gpu):
    cs.run_select_titles(gpu, SHAPES)


def test_select_capacity(gpu):
    cs.run_select_capacity(gpu, SHAPES)


def test_select_start_offset_and_no_records(gpu):
    cs.run_select_offset(gpu, SHAPES)


def test_select_input_errors(gpu):
    cs.run_select_input_errors(gpu, SHAPES)


def test_closed_loop_through_torch(gpu):
    cs.run_closed_loop(gpu, SHAPES, "cuda:0")


def test_codec_state_is_left_alone(gpu):
    cs.run_codec_state(gpu, SHAPES)


def test_mates_stay_in_step(gpu):
    cs.run_mates(gpu, SHAPES, "cuda:0")
