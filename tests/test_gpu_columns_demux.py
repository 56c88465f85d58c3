"""Columnar demultiplex (dsrcgpu_columns_demux_plan, dsrcgpu_columns_partition_device; dsrc_amd/csrc/k_columns_demux.h) on the
MI355X: the product library, through the C ABI and both Python layers, compared with the integer model of
tests/columns_demux_cases.py -- the same cases as tests/test_emu_columns_demux.py, here with workgroups of 1024 threads, the full fuzz
and the record count that takes the planner's grid stride into a second round.  Exact equality throughout."""
import os

import pytest

from tests import columns_demux_cases as dx

SHAPES = dx.SHAPES["gpu"]
WG = SHAPES["wg"]

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    os.environ.pop("DSRC_GPU_LIB", None)
    from dsrc_amd import _lib
    _lib._lib = None
    return _lib


@pytest.mark.parametrize("length", dx.BARCODE_LENGTHS)
def test_geometry(gpu, length):
    dx.run_geometry(gpu, SHAPES, length)


@pytest.mark.parametrize("length", dx.BARCODE_LENGTHS)
def test_distance_exact_and_one_more(gpu, length):
    dx.run_distance(gpu, SHAPES, length)


def test_slot_budget(gpu):
    dx.run_slot_budget(gpu, SHAPES)


def test_choice(gpu):
    dx.run_choice(gpu, SHAPES)


@pytest.mark.parametrize("samples", dx.SAMPLE_COUNTS)
def test_sample_counts_and_winners(gpu, samples):
    dx.run_sample_counts(gpu, SHAPES, samples)


def test_plan_ranges_keep_in_place_info_and_counts(gpu):
    dx.run_plan(gpu, SHAPES)


def test_index_sets(gpu):
    dx.run_index_sets(gpu, SHAPES)


def test_argument_refusals(gpu):
    dx.run_arg_refusals(gpu, SHAPES)


def test_input_errors(gpu):
    dx.run_input_errors(gpu, SHAPES)


def test_codec_state_is_left_alone(gpu):
    dx.run_codec_state(gpu, SHAPES)


@pytest.mark.parametrize("n", [0] + SHAPES["counts"])
def test_record_counts(gpu, n):
    dx.run_count(gpu, SHAPES, n)


def test_grid_stride_second_round(gpu):
    dx.run_count(gpu, SHAPES, SHAPES["stride_count"])


def test_fuzz_exercises_every_statistic(gpu):
    dx.run_fuzz_exercises_everything(gpu, SHAPES)


@pytest.mark.parametrize("seed", range(SHAPES["demux_fuzz"][0]))
def test_fuzz(gpu, seed):
    dx.run_fuzz(gpu, SHAPES, seed)


@pytest.mark.parametrize("n", sorted({0, 1, WG - 1, WG, WG + 1, 2 * WG + 1} | set(SHAPES["counts"])))
def test_partition_tiles(gpu, n):
    dx.run_part_tiles(gpu, SHAPES, n)


@pytest.mark.parametrize("n_classes", [1, 2, 63, 64, 65, 1024])
def test_partition_classes(gpu, n_classes):
    dx.run_part_classes(gpu, SHAPES, n_classes)


def test_partition_patterns(gpu):
    dx.run_part_patterns(gpu, SHAPES)


def test_partition_refusals_capacities_and_errors(gpu):
    dx.run_part_refusals(gpu, SHAPES)


def test_demux_through_torch(gpu):
    dx.run_python_layers(gpu, SHAPES, "cuda:0")


def test_filter_columns_with_demux(gpu):
    dx.run_filter_columns(gpu, SHAPES, "cuda:0")


def test_filter_pairs_with_demux(gpu):
    dx.run_filter_pairs(gpu, SHAPES, "cuda:0")


def test_closed_loop_through_torch(gpu):
    dx.run_closed_loop(gpu, SHAPES, "cuda:0")
