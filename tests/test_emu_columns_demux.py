"""Columnar demultiplex (dsrcgpu_columns_demux_plan, dsrcgpu_columns_partition_device; dsrc_amd/csrc/k_columns_demux.h) on the CPU:
the kernel sources compiled against the HIP emulator in tests/emu (workgroups of 256 threads), driven through the C ABI and both
Python layers, and compared with the integer model of tests/columns_demux_cases.py.  Exact equality throughout."""
import os
import subprocess

import pytest

from tests import columns_demux_cases as dx

SHAPES = dx.SHAPES["emu"]
WG = SHAPES["wg"]

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
    dx.run_model_forms(emu, SHAPES)


@pytest.mark.parametrize("length", dx.BARCODE_LENGTHS)
def test_geometry(emu, length):
    dx.run_geometry(emu, SHAPES, length)


@pytest.mark.parametrize("length", dx.BARCODE_LENGTHS)
def test_distance_exact_and_one_more(emu, length):
    dx.run_distance(emu, SHAPES, length)


def test_slot_budget(emu):
    dx.run_slot_budget(emu, SHAPES)


def test_choice(emu):
    dx.run_choice(emu, SHAPES)


@pytest.mark.parametrize("samples", dx.SAMPLE_COUNTS)
def test_sample_counts_and_winners(emu, samples):
    dx.run_sample_counts(emu, SHAPES, samples)


def test_plan_ranges_keep_in_place_info_and_counts(emu):
    dx.run_plan(emu, SHAPES)


def test_index_sets(emu):
    dx.run_index_sets(emu, SHAPES)


def test_argument_refusals(emu):
    dx.run_arg_refusals(emu, SHAPES)


def test_input_errors(emu):
    dx.run_input_errors(emu, SHAPES)


def test_codec_state_is_left_alone(emu):
    dx.run_codec_state(emu, SHAPES)


@pytest.mark.parametrize("n", [0] + SHAPES["counts"])
def test_record_counts(emu, n):
    dx.run_count(emu, SHAPES, n)


def test_fuzz_exercises_every_statistic(emu):
    dx.run_fuzz_exercises_everything(emu, SHAPES)


@pytest.mark.parametrize("seed", range(SHAPES["demux_fuzz"][0]))
def test_fuzz(emu, seed):
    dx.run_fuzz(emu, SHAPES, seed)


@pytest.mark.parametrize("n", sorted({0, 1, WG - 1, WG, WG + 1, 2 * WG + 1} | set(SHAPES["counts"])))
def test_partition_tiles(emu, n):
    dx.run_part_tiles(emu, SHAPES, n)


@pytest.mark.parametrize("n_classes", [1, 2, 63, 64, 65, 1024])
def test_partition_classes(emu, n_classes):
    dx.run_part_classes(emu, SHAPES, n_classes)


def test_partition_patterns(emu):
    dx.run_part_patterns(emu, SHAPES)


def test_partition_refusals_capacities_and_errors(emu):
    dx.run_part_refusals(emu, SHAPES)


def test_demux_through_torch(emu):
    dx.run_python_layers(emu, SHAPES, "cpu")


def test_filter_columns_with_demux(emu):
    dx.run_filter_columns(emu, SHAPES, "cpu")


def test_filter_pairs_with_demux(emu):
    dx.run_filter_pairs(emu, SHAPES, "cpu")


def test_closed_loop_through_torch(emu):
    dx.run_closed_loop(emu, SHAPES, "cpu")
