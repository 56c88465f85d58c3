"""Decode batches under a table budget on the GPU: run_decode's rounds, mixed quality alphabets and DNA schemes in one batch,
several passes on one handle, the other entry points (tests/decode_batch_cases.py) on the product library.  The library checks on
the host, before a round is filled, that every table of it lies inside the region (DSRCGPU_E_STATE otherwise)."""
import os

import pytest

from tests import decode_batch_cases as bc

pytestmark = pytest.mark.gpu

S = bc.SHAPES["gpu"]


@pytest.fixture(scope="module")
def gpu():
    os.environ.pop("DSRC_GPU_LIB", None)
    from dsrc_amd import _lib
    _lib._lib = None
    return _lib


@pytest.mark.parametrize("dna_order,quality_order,lossy,budget", bc.TRIPLES)
def test_budget_below_the_dna_table(gpu, oracle, capfd, monkeypatch, dna_order, quality_order, lossy, budget):
    bc.run_overflow_triple(gpu, oracle, S, capfd, monkeypatch, dna_order, quality_order, lossy, budget)


def test_rounds_lossy(gpu, oracle, capfd, monkeypatch):
    bc.run_rounds_lossy(gpu, oracle, S, capfd, monkeypatch)


def test_rounds_one_table_each(gpu, oracle, capfd, monkeypatch):
    bc.run_rounds_one_table(gpu, oracle, S, capfd, monkeypatch)


def test_rounds_mixed_tables(gpu, oracle, capfd, monkeypatch):
    bc.run_rounds_mixed(gpu, oracle, S, capfd, monkeypatch)


@pytest.mark.parametrize("d,q,lossy,crc", bc.MIXED_LEVELS)
def test_mixed_quality_alphabets(gpu, oracle, capfd, monkeypatch, d, q, lossy, crc):
    bc.run_mixed_alphabets(gpu, oracle, S, capfd, monkeypatch, d, q, lossy, crc)


@pytest.mark.parametrize("where", bc.DNA_ORDERS)
@pytest.mark.parametrize("d", [2, 3])
def test_mixed_dna_schemes(gpu, oracle, capfd, monkeypatch, d, where):
    bc.run_mixed_dna(gpu, oracle, S, capfd, monkeypatch, d, where)


def test_one_handle_several_passes(gpu, oracle, capfd, monkeypatch):
    bc.run_handle_passes(gpu, oracle, S, capfd, monkeypatch)


def test_device_entry(gpu, oracle, capfd, monkeypatch):
    bc.run_device_entry(gpu, oracle, S, capfd, monkeypatch)


def test_columns_entry(gpu, oracle, capfd, monkeypatch):
    bc.run_columns_entry(gpu, oracle, S, capfd, monkeypatch)


def test_verifying_compress(gpu, oracle, capfd, monkeypatch):
    bc.run_verifying_compress(gpu, oracle, S, capfd, monkeypatch)


def test_refusal_in_a_batch(gpu, oracle, capfd, monkeypatch):
    bc.run_refusal_in_a_batch(gpu, oracle, S, capfd, monkeypatch)


def test_serial_decoder_sizes_itself(gpu_hooks, oracle, capfd, monkeypatch):
    bc.run_serial_decoder_sizes_itself(gpu_hooks, oracle, S, capfd, monkeypatch)
