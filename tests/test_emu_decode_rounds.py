"""Decode batches under a table budget on the CPU: run_decode's rounds, mixed quality alphabets and DNA schemes in one batch, several
passes on one handle, the other entry points (tests/decode_batch_cases.py) with the kernel sources compiled against the HIP
emulator in tests/emu.  These run the WAVE kernels (k_dec_qrc, k_dec_dnarc, k_dec_dna0), not the one-lane decoder most of
tests/test_emu_decode.py uses: that one sizes its own slots and never plans a round."""
import pytest

from tests import decode_batch_cases as bc
from tests.test_emu_kernels import emu  # noqa: F401  (fixture)

S = bc.SHAPES["emu"]


@pytest.mark.parametrize("dna_order,quality_order,lossy,budget", bc.TRIPLES)
def test_wave_budget_below_the_dna_table(emu, oracle, capfd, monkeypatch, dna_order, quality_order, lossy, budget):
    bc.run_overflow_triple(emu, oracle, S, capfd, monkeypatch, dna_order, quality_order, lossy, budget)


def test_wave_rounds_lossy(emu, oracle, capfd, monkeypatch):
    bc.run_rounds_lossy(emu, oracle, S, capfd, monkeypatch)


def test_wave_rounds_one_table_each(emu, oracle, capfd, monkeypatch):
    bc.run_rounds_one_table(emu, oracle, S, capfd, monkeypatch)


def test_wave_rounds_mixed_tables(emu, oracle, capfd, monkeypatch):
    bc.run_rounds_mixed(emu, oracle, S, capfd, monkeypatch)


@pytest.mark.parametrize("d,q,lossy,crc", bc.MIXED_LEVELS)
def test_wave_mixed_quality_alphabets(emu, oracle, capfd, monkeypatch, d, q, lossy, crc):
    bc.run_mixed_alphabets(emu, oracle, S, capfd, monkeypatch, d, q, lossy, crc)


@pytest.mark.parametrize("where", bc.DNA_ORDERS)
@pytest.mark.parametrize("d", [2, 3])
def test_wave_mixed_dna_schemes(emu, oracle, capfd, monkeypatch, d, where):
    bc.run_mixed_dna(emu, oracle, S, capfd, monkeypatch, d, where)


def test_wave_one_handle_several_passes(emu, oracle, capfd, monkeypatch):
    bc.run_handle_passes(emu, oracle, S, capfd, monkeypatch)


def test_wave_device_entry(emu, oracle, capfd, monkeypatch):
    bc.run_device_entry(emu, oracle, S, capfd, monkeypatch)


def test_wave_columns_entry(emu, oracle, capfd, monkeypatch):
    bc.run_columns_entry(emu, oracle, S, capfd, monkeypatch)


def test_wave_verifying_compress(emu, oracle, capfd, monkeypatch):
    bc.run_verifying_compress(emu, oracle, S, capfd, monkeypatch)


def test_wave_refusal_in_a_batch(emu, oracle, capfd, monkeypatch):
    bc.run_refusal_in_a_batch(emu, oracle, S, capfd, monkeypatch)


def test_serial_decoder_sizes_itself(emu, oracle, capfd, monkeypatch):
    bc.run_serial_decoder_sizes_itself(emu, oracle, S, capfd, monkeypatch)
