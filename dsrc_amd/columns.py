"""Records as torch tensors: decode_columns (dsrcgpu_decompress_batch_columns_device) and the way back, encode_columns
(dsrcgpu_compress_columns_device), include/dsrc_gpu.h.

The blocks are already in device memory; the arrays are allocated by torch on the same device and filled by the library's
kernels -- no text, no host round trip of the payload.  With the emulator build of the library (tests/emu) device pointers
are host pointers, so CPU tensors work there.

Import this module (or torch) before the first Handle is created: a torch wheel that bundles its own HIP runtime finds no
device when another copy of the runtime -- the one libdsrc_gpu.so is linked to -- is already in the process; loaded after
torch, the library shares torch's copy (bench.py and dsrc_amd/dist.py work the same way).
"""
from __future__ import annotations

import dataclasses

import torch

from . import _lib


@dataclasses.dataclass
class RecordColumns:
    bases: torch.Tensor            # uint8, one code per base: index in "ACGTNRWSKMDVHBYXU.-", 255 = any other byte
    quals: torch.Tensor            # uint8, quality character - quality offset, same positions as bases
    titles: torch.Tensor           # uint8, title lines back to back ('@' included, no newline); empty when titles=False
    seq_offsets: torch.Tensor      # int64, records + 1: record r's bases and qualities are [seq_offsets[r], seq_offsets[r + 1])
    title_offsets: torch.Tensor    # int64, records + 1; empty when titles=False
    block_records: torch.Tensor    # int64, blocks + 1: exclusive prefix of the records per block

    @property
    def n_records(self) -> int:
        return self.seq_offsets.numel() - 1


def decode_columns(handle: _lib.Handle, d_blocks, offs, sizes, device, titles: bool = True) -> RecordColumns:
    """Decode the blocks d_blocks[offs[i] : offs[i] + sizes[i]] (a uint8 tensor on `device`, or a device address) into
    RecordColumns on `device`.  The first library call only sizes the arrays (capacities of zero), the second one decodes."""
    device = torch.device(device)
    d_in = d_blocks.data_ptr() if isinstance(d_blocks, torch.Tensor) else int(d_blocks)
    offs = [int(o) for o in offs]; sizes = [int(s) for s in sizes]

    def quiesce():
        # the library works on its own stream and returns only after synchronising it: memory the allocator has just handed
        # out again (and the blocks themselves) must not have work of torch's stream pending on it
        if device.type == "cuda":
            torch.cuda.current_stream(device).synchronize()

    need = [0, 0, 0]
    if offs:
        quiesce()
        try:
            handle.decompress_columns_device(d_in, offs, sizes, _lib.Columns())
        except _lib.DsrcGpuError as e:
            if e.code != _lib.E_CAPACITY or not any(e.need):      # (all zero: it is a block's text that does not fit)
                raise
            need = e.need
    n_recs, n_bases, n_title = need
    u8 = dict(dtype=torch.uint8, device=device); i64 = dict(dtype=torch.int64, device=device)
    bases = torch.empty(n_bases, **u8); quals = torch.empty(n_bases, **u8)
    seq_offsets = torch.empty(n_recs + 1, **i64)
    title_bytes = torch.empty(n_title if titles else 0, **u8)
    title_offsets = torch.empty(n_recs + 1 if titles else 0, **i64)
    # (data_ptr() of an empty tensor is null: one spare byte keeps "titles wanted, none there" apart from "not wanted")
    spare = torch.empty(8, **u8)
    ptr = lambda t: t.data_ptr() if t.numel() else spare.data_ptr()
    cols = _lib.Columns(ptr(bases), n_bases, ptr(quals), n_bases, ptr(title_bytes) if titles else None, n_title if titles else 0,
                        seq_offsets.data_ptr(), title_offsets.data_ptr() if titles else None, n_recs)
    quiesce()
    block_records, totals = handle.decompress_columns_device(d_in, offs, sizes, cols)
    assert totals == need
    return RecordColumns(bases, quals, title_bytes, seq_offsets, title_offsets, torch.tensor(block_records, **i64))


def encode_columns(handle: _lib.Handle, cols: RecordColumns, block_records=None, chunk_bytes: int = 8 << 20):
    """Compress the records of `cols` (tensors on one device, as decode_columns returns them) into DSRC blocks on that device:
    -> (blocks: uint8 tensor, offs, sizes, block_records); block i is blocks[offs[i] : offs[i] + sizes[i]] and holds records
    block_records[i] .. block_records[i + 1] - 1.  block_records=None: the greedy cut of dsrcgpu_columns_cut at chunk_bytes of
    chunk text per block.  No text is written by the caller and nothing of the payload crosses to the host."""
    device = cols.bases.device
    R = cols.n_records
    if cols.title_offsets.numel() != R + 1:
        raise ValueError("encode_columns needs the titles (decode_columns(..., titles=True))")

    def quiesce():       # as in decode_columns: the library works on its own stream
        if device.type == "cuda":
            torch.cuda.current_stream(device).synchronize()

    spare = torch.empty(8, dtype=torch.uint8, device=device)
    ptr = lambda t: t.data_ptr() if t.numel() else spare.data_ptr()
    held = [t.contiguous() for t in (cols.bases, cols.quals, cols.titles, cols.seq_offsets, cols.title_offsets)]
    bases, quals, titles, seq_offs, title_offs = held
    cin = _lib.ColumnsIn(ptr(bases), bases.numel(), ptr(quals), ptr(titles), titles.numel(), seq_offs.data_ptr(), title_offs.data_ptr(), R)
    if block_records is None:
        quiesce()
        block_records = handle.columns_cut(cin, chunk_bytes)
    block_records = [int(v) for v in (block_records.tolist() if isinstance(block_records, torch.Tensor) else block_records)]
    n = len(block_records) - 1
    # (the text: two bytes a base, the title at most twice, six more a record; a block is not larger than its text + 64 KiB)
    cap = 2 * bases.numel() + 2 * titles.numel() + 6 * R + n * (1 << 16) + 64
    blocks = torch.empty(cap, dtype=torch.uint8, device=device)
    quiesce()
    offs, sizes, _, _ = handle.compress_columns_device(cin, block_records, blocks.data_ptr(), cap)
    return blocks, offs, sizes, block_records
