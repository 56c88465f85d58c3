#!/usr/bin/env python3
"""What the columnar demultiplex costs: 2^20 reads of 150 bases as tensors on the device (random bases drawn by torch -- not the
device generator: the barcodes have to be planted anyway, and nothing here depends on the bases behind them), every read with one
of S sample barcodes in front -- 88 % exact, 10 % with one substitution, 2 % random.  Timed on those tensors, with the classes and
the partition's bytes compared with a composition of torch ops and of select_columns first:
  demux_plan            8-base inline barcodes at 8 / 96 / 384 / 1023 samples; 8 + 8 dual index from two index sets at 96 and 384
  partition_columns     the result of each, at the same sample counts
  trim_plan, adapter_plan on the same columns; select_columns with keep-all (what a partition cannot beat)
  S x select_columns    keep = classes == s, at S = 8 and 96 (what the partition replaces)
  torch assignment      chunked broadcast compare and two mins
One warm-up and --steps timed calls each (at least 5), host wall time around the synchronous call as min / median / max.
A timing tool, not a gate.  With the emulator build of the library (DSRC_GPU_LIB, --device cpu, --reads 2000) it runs end to end
and the figures mean nothing.  Results go to profiles/."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402  (before the first handle: dsrc_amd/columns.py)
from columns_adapter_bench import ADAPTERS  # noqa: E402
from columns_filter_bench import timed  # noqa: E402
from dsrc_amd import _lib, columns  # noqa: E402
from dsrc_amd.config import Config  # noqa: E402


def ms(secs):
    v = sorted(s * 1e3 for s in secs)
    return {"min": round(v[0], 3), "median": round(statistics.median(v), 3), "max": round(v[-1], 3)}


def barcodes(S, lens, g):
    """S distinct samples: per slot a (S, len) tensor of codes."""
    while True:
        slots = [torch.randint(0, 4, (S, L), generator=g, dtype=torch.uint8) for L in lens]
        if torch.unique(torch.cat(slots, 1), dim=0).shape[0] == S:
            return slots


def spoil(B, which, g):
    """The barcode of sample which[r] for every record: 10 % with one substitution, 2 % random."""
    n, L = which.numel(), B.shape[1]
    X = B[which].clone()
    u = torch.rand(n, generator=g)
    sub = torch.nonzero((u >= 0.88) & (u < 0.98))[:, 0]
    at = torch.randint(0, L, (sub.numel(),), generator=g)
    X[sub, at] = (X[sub, at] + torch.randint(1, 4, (sub.numel(),), generator=g, dtype=torch.uint8)) % 4
    rnd = torch.nonzero(u >= 0.98)[:, 0]
    X[rnd] = torch.randint(0, 4, (rnd.numel(), L), generator=g, dtype=torch.uint8)
    return X


def fixed_columns(bases, device, title=b"@read/01"):
    n, L = bases.shape
    t = torch.tensor(list(title), dtype=torch.uint8).repeat(n)
    return columns.RecordColumns(bases.reshape(-1).to(device), torch.full((n * L,), 30, dtype=torch.uint8, device=device), t.to(device),
                                 (torch.arange(n + 1, dtype=torch.int64) * L).to(device), (torch.arange(n + 1, dtype=torch.int64) * len(title)).to(device),
                                 torch.tensor([0, n], dtype=torch.int64, device=device))


def torch_assign(windows, slots, max_mismatches, min_delta, chunk=8192):
    """The planner's rule in torch ops: per chunk of records a broadcast compare against every sample, the first minimum, the minimum
    of the rest -> classes (the unassigned class is S)."""
    S = slots[0].shape[0]
    out = []
    for i in range(0, windows[0].shape[0], chunk):
        d = sum((X[i: i + chunk, None, :] != B[None, :, :]).sum(2) for X, B in zip(windows, slots))
        best, at = d.min(1)
        rest = d.scatter(1, at[:, None], 255)
        second = rest.min(1).values if S > 1 else torch.full_like(best, 255)
        out.append(torch.where((best <= max_mismatches) & (second - best >= min_delta), at, torch.full_like(at, S)))
    return torch.cat(out).to(torch.int32)


def run(n, read_len, steps, device, out_path):
    g = torch.Generator(device="cpu"); g.manual_seed(24)
    cfg = Config.from_levels(0, 0)
    h = _lib.Handle(cfg.dna_order, cfg.quality_order, cfg.lossy, cfg.crc)
    out = {"case": "columnar demultiplex, device-resident tensors", "reads": n, "read_length": read_len, "steps": steps,
           "figures": "host wall time in ms around the synchronous call of dsrc_amd/columns.py (torch's allocation of the outputs included)",
           "shape": "the planner stages 64 records a wave and compares a record a lane (dsrc_amd/csrc/k_columns_demux.h)", "legs": {}}
    try:
        body = torch.randint(0, 4, (n, read_len), generator=g, dtype=torch.uint8)
        for S in (8, 96, 384, 1023):
            slots = barcodes(S, [8], g)
            which = torch.randint(0, S, (n,), generator=g)
            reads = body.clone(); reads[:, :8] = spoil(slots[0], which, g)
            cols = fixed_columns(reads, device)
            names = ["".join("ACGT"[v] for v in row) for row in slots[0].tolist()]
            kw = dict(max_mismatches=1, min_delta=1, min_length=1)
            secs, (b, e, k, c, stats) = timed(device, steps, lambda: columns.demux_plan(h, cols, names, **kw))
            want = torch_assign([cols.bases.view(n, read_len)[:, :8]], [slots[0].to(device)], 1, 1)
            assert torch.equal(c, want), "the torch rule and the library disagree on a class"
            leg = {"demux_plan": ms(secs), "assigned": stats["records_assigned"], "kept": stats["records_kept"]}
            secs, _ = timed(device, steps, lambda: torch_assign([cols.bases.view(n, read_len)[:, :8]], [slots[0].to(device)], 1, 1))
            leg["torch_assignment"] = ms(secs)
            secs, parts = timed(device, steps, lambda: columns.partition_columns(h, cols, c, S, b, e, k))
            leg["partition_columns"] = ms(secs)
            if S in (8, 96):
                def selects():
                    return [columns.select_columns(h, cols, b, e, k & (c == s).to(torch.uint8)) for s in range(S)]
                secs, sel = timed(device, steps, selects)
                leg["S_selects"] = ms(secs)
                assert torch.equal(torch.cat([x.bases for x in sel]), parts.bases) and torch.equal(torch.cat([x.quals for x in sel]), parts.quals)
                assert torch.equal(torch.cat([x.titles for x in sel]), parts.titles) and [x.n_records for x in sel] == parts.block_records.diff().tolist()
            if S == 8:
                secs, _ = timed(device, steps, lambda: columns.trim_plan(h, cols, quality_5=20, quality_3=20, min_length=1))
                out["trim_plan_both_ends"] = ms(secs)
                secs, _ = timed(device, steps, lambda: columns.adapter_plan(h, cols, ADAPTERS[:1]))
                out["adapter_plan_1"] = ms(secs)
                secs, _ = timed(device, steps, lambda: columns.select_columns(h, cols))
                out["select_columns_keep_all"] = ms(secs)
            out["legs"]["inline_8_S%d" % S] = leg
            del cols, reads, parts
        cols = fixed_columns(body, device)
        for S in (96, 384):
            slots = barcodes(S, [8, 8], g)
            which = torch.randint(0, S, (n,), generator=g)
            index = [fixed_columns(spoil(B, which, g), device) for B in slots]
            names = ["".join("ACGT"[v] for v in r0) + "+" + "".join("ACGT"[v] for v in r1) for r0, r1 in zip(slots[0].tolist(), slots[1].tolist())]
            secs, (b, e, k, c, stats) = timed(device, steps, lambda: columns.demux_plan(h, cols, names, index=index, max_mismatches=1, min_delta=1))
            want = torch_assign([x.bases.view(n, 8) for x in index], [B.to(device) for B in slots], 1, 1)
            assert torch.equal(c, want), "the torch rule and the library disagree on a class"
            leg = {"demux_plan": ms(secs), "assigned": stats["records_assigned"]}
            if stats["records_assigned"] < n // 2:
                raise AssertionError("too few records assigned")
            secs, parts = timed(device, steps, lambda: columns.partition_columns(h, cols, c, S, b, e, k))
            leg["partition_columns"] = ms(secs)
            assert parts.n_records == stats["records_kept"]
            out["legs"]["dual_8_8_S%d" % S] = leg
    finally:
        h.close()
    print(json.dumps(out), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write(json.dumps(out) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reads", type=int, default=1 << 20)
    ap.add_argument("--read-length", type=int, default=150)
    ap.add_argument("--steps", type=int, default=5, help="timed calls (at least 5: the spread is min..max)")
    ap.add_argument("--device", default="cuda:0", help="torch device of the arrays (cpu with the emulator build)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_columns_demux_bench.json"))
    a = ap.parse_args()
    run(a.reads, a.read_length, max(a.steps, 5), torch.device(a.device), a.out)


if __name__ == "__main__":
    main()
