"""bench.py --dump-outputs (CPU, no GPU): dump_outputs writes the per-block tables of every scheduler instance's last call whole,
and of the block bytes a fixed seeded sample of whole blocks within DUMP_BYTES; float32 / float64 only, the same files for the same
outputs."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    return m


class _Handle:
    """dev_download over a host buffer that stands for the device."""

    def __init__(self, mem):
        self.mem = mem

    def dev_download(self, ptr, n):
        assert 0 <= ptr and ptr + n <= len(self.mem)
        return bytes(self.mem[ptr: ptr + n])


class _Lane:
    def __init__(self, rng, n_blocks, base):
        sizes = [int(x) for x in rng.integers(1000, 5000, n_blocks)]
        offs = [int(x) for x in np.concatenate([[0], np.cumsum(sizes)[:-1]])]
        self.mem = rng.integers(0, 256, base + sum(sizes), dtype=np.uint8).tobytes()
        self.h = _Handle(self.mem)
        self.outs = [(base, None), (base + 7, None)]
        raw = [int(x) for x in rng.integers(1, 1 << 20, 4 * n_blocks)]
        comp = [int(x) for x in rng.integers(1, 1 << 20, 4 * n_blocks)]
        self.results = {4: (offs, sizes, raw, comp)}       # step 4 uses self.outs[0]


def test_dump_outputs(tmp_path, monkeypatch):
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_BYTES", 20000)
    rng = np.random.default_rng(5)
    lanes = [_Lane(rng, 9, 64), _Lane(rng, 6, 128)]
    bench.dump_outputs(str(tmp_path / "a"), lanes, 4)
    bench.dump_outputs(str(tmp_path / "b"), lanes, 4)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    got = {n[:-4]: np.load(tmp_path / "a" / n) for n in names}
    for n in names:
        assert np.array_equal(got[n[:-4]], np.load(tmp_path / "b" / n))
        assert got[n[:-4]].dtype in (np.float32, np.float64)
    offs = [o for ln in lanes for o in ln.results[4][0]]
    sizes = [s for ln in lanes for s in ln.results[4][1]]
    assert got["block_offsets"].tolist() == offs and got["block_sizes"].tolist() == sizes
    assert got["raw_sizes"].shape == (15, 4) and got["raw_sizes"].ravel().tolist() == [x for ln in lanes for x in ln.results[4][2]]
    assert got["comp_sizes"].ravel().tolist() == [x for ln in lanes for x in ln.results[4][3]]
    # the sample: distinct blocks, whole but for the last, DUMP_BYTES in all, each the bytes its caller's buffer holds
    picked = [int(i) for i in got["sample_blocks"]]
    assert len(set(picked)) == len(picked) and got["sample_bytes"].size == 20000
    assert sum(sizes[i] for i in picked[:-1]) < 20000 <= sum(sizes[i] for i in picked)
    where = [(ln, ln.outs[0][0] + o) for ln in lanes for o in ln.results[4][0]]
    at = 0
    for i in picked:
        ln, ptr = where[i]
        n = min(sizes[i], 20000 - at)
        assert got["sample_bytes"][at: at + n].astype(np.uint8).tobytes() == ln.mem[ptr: ptr + n]
        at += n
