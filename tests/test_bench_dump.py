"""bench.py --dump-outputs on CPU tensors: what the last timed step handed its caller, as float .npy files that are the same
from run to run and stay within 64 MB."""
import os

import numpy as np
import torch

import bench


def _step(rng, n=5, frame_bytes=3000):
    sizes = rng.integers(1, 900, n).astype(np.uint32)
    out = torch.from_numpy(rng.integers(0, 256, int(sizes.sum()), dtype=np.uint8))
    dec = torch.from_numpy(rng.integers(0, 256, n * frame_bytes, dtype=np.uint8))
    return dict(out=out, sizes=sizes, ft=[0] + [1] * (n - 1), dec=dec)


def test_the_flag_is_parsed():
    assert bench.parse_args(["--dump-outputs", "d", "--steps", "7"]).dump_outputs == "d"
    assert bench.parse_args([]).dump_outputs is None


def test_dump_holds_the_last_steps_outputs(tmp_path):
    m = _step(np.random.default_rng(0))
    names = bench.dump_outputs(str(tmp_path), m)
    assert sorted(os.listdir(tmp_path)) == sorted(n + ".npy" for n in names)
    got = {n: np.load(os.path.join(tmp_path, n + ".npy")) for n in names}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    sizes, pk, dec = m["sizes"].astype(np.int64), m["out"].numpy(), m["dec"].numpy().reshape(len(m["sizes"]), -1)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    assert np.array_equal(got["packet_sizes"], sizes)
    assert np.array_equal(got["frame_types"], m["ft"])
    assert np.array_equal(got["packet_byte_sums"], [int(pk[a:b].sum()) for a, b in zip(offs[:-1], offs[1:])])
    assert np.array_equal(got["packet_bytes_sample"], pk)  # small outputs are kept whole
    assert np.array_equal(got["decoded_frame_byte_sums"], dec.sum(1))
    assert np.array_equal(got["decoded_bytes_sample"], dec.reshape(-1))


def test_large_outputs_are_a_fixed_sample_within_64_mb(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 1000)
    m = _step(np.random.default_rng(1), n=20, frame_bytes=4000)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), m)
    for name in os.listdir(tmp_path / "a"):
        assert np.array_equal(np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name))
    s = np.load(tmp_path / "a" / "decoded_bytes_sample.npy")
    idx = bench._sample_index(m["dec"].numel(), 2)
    assert s.size == 1000 and np.array_equal(s, m["dec"].numpy()[idx])
    monkeypatch.undo()
    assert 2 * bench.DUMP_SAMPLE * 4 + 8 * 4 * 1200 < 64 << 20  # the two samples + four per-frame float64 arrays of a 1200-frame run
