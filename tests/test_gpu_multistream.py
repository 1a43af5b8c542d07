"""GPU tests (-m gpu) of scpr_decompress_streams (codec.decompress_streams): many codecs' streams decoded with their GOPs side by side
in shared launches must be observably the same as scpr_decompress_batch on every codec in turn - results, pictures, and the state
each codec is left in.  Every picture against the input (the streams are lossless) and the oracle's decoder."""
import ctypes as C
import importlib.util
import json
import os

import numpy as np
import pytest

import oracle_api as O
from screenpressor_amd.synth import DesktopSequence, pack24

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class Stream:
    """one encoded stream: packets, frame types, the input rows and the oracle's decoded pictures at the decode pitch"""

    def __init__(self, w, h, bpp, n, keys, seed, workers=1, version=4, pitch=None):
        self.w, self.h, self.bpp, self.n, self.workers, self.version = w, h, bpp, n, workers, version
        self.rowbytes = w * (bpp // 8)
        self.pitch = pitch if pitch is not None else (w * 4 if bpp == 32 else (self.rowbytes + 3) & ~3)
        seq = DesktopSequence(w, h, seed=seed, sparkles=20)
        frames = []
        for t in range(n):
            if bpp == 32:
                f = seq.frame(t)
            elif bpp == 24:
                f = pack24(seq.frame24(t))
            else:  # RGB16 555, rows back to back (screencap.cpp:1668)
                c = seq.frame24(t).astype(np.uint16) >> 3
                f = ((c[..., 2] << 10) | (c[..., 1] << 5) | c[..., 0]).astype(np.uint16).view(np.uint8).reshape(h, w * 2)
            frames.append(np.ascontiguousarray(f))
        self.rows = np.stack([np.asarray(f).reshape(h, -1)[:, : self.rowbytes] for f in frames])
        enc = O.OracleCodec(w, h, bpp, workers=workers, version=version)
        ref = [enc.compress(f, key=(t in keys)) for t, f in enumerate(frames)]
        self.packets = [p for p, _ in ref]
        self.ftypes = [ft for _, ft in ref]
        dec = O.OracleCodec(w, h, bpp, version=version)
        outs = []
        for p, ft in zip(self.packets, self.ftypes):
            r, out = dec.decompress(p, ft, self.pitch)
            assert r == 1
            outs.append(out.reshape(h, self.pitch)[:, : self.rowbytes])
        self.oracle = np.stack(outs)
        assert np.array_equal(self.oracle, self.rows)  # (lossless: the oracle's pictures are the input)

    def codec(self):
        from screenpressor_amd.codec import ScreenCodec
        return ScreenCodec(0).Init(self.w, self.h, self.bpp, workers=self.workers)

    def blob(self, a, b):
        import torch
        data = b"".join(self.packets[a:b])
        return torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda() if data else torch.zeros(1, dtype=torch.uint8, device="cuda")

    def entry(self, codec, a, b):
        import torch
        out = torch.zeros(max((b - a) * self.pitch * self.h, 1), dtype=torch.uint8, device="cuda")
        return (codec, self.blob(a, b), [len(p) for p in self.packets[a:b]], self.ftypes[a:b], self.pitch, out)

    def pictures(self, out, k):
        return out[: k * self.pitch * self.h].cpu().numpy().reshape(k, self.h, self.pitch)[:, :, : self.rowbytes]

    def exact(self, out, a, b):
        got = self.pictures(out, b - a)
        return np.array_equal(got, self.rows[a:b]) and np.array_equal(got, self.oracle[a:b])


def serial(entry):
    """scpr_decompress_batch on one entry, its raw result (an error is a value here, as in decompress_streams)"""
    import torch
    codec, packets, sizes, ftypes, pitch, out = entry
    k = len(sizes)
    torch.cuda.synchronize()
    r = codec._L.scpr_decompress_batch(codec._h, C.c_void_p(packets.data_ptr()), (C.c_uint32 * max(k, 1))(*sizes), (C.c_int * max(k, 1))(*ftypes), k,
                                       C.c_void_p(out.data_ptr()), pitch)
    return r, out


_STREAMS = None


def streams():
    """the six streams of the mixed call (built once): 1080p RGB32 one GOP; 640x480 RGB24 at pitch = stride, keys every 5;
    100x37 RGB24 at a foreign pitch; 33x21 RGB16; 1030x40 with 4 workers, keys only; a version 3 stream"""
    global _STREAMS
    if _STREAMS is None:
        _STREAMS = [Stream(1920, 1080, 32, 4, {0}, 1),
                    Stream(640, 480, 24, 12, {0, 5, 10}, 2),
                    Stream(100, 37, 24, 9, {0, 4}, 3, pitch=333),
                    Stream(33, 21, 16, 8, {0, 5}, 4),
                    Stream(1030, 40, 32, 6, set(range(6)), 5, workers=4),
                    Stream(200, 64, 32, 8, {0, 6}, 6, version=3)]
    return _STREAMS


# three consecutive calls of uneven sizes per stream (one entry of 0 frames)
SPLITS = [[2, 0, 2], [5, 4, 3], [0, 6, 3], [3, 3, 2], [1, 4, 1], [4, 1, 3]]


def _cuts(split):
    c = [0]
    for k in split:
        c.append(c[-1] + k)
    return c


def test_mixed_streams_over_several_calls_equal_the_serial_path():
    from screenpressor_amd.codec import decompress_streams
    ss = streams()
    multi = [s.codec() for s in ss]
    twins = [s.codec() for s in ss]
    for call in range(3):
        entries, twin_entries = [], []
        for s, m, t, split in zip(ss, multi, twins, SPLITS):
            c = _cuts(split)
            entries.append(s.entry(m, c[call], c[call + 1]))
            twin_entries.append(s.entry(t, c[call], c[call + 1]))
        res = decompress_streams(entries)
        for i, (s, split, (r, out), te) in enumerate(zip(ss, SPLITS, res, twin_entries)):
            c = _cuts(split)
            assert r == split[call], (i, call, r)
            assert s.exact(out, c[call], c[call + 1]), (i, call)
            rt, tout = serial(te)
            assert rt == r and np.array_equal(s.pictures(tout, split[call]), s.pictures(out, split[call])), (i, call)
    # a call whose first frame is a P-frame on a fresh codec: nothing decoded, on both paths
    s = ss[1]
    fresh, fresh_twin = s.codec(), s.codec()
    (r, _), = decompress_streams([s.entry(fresh, 1, 3)])
    rt, _ = serial(s.entry(fresh_twin, 1, 3))
    assert r == rt == 0


@pytest.mark.parametrize("damage", ["flip", "truncate"])
def test_a_damaged_stream_stays_isolated(damage):
    """one stream's third packet damaged (as corrupt_shape in stress_cases.py does): its result and pictures equal its serial twin's,
    the other streams stay exact, and a further call on every codec behaves as on the twins"""
    import torch
    from screenpressor_amd.codec import decompress_streams
    ss = streams()
    victim = 1
    bad = Stream.__new__(Stream)
    bad.__dict__.update(ss[victim].__dict__)
    pk = bytearray(bad.packets[2])
    if damage == "flip":
        rng = np.random.default_rng(77)
        for _ in range(5):
            pk[int(rng.integers(1, len(pk)))] ^= int(rng.integers(1, 256))
    else:
        pk = pk[: max(1, len(pk) // 3)]
    bad.packets = list(bad.packets)
    bad.packets[2] = bytes(pk)
    used = [bad if i == victim else s for i, s in enumerate(ss)]
    multi = [s.codec() for s in used]
    twins = [s.codec() for s in used]
    for a, b in ((0, None), (None, None)):  # the first n - 2 frames, then the last two
        entries, twin_entries = [], []
        for s, m, t in zip(used, multi, twins):
            lo, hi = (0, s.n - 2) if a == 0 else (s.n - 2, s.n)
            entries.append(s.entry(m, lo, hi))
            twin_entries.append(s.entry(t, lo, hi))
        res = decompress_streams(entries)
        for i, (s, (r, out), te) in enumerate(zip(used, res, twin_entries)):
            lo, hi = (0, s.n - 2) if a == 0 else (s.n - 2, s.n)
            rt, tout = serial(te)
            assert r == rt, (i, r, rt)
            assert torch.equal(out, tout), i
            if i != victim:
                assert r == hi - lo and s.exact(out, lo, hi), i


def _golden_v2():
    m = json.load(open(os.path.join(GOLD, "manifest.json")))["desktop_100x37_v2_ip"]
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(GOLD, "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    case = [c for c in mg.CASES_ALL if c[0] == "desktop_100x37_v2_ip"][0]
    frames = np.stack([np.asarray(f) for _, f in mg.frames_of(case)])
    return m, open(os.path.join(GOLD, m["file"]), "rb").read(), frames


def test_version2_golden_stream_beside_version4_streams():
    import torch
    from screenpressor_amd.codec import ScreenCodec, decompress_streams
    m, blob, frames = _golden_v2()
    ss = streams()
    v2, v2_twin = ScreenCodec(0).Init(m["width"], m["height"], 32), ScreenCodec(0).Init(m["width"], m["height"], 32)
    n = m["frames"]
    pk = torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).cuda()
    others = [ss[2], ss[3]]
    entries = [(v2, pk, m["sizes"], m["ftypes"], None, torch.zeros(n * m["width"] * 4 * m["height"], dtype=torch.uint8, device="cuda"))]
    entries += [s.entry(s.codec(), 0, s.n) for s in others]
    res = decompress_streams(entries)
    r, out = res[0]
    assert r == n
    got = out.cpu().numpy().reshape(frames.shape)
    assert np.array_equal(got[..., :3], frames[..., :3])
    rt, tout = serial((v2_twin, pk, m["sizes"], m["ftypes"], m["width"] * 4, torch.zeros_like(out)))
    assert rt == n and torch.equal(out, tout)
    for s, (r, out) in zip(others, res[1:]):
        assert r == s.n and s.exact(out, 0, s.n)


def test_arena_second_attempt(monkeypatch):
    """SCPR_DEBUG_DEC_ARENA (read per call) makes every fresh chunk's estimate too small: those chunks are decoded again with the true
    bound, and every picture is still exact"""
    from screenpressor_amd.codec import decompress_streams
    ss = streams()
    codecs = [s.codec() for s in ss]
    monkeypatch.setenv("SCPR_DEBUG_DEC_ARENA", "1")
    res = decompress_streams([s.entry(c, 0, s.n - 3) for s, c in zip(ss, codecs)])
    for i, (s, (r, out)) in enumerate(zip(ss, res)):
        assert r == s.n - 3 and s.exact(out, 0, s.n - 3), i
    monkeypatch.delenv("SCPR_DEBUG_DEC_ARENA")
    res = decompress_streams([s.entry(c, s.n - 3, s.n) for s, c in zip(ss, codecs)])
    for i, (s, (r, out)) in enumerate(zip(ss, res)):
        assert r == 3 and s.exact(out, s.n - 3, s.n), i


def test_whole_call_refusals_touch_nothing():
    """a duplicate codec, a codec never initialised, a NULL pointer: SCPR_E_PARAM, and afterwards every codec decodes its stream as if
    the refused call had never been made"""
    import torch
    from screenpressor_amd.codec import ScreenCodec, ScprDecodeCall, decompress_streams, load_library
    ss = streams()[1:4]
    codecs = [s.codec() for s in ss]
    res = decompress_streams([s.entry(c, 0, 2) for s, c in zip(ss, codecs)])
    assert [r for r, _ in res] == [2, 2, 2]
    later = [s.entry(c, 2, s.n) for s, c in zip(ss, codecs)]
    with pytest.raises(RuntimeError):  # the same codec twice
        decompress_streams(later + [ss[0].entry(codecs[0], 2, ss[0].n)])
    with pytest.raises(RuntimeError):  # a codec never initialised
        decompress_streams(later + [(ScreenCodec(0), torch.zeros(4, dtype=torch.uint8, device="cuda"), [4], [0], 4, torch.zeros(4, dtype=torch.uint8, device="cuda"))])
    L = load_library()
    arr = (ScprDecodeCall * len(later))()
    keep = []
    for i, (codec, packets, sizes, ftypes, pitch, out) in enumerate(later):
        sz, ft = (C.c_uint32 * len(sizes))(*sizes), (C.c_int * len(ftypes))(*ftypes)
        keep += [sz, ft]
        arr[i] = ScprDecodeCall(codec._h, packets.data_ptr(), sz, ft, len(sizes), None if i == 1 else out.data_ptr(), pitch, 99)
    torch.cuda.synchronize()
    assert L.scpr_decompress_streams(arr, len(later)) == -2  # (entry 1: no output buffer)
    assert [arr[i].result for i in range(len(later))] == [99] * len(later)
    assert all(int(out.count_nonzero()) == 0 for _, _, _, _, _, out in later)
    res = decompress_streams(later)
    for i, (s, (r, out)) in enumerate(zip(ss, res)):
        assert r == s.n - 2 and s.exact(out, 2, s.n), i


def test_more_gops_than_one_launch_holds():
    """300 small codecs of three GOPs each (900 GOPs: more than the 768 of one launch) in one call"""
    from screenpressor_amd.codec import decompress_streams
    kinds = [Stream(64, 48, 32, 6, {0, 2, 4}, 100 + k) for k in range(25)]
    used = [kinds[i % len(kinds)] for i in range(300)]
    res = decompress_streams([s.entry(s.codec(), 0, s.n) for s in used])
    for i, (s, (r, out)) in enumerate(zip(used, res)):
        assert r == s.n and s.exact(out, 0, s.n), i
